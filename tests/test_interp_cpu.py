"""CPU-side checks of the interpolated demapper's surface: the CLI flag, the `demapper` keyword's
validation (before any device is touched) and the well-formedness of tests/golden/interp.npz."""
import re

import numpy as np
import pytest

from conftest import golden


def test_cli_parses_demapper():
    from qamr.sim_reconciliation import build_parser

    p = build_parser()
    assert p.parse_args(["edges.csv"]).demapper == "search"
    assert p.parse_args(["edges.csv", "--demapper", "search"]).demapper == "search"
    assert p.parse_args(["edges.csv", "--demapper", "simplified", "--bps", "4"]).demapper == "simplified"
    for bad in ("sofisticated", "Simplified", ""):
        with pytest.raises(SystemExit):
            p.parse_args(["edges.csv", "--demapper", bad])


def test_unknown_demapper_rejected_before_device():
    """The keyword is validated first: no decoder handle, torch or device is needed to be refused."""
    from qamr.pipeline import DEMAPPERS, SofteningPipeline, check_demapper
    from qamr.sim import Simulator

    assert DEMAPPERS == ("search", "simplified")
    for ok in DEMAPPERS:
        assert check_demapper(ok) == ok
    for bad in ("interp", "sofisticated", None, 1):
        with pytest.raises(ValueError, match="demapper"):
            check_demapper(bad)
        with pytest.raises(ValueError, match="demapper"):
            SofteningPipeline(None, 2, 4.0, 64, demapper=bad)
        with pytest.raises(ValueError, match="demapper"):
            Simulator(None, 2, demapper=bad)


def test_noisemapper_has_interpolated_surface():
    import qamr

    for name in ("g_inv", "demap_noise", "demap_lappr_simplified", "demap_lappr_simplified_array",
                 "demap_simplified_device"):
        assert callable(getattr(qamr.NoiseMapper, name)), name


def test_interp_knob_and_entry_points():
    from qamr import _lib

    saved = _lib.tune_get("interp_fast")
    try:
        assert saved == 1   # default: the shortcut search where the table is certified nondecreasing
        _lib.tune_set("interp_fast", 0)
        assert _lib.tune_get("interp_fast") == 0
    finally:
        _lib.tune_set("interp_fast", saved)
    assert _lib.tune_get("interp_seg") == 4   # 16 grid entries per coarse-table segment
    L = _lib.load()
    for s in ("qr_demap_grid_create", "qr_demap_grid_info", "qr_demap_grid_host", "qr_g_inv_host",
              "qr_demap_simplified_host", "qr_demap_simplified_batch_device"):
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    # a null handle is refused before any device call
    assert L.qr_demap_grid_create(None, 1e-21, 1000, 2.0) == _lib.QR_EVALUE
    assert L.qr_demap_simplified_batch_device(None, 64, 64, 1, None, None, 1.0, None, None) == _lib.QR_EVALUE


def test_fixture_is_well_formed():
    g = golden("interp.npz")
    n_cases = int(g["n_cases"])
    assert n_cases == 11
    assert g["n300"].shape == (309,) and np.isnan(g["n300"][-1]) and not np.isnan(g["n300"][:-1]).any()
    assert g["n2000"].shape == (2008,)
    seen_inf = False
    for c in range(n_cases):
        k = f"c{c}_"
        bps = int(g[k + "bps"])
        M = 1 << bps
        for d in ("y_sha", "F_sha"):
            assert re.fullmatch(r"[0-9a-f]{64}", str(g[k + d])), (c, d)
        assert str(g[k + "y_sha"]) != str(g[k + "F_sha"])
        n_points = int(g[k + "n_points"])
        assert n_points >= 2
        y0, y1 = g[k + "y_ends"]
        F0, F1 = g[k + "F_ends"]
        assert y0 < y1 and 0.0 <= F0 < F1 <= 1.0
        assert g[k + "cfg"].shape == (M,) and g[k + "probs"].shape == (M,)
        assert abs(g[k + "probs"].sum() - 1) < 1e-9
        assert g[k + "ginv"].shape == (M, 309)
        assert g[k + "la"].shape == (2008 * bps,) and g[k + "j2000"].shape == (2008,)
        assert g[k + "j2000"].min() >= 0 and g[k + "j2000"].max() < M
        assert g[k + "blk_n"].shape == (6, 70) and g[k + "blk_j"].shape == (6, 70)
        assert g[k + "blk_la"].shape == (420 * bps,)
        # n_hat in [0, 1) interpolates inside the grid (a target below F[0], n_hat = -0.1, extrapolates)
        gi = g[k + "ginv"][:, :300]
        assert ((gi >= y0) & (gi <= y1)).all()
        seen_inf |= bool(np.isinf(g[k + "la"]).any())
    assert seen_inf
    # (bps, non-default grid parameters) the issue's table asks for
    assert sorted(int(g[f"c{c}_bps"]) for c in range(n_cases)) == [1, 1, 1, 2, 2, 2, 3, 3, 4, 4, 4]
    assert {(float(g[f"c{c}_trunc"]), int(g[f"c{c}_nips"])) for c in range(n_cases)} == {(1e-21, 1000), (1e-12, 100),
                                                                                          (2.0, 100)}
    assert g["e2e_lappr"].shape == (12, 1008) and g["e2e_final"].shape == (12, 1008)
    assert list(zip(g["e2e_success"].tolist(), g["e2e_iters"].tolist())) == [
        (0, 50), (0, 50), (0, 50), (1, 11), (0, 50), (1, 10), (1, 13), (1, 31), (0, 50), (1, 12), (1, 14), (1, 19)]
