"""CPU-side checks of the Monte-Carlo mutual-information estimator: the reference's import line,
the fixture (tests/golden/mi.npz, written by tests/golden/make_golden_mi.py), the host-only
evaluators, the restated glibc log2 and the per-sample arithmetic (tests/native/mi_check.cpp calls
the very function the kernel calls), the entry points' argument checks and the CLI's defaults."""
import os

import numpy as np
import pytest

from conftest import ROOT, assert_bit_exact, golden

import native_check
from mapper_fixture import alphabet, host_mapper

CASES = range(1, 9)
B, S, N_YHAT = 70, 37, 5


@pytest.fixture(scope="module")
def fx():
    return golden("mi.npz")


def test_reference_import_line_resolves():
    from qamreconciliation.mutual_information import P_xhat, montecarlo_information  # sim_montecarlo_information.py:4-5
    from qamreconciliation.mutual_information import mutual_information_X_Xhat
    import qamr.mutual_information as mi

    assert P_xhat is mi.P_xhat and montecarlo_information is mi.montecarlo_information
    assert mutual_information_X_Xhat is mi.mutual_information_X_Xhat
    assert all(callable(f) for f in (P_xhat, montecarlo_information, mutual_information_X_Xhat,
                                     mi.montecarlo_information_device))


def test_fixture_is_well_formed(fx):
    assert int(fx["n_cases"]) == 8 and int(fx["B"]) == B and int(fx["S"]) == S
    assert [int(fx[f"c{c}_bps"]) for c in CASES] == [1, 2, 2, 2, 3, 4, 4, 2]
    special = 0
    for c in CASES:
        k = f"c{c}_"
        M = 1 << int(fx[k + "bps"])
        assert fx[k + "x"].shape == (B, S) and fx[k + "x"].dtype == np.int8
        assert fx[k + "xhat"].shape == (B, S) and fx[k + "y"].shape == (B, S)
        assert fx[k + "x"].min() >= 0 and fx[k + "x"].max() < M
        assert fx[k + "xhat"].min() >= 0 and fx[k + "xhat"].max() < M
        assert fx[k + "terms"].shape == (3, B, S) and fx[k + "totals"].shape == (B, 3)
        assert fx[k + "yhat"].shape == (N_YHAT, S, M) and np.isfinite(fx[k + "yhat"]).all()
        assert fx[k + "p_Xhat"].shape == (M,) and fx[k + "fwrd"].shape == (M, M)
        assert abs(fx[k + "p_Xhat"].sum() - 1) < 1e-9 and np.allclose(fx[k + "fwrd"].sum(axis=1), 1, atol=1e-9)
        assert fx[k + "cfg"].shape == (M,) and abs(fx[k + "probs"].sum() - 1) < 1e-9
        # the generator's conditions, on the stored data
        for q in range(3):
            assert np.isfinite(fx[k + "terms"][q]).mean() >= 0.9, (c, q)
        special += int((~np.isfinite(fx[k + "terms"])).sum()) + int(fx[k + "n_overflow"])
        # the totals are the sequential sums of the terms
        t = fx[k + "terms"]
        for f in (0, B - 1):
            I = [0.0, 0.0, 0.0]
            for p in range(S):
                I[0] += float(t[0, f, p])
                I[1] += float(t[1, f, p])
                I[2] -= float(t[2, f, p])
            assert_bit_exact([v / S for v in I], fx[k + "totals"][f])
        assert 0.0 <= float(fx[k + "I_X_Xhat"]) <= int(fx[k + "bps"]) + 1e-9
    assert special > 0   # a non-finite term or an exp that overflowed is on some case's path
    assert int(fx["c7_n_overflow"]) > 0
    assert not np.all(fx["c4_probs"] == fx["c4_probs"][0]) and not fx["c3_cfg"].any() and fx["c2_cfg"].tolist() == [0, 1, 0, 1]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mi.npz")) < os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "interp.npz"))


def test_fixture_draw_order_is_the_references(fx):
    """An array draw np.random.randn(S) after random_symbols equals the S scalar draws, and the
    fixture's blocks are those draws (PAMAlphabet.random_symbols uses numpy's global stream)."""
    for c in (2, 4, 6):
        pa = alphabet(fx, f"c{c}_")
        sigma = float(np.sqrt(float(fx[f"c{c}_noise_var"])))
        for f in (0, 69):
            np.random.seed(5000 + 100 * c + f)
            x = pa.random_symbols(S)
            y = pa.index_to_value(x) + sigma * np.random.randn(S)
            assert np.array_equal(x, fx[f"c{c}_x"][f])
            assert_bit_exact(y, fx[f"c{c}_y"][f])


@pytest.mark.parametrize("c", CASES)
def test_host_evaluators_bit_exact(fx, c):
    from qamr.mutual_information import P_xhat, mutual_information_X_Xhat

    pa, nm = host_mapper(fx, f"c{c}_")
    assert_bit_exact(nm.fwrd_transition_probability, fx[f"c{c}_fwrd"])
    pX = P_xhat(nm)
    assert_bit_exact(pX, fx[f"c{c}_p_Xhat"])
    assert_bit_exact([mutual_information_X_Xhat(nm, pX)], [fx[f"c{c}_I_X_Xhat"]])


def dump_case(fx, c, path):
    """The raw input of `mi_check sample`: header, tables, then per block x, x_hat, y, y_hat, terms, totals."""
    k = f"c{c}_"
    pa = alphabet(fx, k)
    parts = [np.array([pa.bit_per_symbol, N_YHAT, S, float(fx[k + "noise_var"])]), pa.constellation, pa.probabilities,
             pa.thresholds, fx[k + "cfg"], fx[k + "p_Xhat"], fx[k + "fwrd"]]
    for f in range(N_YHAT):
        parts += [fx[k + "x"][f], fx[k + "xhat"][f], fx[k + "y"][f], fx[k + "yhat"][f], fx[k + "terms"][:, f, :],
                  fx[k + "totals"][f]]
    np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]).tofile(path)


def run_check(exe, fx, tmp_path, n_log2):
    native_check.run(exe, "log2", str(n_log2))
    for c in CASES:
        path = str(tmp_path / f"case{c}.bin")
        dump_case(fx, c, path)
        assert f"{N_YHAT * S * 3} inputs, 0 mismatches" in native_check.run(exe, "sample", path), c


def test_log2_and_sample_arithmetic_bit_exact(fx, tmp_path):
    """g_log2_full == libm's log2 on 18 M inputs; mi_sample_terms on the fixture's x, x_hat, y, y_hat
    gives the fixture's terms and totals (and mi_bob its x_hat), every case."""
    run_check(native_check.build(tmp_path, "mi_check.cpp"), fx, tmp_path, 4000000)


def test_log2_and_sample_arithmetic_under_sanitizers(fx, tmp_path):
    """The same stand-alone program with the address and undefined-behaviour sanitizers on the host code."""
    run_check(native_check.build(tmp_path, "mi_check.cpp", exe_name="mi_check_san", sanitize=True), fx, tmp_path, 300000)


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    import ctypes as C

    from qamr import _lib

    L = _lib.load()
    for s in ("qr_demap_mi_tables", "qr_mi_workspace_size", "qr_mi_montecarlo_device", "qr_mi_montecarlo_host",
              "qr_log2_host", "qr_math_eval_host"):
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    E = _lib.QR_EVALUE
    z = np.zeros(4)
    assert L.qr_demap_mi_tables(None, _lib.ptr(z), _lib.ptr(z)) == E
    # null handle, good shape
    assert L.qr_mi_montecarlo_device(None, 7, 64, 64, 1, None, None, None, None, None, 0, None) == E
    assert "null" in _lib.last_error()
    # bad shapes: S < 1, B > ld, ld not a multiple of 64, B < 1
    for (Bq, ld, Sq) in ((64, 64, 0), (65, 64, 4), (60, 100, 4), (0, 64, 4)):
        assert L.qr_mi_montecarlo_device(None, 7, Bq, ld, Sq, None, None, None, None, None, 0, None) == E
        assert "null" not in _lib.last_error()   # refused for its shape
    assert L.qr_mi_montecarlo_host(None, 4, None, None, None, None, None) == E
    assert L.qr_mi_montecarlo_host(None, 0, None, None, None, None, None) == E
    n = C.c_size_t(99)
    assert L.qr_mi_workspace_size(100, 4, C.byref(n)) == E and n.value == 0
    assert L.qr_mi_workspace_size(64, 0, C.byref(n)) == E
    assert L.qr_mi_workspace_size(64, 4, None) == E
    assert L.qr_mi_workspace_size(128, 37, C.byref(n)) == 0 and n.value >= 3 * 37 * 128 * 8
    assert L.qr_log2_host(-1, None, None) == E
    assert L.qr_log2_host(3, None, None) == E
    assert L.qr_log2_host(0, None, None) == 0
    # the other test-only device entry, same rule (every function and table home: tests/test_device_math_cpu.py)
    assert L.qr_math_eval_host(2, 2, -1, None, None, None) == E
    assert L.qr_math_eval_host(2, 2, 3, None, None, None) == E
    assert "null" in _lib.last_error()
    assert L.qr_math_eval_host(2, 2, 3, _lib.ptr(z), None, None) == E
    assert L.qr_math_eval_host(2, 2, 0, None, None, None) == 0


def test_cli_parser_defaults_match_the_reference():
    from qamr.sim_montecarlo_information import build_parser

    a = build_parser().parse_args([])
    assert (a.out, a.snr, a.nsnr, a.bps, a.niters, a.samples_per_iter) == ("out.csv", [-20, 20], 401, 2, 256, 4096)
    assert (a.seed, a.device) == (0, 0)
    a = build_parser().parse_args(["--snr", "-3", "7.5", "--nsnr", "2", "--bps", "4", "--niters", "4",
                                   "--samples-per-iter", "64", "--seed", "9", "--device", "1", "--out", "x.csv"])
    assert (a.out, a.snr, a.nsnr, a.bps, a.niters, a.samples_per_iter, a.seed, a.device) == (
        "x.csv", [-3.0, 7.5], 2, 4, 4, 64, 9, 1)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--display"])   # plotting is out of scope
