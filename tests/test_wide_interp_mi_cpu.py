"""CPU-side checks at 32- and 64-PAM: the fixture tests/golden/wide_interp_mi.npz (written by
tests/golden/make_golden_wide_interp_mi.py from the compiled reference) is well formed and holds the
generator's conditions; the host-side tables (host_tables, P_xhat, mutual_information_X_Xhat), the draws of
montecarlo_information and -- through the native replays tests/native/mi_check.cpp and mi_quad_check.cpp, which
call the very functions the kernels call -- the per-sample and per-abscissa arithmetic of mi_math.hpp and the
host integrator equal the reference bit for bit before any GPU is involved."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, assert_bit_exact, golden

import native_check
from mapper_fixture import alphabet, host_mapper, sha

PATH = os.path.join(ROOT, "tests", "golden", "wide_interp_mi.npz")
CASES = range(1, 8)
MC_CASES = (1, 2, 3, 4, 5, 7)
QUAD_CASES = (1, 2, 3, 4, 5)
B, S, N_YHAT = 70, 11, 5
EDGE = np.array([0.0, 1.0, 5e-324, 1 - 2 ** -53, 2 ** -53, 1e-300, -0.1, 1.1])   # make_golden_interp.EDGE
# k: (bps, SNR dB, shaped?, configuration, (trunkation_threshold, n_intervals_per_step), n_points above)
TABLE = {
    1: (5, 22.0, False, "random", (1e-21, 1000), 0),
    2: (6, 28.0, False, "random", (1e-21, 1000), 65536),
    3: (6, 10.0, False, "alternating", (1e-21, 1000), 131072),
    4: (5, 5.0, True, "zero", (1e-21, 1000), 65536),
    5: (3, 8.0, True, "random", (1e-21, 1000), 0),
    6: (6, -5.0, False, "alternating", (1e-21, 1000), 262144),
    7: (6, 40.0, False, "alternating", (1e-12, 100), 0),
}


@pytest.fixture(scope="module")
def fx():
    return golden("wide_interp_mi.npz")


def test_fixture_is_well_formed(fx):
    assert int(fx["n_cases"]) == 7 and int(fx["B"]) == B and int(fx["S"]) == S
    assert os.path.getsize(PATH) <= 1_500_000
    deep_last = False
    for k in CASES:
        bps, snr, shaped, cfgkind, grid, above = TABLE[k]
        key = f"w{k}_"
        M = 1 << bps
        pa = alphabet(fx, key)
        assert int(fx[key + "bps"]) == bps and pa.order == M
        assert (float(fx[key + "trunc"]), int(fx[key + "nips"])) == grid
        probs, cfg = fx[key + "probs"], fx[key + "cfg"]
        assert probs.shape == (M,) and cfg.shape == (M,) and cfg.dtype == np.uint8 and cfg.max() <= 1
        assert bool(np.all(probs == probs[0])) != shaped
        if shaped:   # the outermost symbol has a tenth of the innermost's mass; the in-order sum is exactly 1
            assert abs(probs[0] / probs[M // 2] - 0.1) < 1e-9 and abs(probs[-1] / probs[M // 2 - 1] - 0.1) < 1e-9
            s = 0.0
            for v in probs:
                s += float(v)
            assert s == 1.0
        assert_bit_exact([fx[key + "noise_var"]], [pa.variance * (10 ** (-snr / 10)) / 2])
        want = {"zero": np.zeros(M, np.uint8), "alternating": np.arange(M, dtype=np.uint8) & 1,
                "random": np.random.default_rng(7000 + k).integers(0, 2, M).astype(np.uint8)}[cfgkind]
        assert np.array_equal(cfg, want)
        if cfgkind == "random" and M == 64:   # mask bits below and at or above index 32, set and clear
            assert cfg[:32].any() and cfg[32:].any() and not cfg[:32].all() and not cfg[32:].all()
        # the grid
        n = int(fx[key + "n_points"])
        assert n > above
        for d in ("y_sha", "F_sha", "fwrd_sha"):
            assert re.fullmatch(r"[0-9a-f]{64}", str(fx[key + d])), (k, d)
        ns = (n + 996) // 997
        for t in ("y", "F"):
            assert fx[key + t + "_head"].shape == (64,) and fx[key + t + "_tail"].shape == (64,)
            assert fx[key + t + "_stride"].shape == (ns,)
            assert_bit_exact([fx[key + t + "_stride"][0]], [fx[key + t + "_head"][0]])
            allv = np.concatenate([fx[key + t + "_head"], fx[key + t + "_stride"][1:], fx[key + t + "_tail"]])
            assert not (np.diff(fx[key + t + "_head"]) < 0).any() and not (np.diff(fx[key + t + "_tail"]) < 0).any()
            assert not (np.diff(fx[key + t + "_stride"]) < 0).any() and np.isfinite(allv).all()
        assert (np.diff(fx[key + "y_stride"]) > 0).all()
        assert 0.0 <= fx[key + "F_head"][0] < fx[key + "F_tail"][-1] <= 1.0
        # the small tables
        assert fx[key + "p_Xhat"].shape == (M,) and abs(fx[key + "p_Xhat"].sum() - 1) < 1e-9
        assert fx[key + "Fthr"].shape == (M + 1,) and fx[key + "dF"].shape == (M,)
        assert_bit_exact(fx[key + "dF"], fx[key + "Fthr"][1:] - fx[key + "Fthr"][:-1])
        for t in ("fwrd_first", "fwrd_last", "fwrd_diag"):
            assert fx[key + t].shape == (M,)
        assert fx[key + "fwrd_first"][0] == fx[key + "fwrd_diag"][0] and fx[key + "fwrd_last"][-1] == fx[key + "fwrd_diag"][-1]
        assert 0.0 <= float(fx[key + "I_X_Xhat"]) <= bps + 1e-9
        # g_inv and formulation 1
        n109, n508 = fx[key + "n109"], fx[key + "n508"]
        assert n109.shape == (109,) and np.isnan(n109[-1]) and np.array_equal(n109[100:108], EDGE)
        assert ((n109[:100] >= 0) & (n109[:100] < 1)).all()
        assert n508.shape == (508,) and np.array_equal(n508[500:], EDGE) and ((n508[:500] >= 0) & (n508[:500] < 1)).all()
        assert fx[key + "ginv"].shape == (M, 109) and np.isnan(fx[key + "ginv"][:, -1]).all()
        gi = fx[key + "ginv"][:, :100]
        assert ((gi >= fx[key + "y_head"][0]) & (gi <= fx[key + "y_tail"][-1])).all()
        assert fx[key + "j508"].shape == (508,) and fx[key + "j508"].min() >= 0 and fx[key + "j508"].max() < M
        assert fx[key + "la"].shape == (508 * bps,)
        assert fx[key + "blk_n"].shape == (6, B) and fx[key + "blk_j"].shape == (6, B) and fx[key + "blk_la"].shape == (6 * B * bps,)
        assert fx[key + "blk_j"].min() >= 0 and fx[key + "blk_j"].max() < M
        drawn = np.concatenate([fx[key + "la"][:500 * bps], fx[key + "blk_la"]])
        if k == 7:
            assert np.isposinf(drawn).any() and np.isneginf(drawn).any()
        else:
            assert np.isfinite(fx[key + "la"][:500 * bps]).mean() > 0.5 and np.isfinite(fx[key + "blk_la"]).mean() > 0.5
        # Monte-Carlo
        assert int(fx[key + "has_mc"]) == (k in MC_CASES) and int(fx[key + "has_quad"]) == (k in QUAD_CASES)
        if k in MC_CASES:
            assert fx[key + "x"].shape == (B, S) and fx[key + "x"].dtype == np.int8 and fx[key + "xhat"].shape == (B, S)
            assert fx[key + "x"].min() >= 0 and fx[key + "x"].max() < M
            assert fx[key + "xhat"].min() >= 0 and fx[key + "xhat"].max() < M
            assert fx[key + "y"].shape == (B, S) and fx[key + "terms"].shape == (3, B, S) and fx[key + "totals"].shape == (B, 3)
            assert fx[key + "yhat"].shape == (N_YHAT, S, M) and np.isfinite(fx[key + "yhat"]).all()
            t = fx[key + "terms"]
            for f in (0, 33, B - 1):   # the totals (the compiled reference's) are the sequential sums of the terms
                I = [0.0, 0.0, 0.0]
                for p in range(S):
                    I[0] += float(t[0, f, p])
                    I[1] += float(t[1, f, p])
                    I[2] -= float(t[2, f, p])
                assert_bit_exact([v / S for v in I], fx[key + "totals"][f])
            # no SNR puts a non-finite term on the reference's path; 64-PAM at 40 dB overflows exp to inf instead
            assert np.isfinite(t).all() and int(fx[key + "n_overflow"]) >= 0
            if k == 7:
                assert int(fx[key + "n_overflow"]) > 1000
        else:
            assert key + "x" not in fx.files
        # quadrature
        if k in QUAD_CASES:
            assert int(fx[key + "limit"]) == 50
            for name, per in (("base", 21), ("xy", 30)):
                neval, last = int(fx[f"{key}{name}_neval"]), int(fx[f"{key}{name}_last"])
                assert fx[f"{key}{name}_x"].shape == fx[f"{key}{name}_f"].shape == (min(42, neval),)
                assert neval == (42 * last - 21 if name == "base" else 2 * (30 * last - 15))
                assert int(fx[f"{key}{name}_warned"]) in (0, 1) and 1 <= last <= 50
            assert np.isfinite(fx[key + "base_I"]) and np.isfinite(fx[key + "base_f"]).all()
            assert ((fx[key + "base_x"] > 0) & (fx[key + "base_x"] < 1)).all()
            assert np.isfinite(fx[key + "xy_I"]) or fx[key + "xy_I"] == -np.inf
            deep_last |= bps >= 5 and int(fx[key + "base_last"]) >= 3
        else:
            assert key + "base_I" not in fx.files
    assert np.isfinite(fx["w3_xy_I"])
    assert deep_last   # a work list beyond round 1 runs at M >= 32


@pytest.mark.parametrize("k", CASES)
def test_host_tables_bit_exact(fx, k):
    """host_tables' fwrd_transition_probability (digest, first and last row, diagonal), P_xhat and
    mutual_information_X_Xhat at 8-, 32- and 64-PAM, shaped alphabets included."""
    from qamr.mutual_information import P_xhat, mutual_information_X_Xhat

    key = f"w{k}_"
    pa, nm = host_mapper(fx, key)
    fw = nm.fwrd_transition_probability
    assert_bit_exact(fw[0], fx[key + "fwrd_first"])
    assert_bit_exact(fw[-1], fx[key + "fwrd_last"])
    assert_bit_exact(np.diag(fw), fx[key + "fwrd_diag"])
    assert sha(fw) == str(fx[key + "fwrd_sha"])
    pX = P_xhat(nm)
    assert_bit_exact(pX, fx[key + "p_Xhat"])
    assert_bit_exact([mutual_information_X_Xhat(nm, pX)], [fx[key + "I_X_Xhat"]])


def test_fixture_draw_order_is_the_references(fx):
    """PAMAlphabet.random_symbols and the S scalar normal draws under np.random.seed(9000 + 100 k + f) give the
    fixture's blocks, at the shaped 32-PAM and 8-PAM alphabets and at uniform 64-PAM."""
    for k in (2, 4, 5, 7):
        pa = alphabet(fx, f"w{k}_")
        sigma = float(np.sqrt(float(fx[f"w{k}_noise_var"])))
        for f in (0, 69):
            np.random.seed(9000 + 100 * k + f)
            x = pa.random_symbols(S)
            y = pa.index_to_value(x) + sigma * np.random.randn(S)
            assert np.array_equal(x, fx[f"w{k}_x"][f])
            assert_bit_exact(y, fx[f"w{k}_y"][f])


def dump_mc_case(fx, k, path):
    """The raw input of `mi_check sample` (tests/test_mi_cpu.dump_case's layout) for a case of this fixture; the
    fwrd table is host_tables', whose digest test_host_tables_bit_exact pins."""
    key = f"w{k}_"
    pa, nm = host_mapper(fx, key)
    assert sha(nm.fwrd_transition_probability) == str(fx[key + "fwrd_sha"])
    parts = [np.array([pa.bit_per_symbol, N_YHAT, S, float(fx[key + "noise_var"])]), pa.constellation, pa.probabilities,
             pa.thresholds, fx[key + "cfg"], fx[key + "p_Xhat"], nm.fwrd_transition_probability]
    for f in range(N_YHAT):
        parts += [fx[key + "x"][f], fx[key + "xhat"][f], fx[key + "y"][f], fx[key + "yhat"][f], fx[key + "terms"][:, f, :],
                  fx[key + "totals"][f]]
    np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]).tofile(path)


def dump_quad_case(fx, k, path, integrals):
    """The raw input of `mi_quad_check case` (tests/test_mi_quad_cpu.dump_case's layout)."""
    key = f"w{k}_"
    pa = alphabet(fx, key)
    parts = [np.array([pa.bit_per_symbol, float(fx[key + "noise_var"]), float(fx[key + "limit"]), float(fx[key + "trunc"]),
                       float(fx[key + "nips"]), float(pa.step), float(integrals)]),
             pa.constellation, pa.probabilities, pa.thresholds, fx[key + "cfg"], fx[key + "p_Xhat"]]
    for name in ("base", "xy"):
        parts += [[float(fx[key + name + "_x"].size)], fx[key + name + "_x"], fx[key + name + "_f"]]
    for name in ("base", "xy"):
        parts += [[float(fx[key + name + "_" + f]) for f in ("I", "abserr", "neval", "warned")]]
    np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]).tofile(path)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_sample_arithmetic_bit_exact(fx, tmp_path, sanitize):
    """mi_sample_terms (mi_math.hpp, the function k_mi_terms calls) on the fixture's x, x_hat, y and y_hat of the
    first 5 blocks gives the fixture's terms and the compiled reference's totals, and mi_bob its x_hat, at
    8-, 32- and 64-PAM; once more with the address and undefined-behaviour sanitizers on the host code."""
    exe = native_check.build(tmp_path, "mi_check.cpp", exe_name="mi_check_wide" + ("_san" if sanitize else ""), sanitize=sanitize)
    for k in MC_CASES:
        path = str(tmp_path / f"mc{k}.bin")
        dump_mc_case(fx, k, path)
        out = native_check.run(exe, "sample", path)
        assert f"{N_YHAT * S * 3} inputs, 0 mismatches" in out and f"{N_YHAT * S} samples, 0 mismatches" in out, (k, out)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_integrands_and_host_integrals_bit_exact(fx, tmp_path, sanitize):
    """mi_base_arg / mi_xy_arg (the functions k_mi_quad calls) with host providers -- g_inv on a host-built grid of
    up to 144 244 points -- equal the compiled reference's integrands at every stored abscissa of cases 1..5; in
    the plain build both integrals run wholly on the host through the batch's driver and equal the fixture's."""
    exe = native_check.build(tmp_path, "mi_quad_check.cpp", exe_name="mi_quad_check_wide" + ("_san" if sanitize else ""),
                             sanitize=sanitize)
    for k in QUAD_CASES:
        path = str(tmp_path / f"quad{k}.bin")
        integrals = not sanitize or k == 5
        dump_quad_case(fx, k, path, integrals)
        out = native_check.run(exe, "case", path)
        npts = fx[f"w{k}_base_x"].size + fx[f"w{k}_xy_x"].size
        assert f"{npts} points, 0 mismatches" in out, (k, out)
        assert ("2 on the host, 0 mismatches" in out) == integrals, (k, out)
