"""CPU side of the device-primitive tests: the argument rules of qr_math_eval_host, the input sets of
tests/math_fixture.py (sizes, the specials present, the wavefront layout of the g_exp_wave and h_packed sets),
and the restated direct-reconciliation LAPPRs against both fixtures of the compiled reference."""
import math

import numpy as np
import pytest

from conftest import assert_bit_exact, golden

import math_fixture as MF


def test_math_entry_refuses_bad_arguments_before_any_device_call():
    from qamr import _lib

    L = _lib.load()
    assert "qr_math_eval_host" in _lib.SIGNATURES and hasattr(L, "qr_math_eval_host")
    E = _lib.QR_EVALUE
    z, o = np.zeros(4), np.zeros(4)
    pz, po = _lib.ptr(z), _lib.ptr(o)
    for fn, homes in MF.HOMES.items():
        two = fn in ("box_plus", "box_plus_sel", "div_two_s2")
        for name, h in MF.HOME.items():
            if name in homes:
                # a home of the function: the one rule of *_host entries
                assert L.qr_math_eval_host(MF.FN[fn], h, -1, pz, pz, po) == E and "negative" in _lib.last_error()
                assert L.qr_math_eval_host(MF.FN[fn], h, 4, None, pz, po) == E and "null" in _lib.last_error()
                assert L.qr_math_eval_host(MF.FN[fn], h, 4, pz, pz, None) == E and "null" in _lib.last_error()
                assert (L.qr_math_eval_host(MF.FN[fn], h, 4, pz, None, None) == E) and "null" in _lib.last_error()
                if two:
                    assert L.qr_math_eval_host(MF.FN[fn], h, 4, pz, None, po) == E and "null" in _lib.last_error()
                assert L.qr_math_eval_host(MF.FN[fn], h, 0, None, None, None) == 0
            else:
                assert L.qr_math_eval_host(MF.FN[fn], h, 4, pz, pz, po) == E and "home" in _lib.last_error(), (fn, name)
                assert L.qr_math_eval_host(MF.FN[fn], h, 0, None, None, None) == E
        assert L.qr_math_eval_host(MF.FN[fn], len(MF.HOME), 4, pz, pz, po) == E
        assert L.qr_math_eval_host(MF.FN[fn], -1, 4, pz, pz, po) == E
    assert sorted(MF.FN.values()) == list(range(15)) and sorted(MF.HOME.values()) == list(range(6))
    for fn in (-1, 15, 99):
        assert L.qr_math_eval_host(fn, 0, 4, pz, pz, po) == E and "unknown" in _lib.last_error()
    P = MF.FN["h_packed"]
    for v in range(3 * MF.PACK_MAX_JOBS):
        assert L.qr_math_eval_host(P, v, -1, pz, None, po) == E
        assert L.qr_math_eval_host(P, v, 4, None, None, po) == E
        assert L.qr_math_eval_host(P, v, 4, pz, None, None) == E
        assert L.qr_math_eval_host(P, v, 0, None, None, None) == 0
    for v in (-1, 3 * MF.PACK_MAX_JOBS, 100):
        assert L.qr_math_eval_host(P, v, 4, pz, None, po) == E and "variant" in _lib.last_error()
    assert np.array_equal(o, np.zeros(4))


def _has(x, values):
    xb = np.asarray(x, np.float64).view(np.int64)
    for v in values:
        if v != v:
            assert np.isnan(x).any()
        else:
            assert (xb == np.array([v], np.float64).view(np.int64)[0]).any(), v


def test_elementwise_input_sets():
    """Sizes (about 2e5, so a test takes a few seconds with its Python reference), domains, and the specials."""
    sets = dict(exp=MF.exp_inputs(), exp_neg=MF.exp_neg_inputs(), exp_full=MF.exp_full_inputs(), log_u=MF.log_u_inputs(),
                log=MF.log_inputs(), log_full=MF.log_full_inputs(), h=MF.h_inputs(), box=MF.box_plus_inputs()[0],
                erf=MF.erf_inputs(), div=MF.div_inputs()[0])
    for name, x in sets.items():
        assert 150000 <= x.size <= 260000 and x.dtype == np.float64, (name, x.size)
    x = sets["exp_full"]
    _has(x, MF.FULL_SPECIALS + (np.nextafter(709.78, 0), np.nextafter(-745.2, -math.inf), np.nextafter(1024.0, 0)))
    assert ((x > 709.79) & (x < 760)).sum() > 1000 and ((x < -745.2) & (x > -760)).sum() > 300      # overflow, underflow
    assert ((x < -708.4) & (x > -745.1)).sum() > 800                                                # subnormal results
    assert ((np.abs(x) >= 512) & (np.abs(x) < 708)).sum() > 5000                                    # rescaled, normal results
    assert (np.abs(x) < 2.0 ** -54).sum() > 1000 and (np.abs(x) > 1e300).sum() > 50
    expo = (x.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)
    assert np.unique(expo).size == 2048                                                             # every exponent
    b = np.arange(-128 * 40, 1) * MF.LN2 / 128.0
    for s in (sets["exp"], x):
        assert np.isin(b, s).all() and np.isin(np.nextafter(b, 0.0), s).all() and np.isin(np.nextafter(b, -1e3), s).all()
    _has(sets["exp"], (0.0, -0.0, 2.0 ** -54, -2.0 ** -54, 2.0 ** -55, -5e-324, -40.0, math.nan))
    _has(sets["exp_neg"], (0.0, -0.0, -2.0 ** -54, -5e-324, -37.5, -37.51, math.nan))
    lf = sets["log_full"]
    _has(lf, (0.0, -0.0, math.inf, -math.inf, math.nan, -1.0, 5e-324, MF.DBL_MIN, MF.DBL_MAX, MF.NEAR1_LO, MF.NEAR1_HI,
              np.nextafter(MF.NEAR1_LO, 0), np.nextafter(MF.NEAR1_HI, 0), np.nextafter(MF.NEAR1_LO, 2), np.nextafter(MF.NEAR1_HI, 2)))
    assert ((lf > 0) & (lf < MF.DBL_MIN)).sum() > 20000 and (lf < 0).sum() > 10000
    assert ((lf >= MF.NEAR1_LO) & (lf < MF.NEAR1_HI)).sum() > 30000
    _has(sets["log"], (MF.NEAR1_LO, MF.NEAR1_HI, np.nextafter(MF.NEAR1_LO, 0), np.nextafter(MF.NEAR1_HI, 2), 1.0, 2.0, MF.DBL_MIN, MF.DBL_MAX))
    _has(sets["log_u"], (1.0, 2.0, np.nextafter(1.0, 2), np.nextafter(2.0, 1), MF.NEAR1_HI, np.nextafter(MF.NEAR1_HI, 1), math.nan))
    _has(sets["h"], MF.H_SPECIALS)
    a, bb = MF.box_plus_inputs()
    assert a.size == bb.size == 190000 + 64
    for u in MF.BOX_SPECIALS:
        for v in MF.BOX_SPECIALS:
            same = lambda p, q: (np.isnan(p) if q != q else p.view(np.int64) == np.array([q]).view(np.int64)[0])
            assert (same(a[-64:], u) & same(bb[-64:], v)).sum() == 1
    assert (a[:190000] == -bb[:190000]).sum() > 2000 and (a[:190000] == bb[:190000]).sum() > 2000
    e = sets["erf"]
    _has(e, (0.0, -0.0, math.inf, -math.inf, math.nan, 1.0, -1.0, 8.0, -8.0, MF.SQRT_MAXLOG, -MF.SQRT_MAXLOG, 5e-324,
             np.nextafter(1.0, 2), np.nextafter(1.0, 0), np.nextafter(8.0, 9), np.nextafter(8.0, 0),
             np.nextafter(MF.SQRT_MAXLOG, 27), np.nextafter(MF.SQRT_MAXLOG, 0)))
    assert -MF.SQRT_MAXLOG * MF.SQRT_MAXLOG >= -7.09782712893383996732E2 > -np.nextafter(MF.SQRT_MAXLOG, 27) ** 2 - 1e-12
    x, d = MF.div_inputs()
    assert x.size == d.size and (d > 0).all() and np.isfinite(d).all() and (x == 0).sum() >= 16


def test_exp_wave_layout():
    x, lay = MF.exp_wave_inputs()
    assert 150000 <= x.size <= 260000 and x.size % 64 == lay["tail"] == 37
    sp = MF.exp_special(x)
    nw = x.size // 64
    per = sp[:nw * 64].reshape(nw, 64).sum(1)
    assert len(lay["none"]) >= 100 and (per[lay["none"]] == 0).all()
    assert (per[lay["all"]] == 64).all() and len(lay["all"]) >= len(MF.WAVE_SPECIALS)
    seen = set()
    for w, lane, v in lay["one"]:
        assert per[w] == 1 and sp[64 * w + lane]
        assert (x[64 * w + lane] != x[64 * w + lane]) if v != v else x[64 * w + lane] == v
        seen.add((lane, repr(v)))
    assert seen == {(lane, repr(v)) for lane in (0, 31, 32, 63) for v in MF.WAVE_SPECIALS}
    v = np.abs(np.array(MF.WAVE_SPECIALS))
    assert (v < 2.0 ** -54).any() and ((v >= 512) & (v < 1024)).any() and ((v >= 1024) & np.isfinite(v)).any()
    assert np.isinf(v).any() and np.isnan(v).any()
    # the rescaled range on a lone lane: an overflowing, a subnormal and an underflowing result among them
    r = MF.ref_exp([t for t in MF.WAVE_SPECIALS if 512 <= abs(t) < 1024])
    assert np.isinf(r).any() and ((r > 0) & (r < MF.DBL_MIN)).any() and (r == 0).any() and ((r > 1) & np.isfinite(r)).any()
    assert sp[nw * 64:].sum() == 1 and len(lay["mixed"]) > 2000
    assert sorted(lay["none"] + [w for w, _, _ in lay["one"]] + lay["all"] + lay["mixed"]) == list(range(nw))


@pytest.mark.parametrize("clamp", sorted(MF.CLAMP))
def test_h_packed_layout(clamp):
    total = 0
    for nj in range(1, MF.PACK_MAX_JOBS + 1):
        t, counts = MF.h_packed_inputs(nj, clamp)
        W = 64 * nj
        nw = t.size // W
        assert nw == counts.size and t.size % 64 == 64 - 27 and t.size % W == W - 27
        nN = MF.h_near(t[:nw * W]).reshape(nw, W).sum(1)
        assert np.array_equal(nN, counts)
        want = set(MF.pack_counts(nj))
        assert want >= {0, 1, 63, 64, W} and (nj == 1 or 65 in want)
        assert want <= set(nN.tolist()) and want <= set((W - nN).tolist())      # as near-1 count and as table count
        assert (nN == W).sum() >= 6 and (nN == 0).sum() >= 6 and ((nN > 1) & (nN < W - 1)).sum() >= 20
        _has(t, MF.PACK_SPECIALS[clamp])
        fin = np.isfinite(t)
        if clamp == "none":
            assert fin.all() and (np.abs(t) < 700).all()
        elif clamp == "finite":
            assert fin.all() and (np.abs(t) >= 700).any()
        else:
            assert np.isnan(t).any() and np.isinf(t).any()
        total += t.size
    assert 100000 <= total <= 260000


# ------------------------------------------------------------------ direct-reconciliation LAPPRs
LLR_KEYS = [("b1_s20", 1), ("b2_s30", 2), ("b2_s95", 2), ("b4_s130", 4), ("b4_s250", 4)]


@pytest.mark.parametrize("key,bps", LLR_KEYS)
def test_restated_direct_lappr_vs_reference(key, bps):
    from qamr import PAMAlphabet

    g = golden("llr_sources.npz")
    pa = PAMAlphabet(bps, 2.0)
    assert_bit_exact(MF.y_to_lappr_grey(g[f"{key}_y"], pa.constellation, bps, float(g[f"{key}_two_var"])), g[f"{key}_direct"])


@pytest.mark.parametrize("c", range(len(MF.LAPPR_WIDE_CASES)))
def test_restated_direct_lappr_vs_wide_reference(c):
    """The restatement on llr_sources_wide.npz, whose samples reach exp's and log's tails (asserted here: +-inf
    and NaN LAPPRs, subnormal and zero sums); the alphabet, twoVariance and the hard-reverse table of the
    product's host code equal the reference's."""
    from make_golden_cases import demap_wide_probs
    from qamr import PAMAlphabet
    from qamr.noisemapper import host_tables

    g = golden("llr_sources_wide.npz")
    assert int(g["n_cases"]) == len(MF.LAPPR_WIDE_CASES)
    bps, shape, snr = MF.LAPPR_WIDE_CASES[c]
    k = f"c{c}_"
    probs = demap_wide_probs(bps, shape)
    pa = PAMAlphabet(bps, 2.0, probs)
    two_var = float(g[k + "two_var"])
    assert int(g[k + "bps"]) == bps and np.array_equal(pa.probabilities, g[k + "probs"])
    assert two_var == pa.variance * (10 ** (-snr / 10))
    y = g[k + "y"]
    assert_bit_exact(y, MF.lappr_samples(pa.constellation, pa.thresholds, two_var, 6100 + c))
    direct = g[k + "direct"]
    assert direct.size == y.size * bps
    assert_bit_exact(MF.y_to_lappr_grey(y, pa.constellation, bps, two_var), direct)
    assert (direct == np.inf).any() and (direct == -np.inf).any() and np.isnan(direct).any()
    a = np.asarray(pa.constellation)
    with np.errstate(all="ignore"):
        arg = -((y[:, None] - a[None, :]) ** 2) / two_var
    top = np.where(np.isnan(arg), -np.inf, arg).max(axis=1)
    assert ((top > -745) & (top < -708)).sum() >= 20       # sums of subnormal exponentials only
    assert (np.isfinite(y) & (top < -746)).sum() >= 6      # no exponential survives
    _has(y, tuple(a) + (0.0, -0.0, 1e300, -1e300, np.inf, -np.inf, np.nan))
    bare = host_tables(pa.constellation, pa.thresholds, pa.probabilities, np.sqrt(two_var / 2), bps)[2]
    assert_bit_exact(bare, g[k + "bare"])
    assert_bit_exact(bare[g[k + "x"].astype(np.int64)].reshape(-1), g[k + "bare_llr_x"])
