"""Generate tests/golden/wide_interp_mi.npz: the interpolation grid, the table-interpolated g_inv, the
formulation-1 demapper, the Monte-Carlo estimator and the quad-integrated evaluators at 32- and 64-PAM, with
shaped alphabets, sign configurations that set bits 32..63, and grids of more than 65 536 points.

Run where the reference build is available, as tests/golden/make_golden_interp.py:

    make -C oracle ref
    PYTHONPATH=oracle/_ref python3 tests/golden/make_golden_wide_interp_mi.py

Every value comes from the compiled reference (oracle/Makefile `ref` builds mutual_information.pyx too):
NoiseMapper.y_range / F_Y_values / demap_noise / demap_lappr_simplified_array, P_xhat,
fwrd_transition_probability, mutual_information_base_scheme_arg / _X_Y_int_arg, mutual_information_base_scheme /
_X_Y / _X_Xhat and montecarlo_information under np.random.seed.  Two things are not the reference's own return
values:

  * abserr, neval, last and the warning flag of the integrals are scipy.integrate.quad(..., full_output=1)
    over the compiled integrand functions, through make_golden_mi_quad.run_quad (which also logs the
    abscissae); the I it returns is asserted bit-equal to the reference's own mutual_information_base_scheme /
    mutual_information_X_Y;
  * the per-sample Monte-Carlo terms are the restated scalar lines of make_golden_mi.block (imported, not
    copied); their sequential sums are asserted bit-equal to the compiled montecarlo_information's totals for
    every stored block, under the same seed.

retro_check() asserts the same of the fixtures written before the reference build had the module: the 8 x 70
blocks of mi.npz and the 18 integrals of cases 1..9 of mi_quad.npz.  It rewrites neither file.

Only data is stored, no reference source.  Cases (prefix "w<k>_"), alphabets of step 2, noise_var =
Es 10^(-snr/10) / 2; "random" configurations are default_rng(7000 + k).integers(0, 2, M); shaped probabilities
are exp(-nu a_m^2) with the outermost symbol at a tenth of the innermost's mass, summed to exactly 1
(make_golden_cases.exact_unit_sum):

  k  alphabet        SNR     configuration  grid (trunkation_threshold, n_intervals_per_step)   surfaces
  1  32-PAM uniform  22 dB   random         1e-21, 1000                                         all
  2  64-PAM uniform  28 dB   random         1e-21, 1000   (> 65 536 points)                     all
  3  64-PAM uniform  10 dB   alternating    1e-21, 1000   (> 131 072 points)                    all
  4  32-PAM shaped    5 dB   all-zero       1e-21, 1000   (> 65 536 points)                     all
  5   8-PAM shaped    8 dB   random         1e-21, 1000                                         all
  6  64-PAM uniform  -5 dB   alternating    1e-21, 1000   (> 262 144 points)                    grid, g_inv, formulation 1
  7  64-PAM uniform  40 dB   alternating    1e-12, 100                                          the same and Monte-Carlo

Stored per case:

  bps, noise_var, cfg [M], probs [M], trunc, nips, has_mc, has_quad          the arguments
  n_points, y_sha, F_sha, y_head / y_tail / F_head / F_tail [64],            the grid: digests of the raw bytes,
    y_stride / F_stride (every 997th entry)                                  both ends, strided samples
  p_Xhat [M], I_X_Xhat, fwrd_sha, fwrd_first / fwrd_last / fwrd_diag [M],    the small tables
    Fthr [M + 1], dF [M]
  n109 [109], ginv [M][109]            demap_noise on 100 seeded draws, make_golden_interp.EDGE and NaN, every i
  n508 [508], j508 [508], la [508 bps] demap_lappr_simplified_array on 500 seeded (n, j) and EDGE
  blk_n, blk_j [6][70], blk_la [420 bps]                                     a block for the device layout
  Monte-Carlo (has_mc), B = 70 blocks of S = 11 samples, block f under np.random.seed(9000 + 100 k + f):
    x [B][S] int8, y [B][S], terms [3][B][S], totals [B][3]; for the host replay of the per-sample arithmetic
    n_overflow (exp calls of the restated lines that overflowed to inf);
    also xhat [B][S] int8 (Bob's decisions) and yhat [5][S][M] (first 5 blocks: g_inv(n, k) for k != x_hat,
    g_inv_search(n, x_hat) at k == x_hat)
  quadrature (has_quad): limit, base_x / base_f, xy_x / xy_f [<= 42]  the first abscissae quad visited, the values
    base_I, base_abserr, base_neval, base_last, base_warned; xy_* likewise                     quad's defaults
"""
from __future__ import annotations

import hashlib
import math
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "qam-reconciliation_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))

from qamreconciliation import mutual_information as rmi  # noqa: E402  (the reference build)
from qamreconciliation.alphabet import PAMAlphabet  # noqa: E402
from qamreconciliation.noisemapper import NoiseMapper  # noqa: E402

import make_golden_mi as gmi  # noqa: E402  (the restated per-sample lines: block)
import make_golden_mi_quad as gq  # noqa: E402  (run_quad, the abscissa-logging wrapper)
from make_golden import alternating, noise_var  # noqa: E402
from make_golden_cases import exact_unit_sum, inorder_sum  # noqa: E402
from make_golden_interp import EDGE  # noqa: E402

B, S, N_YHAT = 70, 11, 5
N_ABSC = 42
STRIDE = 997
SIZE_CAP = 1_500_000

# k -> (bps, snr dB, shaped?, configuration, trunkation_threshold, n_intervals_per_step, n_points above,
#       Monte-Carlo?, quadrature?, quad's limit)
CASES = {
    1: (5, 22.0, False, "random", 1e-21, 1000, 0, True, True, 50),
    2: (6, 28.0, False, "random", 1e-21, 1000, 65536, True, True, 50),
    3: (6, 10.0, False, "alternating", 1e-21, 1000, 131072, True, True, 50),
    4: (5, 5.0, True, "zero", 1e-21, 1000, 65536, True, True, 50),
    5: (3, 8.0, True, "random", 1e-21, 1000, 0, True, True, 50),
    6: (6, -5.0, False, "alternating", 1e-21, 1000, 262144, False, False, 50),
    7: (6, 40.0, False, "alternating", 1e-12, 100, 0, True, False, 50),
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def same_bits(a, b):
    """Identical doubles, NaN matching NaN."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return bool(np.array_equal(a[m].view(np.int64), b[m].view(np.int64)))


def shaped_probs(M):
    a = (np.arange(M) - (M - 1) / 2) * 2.0   # alphabet.pyx:62, step 2
    nu = math.log(10.0) / ((M - 1) ** 2 - 1.0)
    p = exact_unit_sum(np.exp(-nu * a * a))
    assert inorder_sum(p) == 1.0 and (p > 0).all()
    assert abs(p[0] / p[M // 2] - 0.1) < 1e-9 and abs(p[-1] / p[M // 2 - 1] - 0.1) < 1e-9
    return p


def sign_config(k, M, kind):
    if kind == "zero":
        return np.zeros(M, np.uint8)
    if kind == "alternating":
        return alternating(M)
    cfg = np.random.default_rng(7000 + k).integers(0, 2, M).astype(np.uint8)
    assert 0 < int(cfg.sum()) < M
    if M == 64:   # the mask has bits set both below and at or above index 32
        assert cfg[:32].any() and cfg[32:].any() and not cfg[:32].all() and not cfg[32:].all()
    return cfg


def build(bps, nv, cfg, probs, trunc, nips):
    uniform = bool(np.all(probs == probs[0]))
    pa = PAMAlphabet(bps, 2.0) if uniform else PAMAlphabet(bps, 2.0, np.array(probs, np.float64))
    return pa, NoiseMapper(pa, float(nv), np.ascontiguousarray(cfg, np.uint8), float(trunc), int(nips))


def draw_block(pa, nm, seed, n):
    """What one montecarlo_information call draws (mutual_information.pyx:236-242), and Bob's side of it."""
    sigma = float(nm.noise_sigma)
    np.random.seed(seed)
    x = np.asarray(pa.random_symbols(n)).astype(np.int64)
    y = np.asarray(pa.index_to_value(x)).copy()
    for q in range(n):
        y[q] += sigma * np.random.randn()
    xh = np.asarray(nm.hard_decide_index(y)).astype(np.int64)
    nh = np.asarray(nm.map_noise(y, xh)).copy()
    return x, y, xh, nh


def mc_tables(pa, nm):
    M = pa.order
    a = [float(v) for v in pa.constellation]
    p = [float(v) for v in pa.probabilities]
    dF = [float(v) for v in nm.delta_F_Y]
    fw = [[float(v) for v in row] for row in np.asarray(nm.fwrd_transition_probability)]
    return M, a, p, dF, fw, 2.0 * float(nm.noise_var)


def gen_mc(out, k, key, pa, nm, pX):
    M, a, p, dF, fw, tv = mc_tables(pa, nm)
    pXl = [float(v) for v in pX]
    X, XH, Y = np.empty((B, S), np.int8), np.empty((B, S), np.int8), np.empty((B, S))
    T, TOT, YH = np.empty((3, B, S)), np.empty((B, 3)), np.empty((N_YHAT, S, M))
    gmi.N_OVERFLOW[0] = 0
    for f in range(B):
        seed = 9000 + 100 * k + f
        x, y, xh, nh = draw_block(pa, nm, seed, S)
        tot, terms, yh = gmi.block(nm, M, a, p, dF, fw, pXl, tv, x, y, xh, nh, f < N_YHAT)
        np.random.seed(seed)
        ref = rmi.montecarlo_information(pa, nm, pX, S)
        assert same_bits(tot, ref), (k, f, tot, ref)
        X[f], XH[f], Y[f], T[:, f, :], TOT[f] = x, xh, y, terms, ref
        if f < N_YHAT:
            YH[f] = yh
    out.update({key + "x": X, key + "xhat": XH, key + "y": Y, key + "terms": T, key + "totals": TOT, key + "yhat": YH,
                key + "n_overflow": gmi.N_OVERFLOW[0]})
    return int((~np.isfinite(T)).sum()), gmi.N_OVERFLOW[0]


def quad_pair(nm, pX, limit):
    """Both integrals over the compiled integrands -> ((I, abserr, neval, last, warned), xs, fs) each; the I are
    the reference's own at quad's default limit."""
    kw = {} if limit == 50 else {"limit": limit}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        b = gq.run_quad(lambda n: rmi.mutual_information_base_scheme_arg(n, nm, pX), 0, 1, (), **kw)
        x = gq.run_quad(lambda y: rmi.mutual_information_X_Y_int_arg(y, nm), -np.inf, np.inf, (), **kw)
        if limit == 50:
            assert same_bits(b[0][0], rmi.mutual_information_base_scheme(nm, pX)), b[0]
            assert same_bits(x[0][0], rmi.mutual_information_X_Y(nm)), x[0]
    return b, x


def gen_case(out, k):
    bps, snr, shaped, cfgkind, trunc, nips, above, has_mc, has_quad, limit = CASES[k]
    t0 = time.time()
    M = 1 << bps
    probs = shaped_probs(M) if shaped else np.full(M, 1.0 / M)
    cfg = sign_config(k, M, cfgkind)
    pa0 = PAMAlphabet(bps, 2.0, probs.copy()) if shaped else PAMAlphabet(bps, 2.0)
    nv = float(noise_var(pa0, snr))
    pa, nm = build(bps, nv, cfg, np.asarray(pa0.probabilities), trunc, nips)
    key = f"w{k}_"
    y, F = np.asarray(nm.y_range), np.asarray(nm.F_Y_values)
    assert y.size == F.size and y.size > above, (k, y.size, above)
    assert not (np.diff(F) < 0).any(), (k, "F_Y_values decreases")
    fw = np.asarray(nm.fwrd_transition_probability).copy()
    pX = np.asarray(rmi.P_xhat(nm)).copy()
    out.update({key + "bps": bps, key + "noise_var": nv, key + "cfg": cfg, key + "probs": np.asarray(pa.probabilities).copy(),
                key + "trunc": trunc, key + "nips": nips, key + "has_mc": int(has_mc), key + "has_quad": int(has_quad),
                key + "n_points": y.size, key + "y_sha": sha(y), key + "F_sha": sha(F),
                key + "y_head": y[:64].copy(), key + "y_tail": y[-64:].copy(), key + "y_stride": y[::STRIDE].copy(),
                key + "F_head": F[:64].copy(), key + "F_tail": F[-64:].copy(), key + "F_stride": F[::STRIDE].copy(),
                key + "p_Xhat": pX, key + "I_X_Xhat": float(rmi.mutual_information_X_Xhat(nm, pX)),
                key + "fwrd_sha": sha(fw), key + "fwrd_first": fw[0].copy(), key + "fwrd_last": fw[-1].copy(),
                key + "fwrd_diag": np.diag(fw).copy(),
                key + "Fthr": np.asarray(nm.F_Y_thresholds).copy(), key + "dF": np.asarray(nm.delta_F_Y).copy()})
    rng = np.random.default_rng(7100 + k)
    n109 = np.concatenate([rng.uniform(0, 1, 100), EDGE, [np.nan]])
    out[key + "n109"] = n109
    out[key + "ginv"] = np.array([np.asarray(nm.demap_noise(n109.copy(), np.full(n109.size, i, np.int64))) for i in range(M)])
    n508 = np.concatenate([rng.uniform(0, 1, 500), EDGE])
    j508 = rng.integers(0, M, n508.size).astype(np.int64)
    la = np.asarray(nm.demap_lappr_simplified_array(n508.copy(), j508.copy())).copy()
    bn = rng.uniform(0, 1, (6, B))
    bj = rng.integers(0, M, (6, B)).astype(np.int64)
    bla = np.asarray(nm.demap_lappr_simplified_array(bn.ravel().copy(), bj.ravel().copy())).copy()
    out.update({key + "n508": n508, key + "j508": j508.astype(np.int16), key + "la": la,
                key + "blk_n": bn, key + "blk_j": bj.astype(np.int16), key + "blk_la": bla})
    drawn = np.concatenate([la[:500 * bps], bla])   # the LAPPRs of the seeded draws (EDGE holds n_hat outside [0, 1])
    if k == 7:
        assert np.isposinf(drawn).any() and np.isneginf(drawn).any(), (k, "no +-inf LAPPR")
    else:   # the other sets hold finite values (at 28 dB the outer regions of 64-PAM underflow too: a minority)
        assert np.isfinite(la[:500 * bps]).mean() > 0.5 and np.isfinite(bla).mean() > 0.5, (k, int((~np.isfinite(drawn)).sum()))
    nonfinite, overflow = gen_mc(out, k, key, pa, nm, pX) if has_mc else (0, 0)
    if k == 7:
        # No SNR puts a non-finite term on the reference's path: each term is the log2 of a sum that starts from a
        # positive probability, and an infinite sum needs a sample 37 sigma off its symbol.  What the case puts on
        # the path is exp's overflow to inf (then delta_F_Y / inf = 0) and its underflow to 0.
        assert overflow > 0, "case 7 overflows no exp"
    res = None
    if has_quad:
        (b, bx, bf), (x, xx, xf) = quad_pair(nm, pX, limit)
        out.update({key + "limit": limit, key + "base_x": bx[:N_ABSC], key + "base_f": bf[:N_ABSC],
                    key + "xy_x": xx[:N_ABSC], key + "xy_f": xf[:N_ABSC]})
        for name, r in (("base", b), ("xy", x)):
            for field, v in zip(("I", "abserr", "neval", "last", "warned"), r):
                out[key + name + "_" + field] = v
        res = (b, x)
    print(f"  case {k}: {M}-PAM {snr} dB {'shaped' if shaped else 'uniform'} {cfgkind} nv={nv:.6g} n_points={y.size} "
          f"lappr inf={int(np.isinf(drawn).sum())} nan={int(np.isnan(drawn).sum())} of {drawn.size}; "
          f"non-finite MC terms={nonfinite} exp overflows={overflow}; quad={res}; {time.time() - t0:.1f} s", flush=True)
    return res


def retro_check():
    """The fixtures written before the reference build had mutual_information: mi.npz's totals are what the
    compiled montecarlo_information returns under the same seed (and the sequential sums of the stored terms),
    and mi_quad.npz's integrals of cases 1..9 what the compiled mutual_information_base_scheme / _X_Y return."""
    g = np.load(os.path.join(HERE, "mi.npz"), allow_pickle=False)
    Bq, Sq = int(g["B"]), int(g["S"])
    for c in range(1, int(g["n_cases"]) + 1):
        key = f"c{c}_"
        pa, nm = build(int(g[key + "bps"]), float(g[key + "noise_var"]), g[key + "cfg"], g[key + "probs"], 1e-21, 1000)
        pX = np.ascontiguousarray(g[key + "p_Xhat"])
        assert same_bits(pX, np.asarray(rmi.P_xhat(nm))), c
        assert same_bits(g[key + "I_X_Xhat"], rmi.mutual_information_X_Xhat(nm, pX)), c
        t = g[key + "terms"]
        for f in range(Bq):
            np.random.seed(5000 + 100 * c + f)
            ref = rmi.montecarlo_information(pa, nm, pX, Sq)
            I = [0.0, 0.0, 0.0]
            for q in range(Sq):
                I[0] += float(t[0, f, q])
                I[1] += float(t[1, f, q])
                I[2] -= float(t[2, f, q])
            assert same_bits([v / Sq for v in I], ref) and same_bits(g[key + "totals"][f], ref), (c, f)
    print(f"  mi.npz: {int(g['n_cases'])} x {Bq} blocks equal the compiled montecarlo_information", flush=True)
    g = np.load(os.path.join(HERE, "mi_quad.npz"), allow_pickle=False)
    n = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in range(1, 10):
            key = f"c{c}_"
            assert int(g[key + "limit"]) == 50
            pa, nm = build(int(g[key + "bps"]), float(g[key + "noise_var"]), g[key + "cfg"], g[key + "probs"], 1e-21, 1000)
            pX = np.ascontiguousarray(g[key + "p_Xhat"])
            assert same_bits(pX, np.asarray(rmi.P_xhat(nm))), c
            assert same_bits(g[key + "base_I"], rmi.mutual_information_base_scheme(nm, pX)), c
            assert same_bits(g[key + "xy_I"], rmi.mutual_information_X_Y(nm)), c
            n += 2
    print(f"  mi_quad.npz: {n} integrals equal the compiled mutual_information_base_scheme / _X_Y", flush=True)


if __name__ == "__main__":
    retro_check()
    out = {"n_cases": len(CASES), "B": B, "S": S}
    res = {k: gen_case(out, k) for k in CASES}
    # conditions on the reference's own values, not measurements of the code under test
    assert math.isfinite(res[3][1][0]), "w3's X;Y integral is not finite"
    assert any(res[k][0][3] >= 3 for k in (1, 2, 3, 4, 5) if CASES[k][0] >= 5), "no base integral at M >= 32 has last >= 3"
    assert all(math.isfinite(res[k][0][0]) for k in (1, 2, 3, 4, 5))
    path = os.path.join(HERE, "wide_interp_mi.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"[golden] wide_interp_mi.npz: {size} bytes", flush=True)
    assert size <= SIZE_CAP
