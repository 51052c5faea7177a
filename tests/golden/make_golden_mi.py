"""Generate tests/golden/mi.npz: the Monte-Carlo mutual-information estimator
(qamreconciliation/mutual_information.pyx: P_xhat :29-39, mutual_information_X_Xhat :152-172,
montecarlo_information :218-297) on seeded blocks.

Run where the reference build is available, as tests/golden/make_golden_interp.py:

    make -C oracle ref
    PYTHONPATH=oracle/_ref python3 tests/golden/make_golden_mi.py

When this file was written the reference build (oracle/Makefile `ref`) did not compile
mutual_information.pyx (it does now: make_golden_wide_interp_mi.retro_check asserts that the compiled
montecarlo_information returns the totals stored here, bit for bit, for all 8 x 70 blocks), so every value
the module takes from its NoiseMapper and PAMAlphabet is taken from the compiled reference here too --
random_symbols, index_to_value, hard_decide_index, map_noise, g_inv, g_inv_search,
fwrd_transition_probability, delta_F_Y, probabilities, constellation, noise_var, noise_sigma -- and
only the module's own scalar lines (:29-39, :152-172, :245-297) are restated below, in plain Python
floats (IEEE doubles, one rounding per operation, the reference's operation order), with math.exp
(OverflowError -> inf, what libm returns) and math.log2 (its domain errors -> libm's -inf / NaN), both
of which call libm as the module's `from libc.math cimport exp, log2` does; numpy's vectorised exp /
log2 are not used.  THESE RESTATED LINES ARE THE ONE PART OF THE FIXTURE NOT EXECUTED BY THE
REFERENCE ITSELF.  Only data is stored, no reference source.

Cases (numbered 1..8 as in CASES; prefix "c<c>_"), B = 70 blocks of S = 37 samples each; block f is
drawn as one montecarlo_information call draws it, under np.random.seed(5000 + 100 * c + f):
x = pa.random_symbols(S), then S scalar np.random.randn() draws, y = a[x] + noise_sigma * z.

  n_cases, B, S
  per case: bps, noise_var, cfg [M], probs [M]          the NoiseMapper's arguments
            p_Xhat [M], fwrd [M][M], I_X_Xhat           P_xhat(nm), nm.fwrd_transition_probability,
                                                         mutual_information_X_Xhat(nm, p_Xhat)
            x [B][S] int8, xhat [B][S] int8, y [B][S]   the draws and Bob's hard decisions
            terms [3][B][S]                             log2(...) of :259, :269 and :295 per sample
            totals [B][3]                               what montecarlo_information returns per block
            yhat [5][S][M]                              first 5 blocks: g_inv(n, k) for k != x_hat and
                                                        g_inv_search(n, x_hat) at k == x_hat
            n_overflow                                  exp calls that overflowed to inf
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "qam-reconciliation_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))

from qamreconciliation.alphabet import PAMAlphabet  # noqa: E402  (the reference build)
from qamreconciliation.noisemapper import NoiseMapper  # noqa: E402

from make_golden import alternating, noise_var  # noqa: E402

B, S, N_YHAT = 70, 37, 5

# c -> (bps, noise_var as a function of the alphabet, all-zero configuration?, probabilities)
CASES = {
    1: (1, lambda pa: pa.variance * 10 ** (-1.2), False, None),
    2: (2, lambda pa: noise_var(pa, 4.0), False, None),
    3: (2, lambda pa: 10 ** (-0.3), True, None),
    4: (2, lambda pa: noise_var(pa, 4.0), False, (0.1, 0.4, 0.3, 0.2)),
    5: (3, lambda pa: 10 ** (-0.8), False, None),
    6: (4, lambda pa: 10 ** (-1.3), False, None),
    7: (4, lambda pa: 10 ** (-3.5), False, None),   # exp under/overflow
    8: (2, lambda pa: noise_var(pa, -20.0), False, None),   # the CLI's default low end
}

N_OVERFLOW = [0]


def c_exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        N_OVERFLOW[0] += 1
        return math.inf


def c_log2(v):
    if v != v:
        return math.nan
    if v == 0.0:
        return -math.inf
    if v < 0.0:
        return math.nan
    return math.log2(v)


def c_div(a, b):
    """a / b with C semantics for b == 0."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def p_xhat(M, p, fw):
    """mutual_information.pyx:29-39"""
    res = [0.0] * M
    for i in range(M):
        res[i] = 0.0
        for j in range(M):
            res[i] += p[j] * fw[j][i]
    return res


def info_x_xhat(M, p, fw, pX):
    """mutual_information.pyx:152-172"""
    res = 0.0
    for j in range(M):
        sum_i = 0.0
        for i in range(M):
            tmp = 0.0
            if fw[j][i] > 0.0:
                tmp += c_log2(fw[j][i])
            if pX[i] > 0.0:
                tmp -= c_log2(pX[i])
            sum_i += tmp * fw[j][i]
        res += p[j] * sum_i
    return res


def block(nm, M, a, p, dF, fw, pX, tv, x_ind, y, xhat_ind, n, keep_yhat):
    """mutual_information.pyx:245-297 for one block; also the per-sample terms and y_hat."""
    N = len(x_ind)
    I0 = 0.0
    I1 = 0.0
    I2 = 0.0
    terms = np.empty((3, N))
    yh = np.empty((N, M)) if keep_yhat else None
    for q in range(N):
        cx, cxh = int(x_ind[q]), int(xhat_ind[q])
        x = a[cx]
        t0 = c_log2(c_div(pX[cxh], fw[cx][cxh]))                                    # :259
        I0 += t0
        tmp = p[cx]                                                                 # :264-269
        for k in (*range(cx), *range(cx + 1, M)):
            tmp += p[k] * c_exp((2 * y[q] - a[k] - x) * (a[k] - x) / tv)
        t1 = c_log2(tmp)
        I1 += t1
        acc = 0.0                                                                   # :274-295
        for k in (*range(cxh), *range(cxh + 1, M)):
            y_hat = float(nm.g_inv(n[q], k))
            if keep_yhat:
                yh[q, k] = y_hat
            tmp = p[cx]
            for m in (*range(cx), *range(cx + 1, M)):
                tmp += p[m] * c_exp((2 * y_hat - x - a[m]) * (a[m] - x) / tv)
            acc += c_div(dF[k], tmp)
        tmp = p[cx]
        y_hat = float(nm.g_inv_search(n[q], cxh))
        if keep_yhat:
            yh[q, cxh] = y_hat
        for m in (*range(cx), *range(cx + 1, M)):
            tmp += p[m] * c_exp((2 * y_hat - x - a[m]) * (a[m] - x) / tv)
        acc *= c_div(tmp, dF[cxh])
        acc += 1
        acc *= pX[cxh]
        t2 = c_log2(acc)
        I2 -= t2
        terms[:, q] = (t0, t1, t2)
    return (I0 / N, I1 / N, I2 / N), terms, yh


def gen_case(out, c):
    bps, nvf, base, probs = CASES[c]
    pa = PAMAlphabet(bps, 2.0) if probs is None else PAMAlphabet(bps, 2.0, np.array(probs))
    M = pa.order
    nv = float(nvf(pa))
    cfg = np.zeros(M, np.uint8) if base else alternating(M)
    nm = NoiseMapper(pa, nv, cfg)
    a = [float(v) for v in pa.constellation]
    p = [float(v) for v in pa.probabilities]
    dF = [float(v) for v in nm.delta_F_Y]
    fw = [[float(v) for v in row] for row in np.asarray(nm.fwrd_transition_probability)]
    tv = 2.0 * float(nm.noise_var)
    sigma = float(nm.noise_sigma)
    pX = p_xhat(M, [float(v) for v in nm.probabilities], fw)
    X = np.empty((B, S), np.int8)
    XH = np.empty((B, S), np.int8)
    Y = np.empty((B, S))
    T = np.empty((3, B, S))
    TOT = np.empty((B, 3))
    YH = np.empty((N_YHAT, S, M))
    N_OVERFLOW[0] = 0
    for f in range(B):
        np.random.seed(5000 + 100 * c + f)
        x_ind = np.asarray(pa.random_symbols(S)).astype(np.int64)
        y = np.asarray(pa.index_to_value(x_ind)).copy()
        for q in range(S):
            y[q] += sigma * np.random.randn()
        if f == 0:   # an array draw after random_symbols equals the S scalar draws
            np.random.seed(5000 + 100 * c + f)
            x2 = np.asarray(pa.random_symbols(S)).astype(np.int64)
            z = np.random.randn(S)
            y2 = np.asarray(pa.index_to_value(x2)) + sigma * z
            assert np.array_equal(x2, x_ind) and np.array_equal(y2.view(np.int64), y.view(np.int64)), c
        xh = np.asarray(nm.hard_decide_index(y)).astype(np.int64)
        n = np.asarray(nm.map_noise(y, xh)).copy()
        tot, terms, yh = block(nm, M, a, p, dF, fw, pX, tv, x_ind, y, xh, n, f < N_YHAT)
        X[f], XH[f], Y[f], T[:, f, :], TOT[f] = x_ind, xh, y, terms, tot
        if f < N_YHAT:
            YH[f] = yh
    finite = [float(np.isfinite(T[q]).mean()) for q in range(3)]
    # a condition on the reference's own values, not a measurement of the code under test
    assert min(finite) >= 0.9, (c, finite)
    k = f"c{c}_"
    out.update({k + "bps": bps, k + "noise_var": nv, k + "cfg": cfg, k + "probs": np.asarray(pa.probabilities),
                k + "p_Xhat": np.array(pX), k + "fwrd": np.array(fw), k + "I_X_Xhat": info_x_xhat(M, p, fw, pX),
                k + "x": X, k + "xhat": XH, k + "y": Y, k + "terms": T, k + "totals": TOT, k + "yhat": YH,
                k + "n_overflow": N_OVERFLOW[0]})
    print(f"  case {c}: {M}-PAM nv={nv:.4g} finite={['%.3f' % v for v in finite]} exp overflows={N_OVERFLOW[0]} "
          f"non-finite terms={int((~np.isfinite(T)).sum())} mean totals={TOT.mean(axis=0)} "
          f"I(X;Xhat)={out[k + 'I_X_Xhat']:.6f}", flush=True)
    return N_OVERFLOW[0] + int((~np.isfinite(T)).sum())


if __name__ == "__main__":
    out = {"n_cases": len(CASES), "B": B, "S": S}
    special = sum(gen_case(out, c) for c in CASES)
    assert special > 0, "no case holds a non-finite term or an overflowed exp"
    path = os.path.join(HERE, "mi.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"[golden] mi.npz: {size} bytes", flush=True)
    assert size < os.path.getsize(os.path.join(HERE, "interp.npz"))
