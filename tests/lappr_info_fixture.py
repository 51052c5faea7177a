"""The host evaluator of the LAPPR information rate (include/qamr.h "LAPPR information rate"): the
reference of tests/test_lappr_info_cpu.py, tests/test_gpu_lappr_info.py and their debug rerun.

Per element and scale it evaluates ``t = m * LOG2E + log2(1.0 + exp(-|x|))`` with ``math.exp`` / ``math.log2``
(libm per element, the convention of tests/math_fixture.py; numpy's vectorised routines are others), every
operation a separately rounded Python float operation, and adds in the normative order: chunks of ``CHUNK``
symbols from 0.0 in ascending s, the chunks from 0.0 in ascending order, the frames from 0.0 in ascending f.
"""
import functools
import math

import numpy as np

CHUNK = 256                      # QR_LAPPR_INFO_CHUNK
LOG2E = 1.4426950408889634
INF, NAN = math.inf, math.nan
SPECIALS = (INF, -INF, NAN, 0.0, -0.0, 5e-324, -5e-324, 1e-320, -1e-320, 36.7, -36.7, 37.5, -37.5, 708.4, -708.4,
            745.2, -745.2, 1000.0, -1000.0)
SCALES = (1.0, 0.5, 0.0, -1.0, 1e-3, 0.8, 1.25, 2.0, 0.25, 0.6, 0.7, 0.9, 1.1, 1.5, 3.0, 0.1)   # 16: a test takes the first A
PAD = -7.25                      # the value of output cells that must stay untouched


def term(x):
    """t of one scaled, signed LAPPR x (the straight-line form)."""
    m = x if x > 0 else 0.0
    return m * LOG2E + math.log2(1.0 + math.exp(-abs(x)))


def term_branch(x):
    """The same quantity by cases: log2(1 + exp(x)) for x <= 0, x LOG2E + log2(1 + exp(-x)) otherwise (NaN: NaN)."""
    if x != x:
        return NAN
    if x <= 0:
        return math.log2(1.0 + math.exp(x))
    return x * LOG2E + math.log2(1.0 + math.exp(-x))


def signed(alpha, L, w):
    """x = alpha * L (one rounding), negated when the word's bit is 0."""
    x = alpha * L
    return -x if w == 0 else x


def evaluate(lappr, word, bps, alphas):
    """lappr float64 [B, S * bps], word uint8 [B, S * bps] (frame-major, element s * bps + k) ->
    (loss float64 [A, bps, B], errors int64 [bps, B], total float64 [A, bps], total_errors int64 [bps])."""
    lappr = np.asarray(lappr, np.float64)
    word = np.asarray(word, np.uint8)
    B, V = lappr.shape
    S = V // bps
    assert V == S * bps and word.shape == lappr.shape
    A = len(alphas)
    loss = np.zeros((A, bps, B))
    errors = np.zeros((bps, B), np.int64)
    for f in range(B):
        Lf, wf = lappr[f].tolist(), word[f].tolist()
        for k in range(bps):
            Lk, wk = Lf[k::bps], wf[k::bps]
            errors[k, f] = sum(1 for L, w in zip(Lk, wk) if (0 if L >= 0 else 1) != w)
            for a, alpha in enumerate(alphas):
                alpha = float(alpha)
                acc = 0.0
                for q0 in range(0, S, CHUNK):
                    c = 0.0
                    for L, w in zip(Lk[q0:q0 + CHUNK], wk[q0:q0 + CHUNK]):
                        c += term(signed(alpha, L, w))
                    acc += c
                loss[a, k, f] = acc
    total = np.zeros((A, bps))
    for a in range(A):
        for k in range(bps):
            acc = 0.0
            for f in range(B):
                acc += float(loss[a, k, f])
            total[a, k] = acc
    return loss, errors, total, errors.sum(axis=1)


def rates(total, B, S):
    """I_k(alpha) = 1.0 - total[a][k] / (B S), I(alpha) their sum from 0.0 over ascending k -> (I [A], I_level [A, bps])."""
    A, bps = total.shape
    I_level = np.array([[1.0 - float(total[a, k]) / float(B * S) for k in range(bps)] for a in range(A)])
    I = np.array([functools.reduce(lambda u, v: u + v, I_level[a].tolist(), 0.0) for a in range(A)])
    return I, I_level


# ------------------------------------------------------------------ inputs
def alternating(M):
    return (np.arange(M) % 2).astype(np.uint8)


def oracle_frames(bps, snr_db, S, B, seed):
    """B frames of S symbols through the oracle alone (alternating configuration, step 2): Bob's bits and
    demap_lappr_array(n_hat, x) -> (lappr [B, S * bps], word [B, S * bps])."""
    import oracle as O

    M = 1 << bps
    a = 2.0 * (np.arange(M) - (M - 1) / 2.0)
    Es = float(np.mean(a * a))
    N0 = Es * 10 ** (-snr_db / 10) / 2
    onm = O.OracleNoiseMapper(bps, 2.0, N0, alternating(M))
    assert np.array_equal(onm.constellation, a)
    rng = np.random.default_rng(seed)
    lappr = np.empty((B, S * bps))
    word = np.empty((B, S * bps), np.uint8)
    for f in range(B):
        x = rng.integers(0, M, S)
        y = a[x] + math.sqrt(N0) * rng.standard_normal(S)
        xh, nh, bits = bob(onm, y)
        lappr[f] = onm.demap_lappr_array(nh, x.astype(np.int64))
        word[f] = bits
    return lappr, word


def bob(onm, y):
    """Bob's side of the oracle: (x_hat int64 [S], n_hat float64 [S], bits uint8 [S * bps])."""
    y = np.ascontiguousarray(y, np.float64)
    xh = np.ascontiguousarray(onm.hard_decide_index(y), np.int64)
    nh = np.ascontiguousarray(onm.map_noise(y, xh), np.float64)
    bits = np.ascontiguousarray(onm.symbols_to_bits(xh), np.uint8)
    return xh, nh, bits


@functools.lru_cache(None)
def motivating_frame():
    """The issue's condition: 4-PAM, step 2, 3.0 dB, alternating configuration, default_rng(1), 4 000 symbols ->
    (x int64, y float64, lappr float64 [8000], word uint8 [8000], N0) from the oracle."""
    import oracle as O

    a = np.array([-3.0, -1.0, 1.0, 3.0])
    Es = 5.0
    N0 = Es * 10 ** (-0.3) / 2
    rng = np.random.default_rng(1)
    x = rng.integers(0, 4, 4000)
    y = a[x] + math.sqrt(N0) * rng.standard_normal(4000)
    onm = O.OracleNoiseMapper(2, 2.0, N0, alternating(4))
    xh, nh, bits = bob(onm, y)
    lappr = onm.demap_lappr_array(nh, x.astype(np.int64))
    return x.astype(np.int64), y, np.ascontiguousarray(lappr, np.float64), bits, N0


def plant_specials(lappr, bps):
    """SPECIALS written over lappr [B, S * bps] at the chunk edges of the first frame (the first and last symbol
    of every chunk, the levels in turn) and, all of them, into the last frame from its end backwards."""
    B, V = lappr.shape
    S = V // bps
    edges = sorted({s for q0 in range(0, S, CHUNK) for s in (q0, min(q0 + CHUNK, S) - 1)})
    for i, s in enumerate(edges):
        lappr[0, s * bps + i % bps] = SPECIALS[i % len(SPECIALS)]
    n = min(len(SPECIALS), V)
    lappr[B - 1, V - n:] = SPECIALS[:n]
    return lappr
