"""Generate tests/golden/binary_channel.npz: the binary-channel code evaluation of sims/sim_decode.py
(= sims/sim_direct.py) and sims/sim_bsc.py, decoded by the REFERENCE's compiled Decoder and Matrix.

Run where the reference build is available, as tests/golden/make_golden_interp.py:

    make -C oracle ref
    PYTHONPATH=oracle/_ref python3 tests/golden/make_golden_binary.py

The sim scripts themselves are `__main__`-only and import galois and parfor, so the LLRs are formed
here with numpy expressions of the same operations in the same order (sim_decode.py:69-71, :98-100,
sim_bsc.py:58-61), and the frame loops below are the scripts' loops over recorded per-frame results.
Every array stored is data: seeded inputs and what the reference returned for them.

Code: qamr.codes.regular_code(1008), 30 iterations, 16 frames per case.  Cases (prefix "c<i>_"):

  0  biawgn       -1.5 dB  alpha 1.0      3  biawgn_hard  0.0 dB        5  bsc  r = 0.07
  1  biawgn       -0.5 dB  alpha 1.0      4  biawgn_hard  1.0 dB        6  bsc  r = 0.04
  2  biawgn       -1.5 dB  alpha 0.7  (the words and noise of case 0: alpha only scales the LLRs)

The normal and uniform draws are taken in float32 and stored as such (every float32 is a double, so
the arithmetic under test is the same double arithmetic; a double plane per case would push the file
past the size of interp.npz, which the fixture must not exceed).

Per case: channel, point, alpha, coef, vsqrt (BIAWGN) -- the host scalars of the formulas;
  word [16][126] (packbits), z or u [16][1008] float32;
  llr [4][1008], final [4][1008]: the first 4 frames;
  synd [16][63] (packbits), success [16], iters [16], err_k [16], err_n [16]: per-frame bit errors
    (bit = final < 0) over the first K = 504 bits and over all N = 1008;
  BIAWGN: loop_args [2][2] = (simloops, minerr), loop_counts [2][5] = {bit errors, frame errors,
    successes, iteration sum, frames} at the stop, loop_tuple [2][3] = (ber, fer, iters);
  BSC: loop_args [2][3] = (niters, minerr, index bound: -1 = the script's max(20, niters // 100)),
    loop_counts, loop_tuple alike (errors over N).

Edge planes of the LLR kernels:
  edge_z [n], edge_w [n]: z in {0, +-1e-300, +-1, +-1e300, +-inf, NaN}, plus per point the z found by
    search for which vsqrt * z rounds to exactly -1 and +1 (the sum is then 0 against w = 0 / 1: sign gives
    0 and LLR0 = inf gives inf * 0 = NaN), against w = 0 and 1;
  edge_pts [2] = (1.0, 30.0) dB; edge_coef [2][2], edge_vsqrt [2] (soft, hard per point; LLR0 = inf at
    30 dB); edge_llr [2][2][n] (point, soft / hard, element);
  bsc_edge_r, bsc_edge_coef, bsc_edge_u [m], bsc_edge_w [m], bsc_edge_llr [m], bsc_edge_rx [m]:
    u in {0, r, nextafter(r, 0), nextafter(r, 1), 1 - 2^-53} against w = 0 and 1.

The generator asserts: for each channel the harder point has at least 3 failed and at least 3
successful frames among its 16; at least one stored stop is decided by the index bound and at least
one by the error count; the file is no larger than interp.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "qam-reconciliation_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))

from scipy.special import erfc  # noqa: E402

from qamreconciliation.decoder import Decoder  # noqa: E402  (the reference build)
from qamreconciliation.matrix import Matrix  # noqa: E402

from qamr import codes  # noqa: E402  (synthetic code generators; pure numpy)

FRAMES, MAXITER, N = 16, 30, 1008
# (channel, point, alpha, rng seed)
CASES = (
    ("biawgn", -1.5, 1.0, 5100), ("biawgn", -0.5, 1.0, 5101), ("biawgn", -1.5, 0.7, 5100),
    ("biawgn_hard", 0.0, 1.0, 5103), ("biawgn_hard", 1.0, 1.0, 5104),
    ("bsc", 0.07, 1.0, 5105), ("bsc", 0.04, 1.0, 5106),
)
HARDER = {"biawgn": 0, "biawgn_hard": 3, "bsc": 5}
BIAWGN_LOOPS = ((16, 20), (16, 100))
BSC_LOOPS = ((16, 20, 2), (16, 20, -1))


def biawgn_scalars(x, alpha, hard):
    v = (10 ** (-x / 10)) / 2
    vsqrt = np.sqrt(v)
    if not hard:
        return 2 * alpha / v, vsqrt
    err_prob = 0.5 * erfc(1 / (np.sqrt(2) * vsqrt))
    with np.errstate(divide="ignore"):
        return np.log((1 - err_prob) / err_prob), vsqrt


def biawgn_llr(coef, vsqrt, word, z, hard):
    w = np.array(word, dtype=np.double)
    with np.errstate(invalid="ignore", over="ignore"):
        if hard:
            return coef * np.sign((1 - 2.0 * w + vsqrt * z))
        return coef * (-2 * w + 1 + vsqrt * z)


def bsc_llr(coef, r, word, u):
    rx = word ^ (u < r).astype(np.ubyte)
    return coef * (1 - 2 * np.array(rx, dtype=np.double)), rx


def biawgn_loop(per_frame, K, simloops, minerr):
    """sim_decode.py:90-124 over recorded frames (success, iterations, errors over K)."""
    err = ferr = its = succ = 0
    for wc in range(simloops):
        s, i, e = per_frame[wc]
        if s:
            its += i
            succ += 1
        if e:
            ferr += 1
            err += e
        if err >= minerr and wc > simloops / 20:
            break
    wc += 1
    return [err, ferr, succ, its, wc], (err / (wc * K), ferr / wc, 0 if succ == 0 else its / succ)


def bsc_loop(per_frame, Nbits, niters, minerr, bound):
    """sim_bsc.py:54-82 over recorded frames (success, iterations, errors over N)."""
    err = ferr = its = succ = 0
    m = max(20, niters // 100) if bound < 0 else bound
    for it in range(1, niters + 1):
        s, i, e = per_frame[it - 1]
        if e > 0:
            err += e
            ferr += 1
        if s:
            succ += 1
            its += i
        if err > minerr and it > m:
            break
    return [err, ferr, succ, its, it], (err / (it * Nbits), ferr / it, its / succ if succ > 0 else 0)


def zero_makers(vsqrt):
    """z with vsqrt * z == -1 and == +1 exactly after rounding, if a double does it."""
    out = []
    for target in (-1.0, 1.0):
        z = target / vsqrt
        cand = [z]
        lo = hi = z
        for _ in range(4):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            cand += [lo, hi]
        hit = [c for c in cand if vsqrt * c == target]
        out += hit[:1]
    return out


def gen_cases(out):
    vid, cid = codes.regular_code(N)
    dec, mat = Decoder(vid, cid), Matrix(vid, cid)
    K = mat.vnum - mat.cnum
    by_index, by_count = 0, 0
    for c, (channel, point, alpha, seed) in enumerate(CASES):
        rng = np.random.default_rng(seed)
        k = f"c{c}_"
        W = rng.integers(0, 2, (FRAMES, N)).astype(np.ubyte)
        if channel == "bsc":
            r = np.float64(point)
            coef = np.log2(1 - r) - np.log2(r)
            noise = rng.random((FRAMES, N), dtype=np.float32)
            out[k + "u"] = noise
        else:
            hard = channel == "biawgn_hard"
            coef, vsqrt = biawgn_scalars(point, alpha, hard)
            noise = rng.standard_normal((FRAMES, N), dtype=np.float32)
            out[k + "z"] = noise
            out[k + "vsqrt"] = vsqrt
        L = np.empty((FRAMES, N)); Fin = np.empty((FRAMES, N)); Sy = np.empty((FRAMES, mat.cnum), np.uint8)
        Su = np.empty(FRAMES, np.uint8); It = np.empty(FRAMES, np.int32)
        Ek = np.empty(FRAMES, np.int32); En = np.empty(FRAMES, np.int32)
        for f in range(FRAMES):
            z = noise[f].astype(np.float64)
            llr = bsc_llr(coef, r, W[f], z)[0] if channel == "bsc" else biawgn_llr(coef, vsqrt, W[f], z, hard)
            synd = np.asarray(mat.eval_syndrome(W[f]), np.uint8)
            ok, it, fin = dec.decode(np.ascontiguousarray(llr, np.float64), synd, MAXITER)
            fin = np.asarray(fin)
            bits = (fin < 0).astype(np.ubyte) ^ W[f]
            L[f], Fin[f], Sy[f], Su[f], It[f], Ek[f], En[f] = llr, fin, synd, ok, it, bits[:K].sum(), bits.sum()
        out.update({k + "channel": channel, k + "point": point, k + "alpha": alpha, k + "coef": coef,
                    k + "word": np.packbits(W, axis=1), k + "llr": L[:4], k + "final": Fin[:4],
                    k + "synd": np.packbits(Sy, axis=1), k + "success": Su, k + "iters": It,
                    k + "err_k": Ek, k + "err_n": En})
        counts, tuples = [], []
        if channel == "bsc":
            per = [(int(Su[f]), int(It[f]), int(En[f])) for f in range(FRAMES)]
            args = BSC_LOOPS
            for niters, minerr, bound in args:
                cnt, tup = bsc_loop(per, N, niters, minerr, bound)
                counts.append(cnt); tuples.append(tup)
                if cnt[4] < niters:
                    run = np.cumsum(En)
                    first = int(np.argmax(run > minerr))      # 0-based frame where the count part first holds
                    by_index += first < cnt[4] - 1
                    by_count += first == cnt[4] - 1
        else:
            per = [(int(Su[f]), int(It[f]), int(Ek[f])) for f in range(FRAMES)]
            args = BIAWGN_LOOPS
            for simloops, minerr in args:
                cnt, tup = biawgn_loop(per, K, simloops, minerr)
                counts.append(cnt); tuples.append(tup)
                if cnt[4] < simloops:
                    run = np.cumsum(Ek)
                    first = int(np.argmax(run >= minerr))
                    by_index += first < cnt[4] - 1
                    by_count += first == cnt[4] - 1
        out.update({k + "loop_args": np.array(args, np.int64), k + "loop_counts": np.array(counts, np.int64),
                    k + "loop_tuple": np.array(tuples, np.float64)})
        print(f"  case {c}: {channel} {point} alpha={alpha} coef={coef!r} successes={int(Su.sum())}/16 "
              f"err_k={Ek.tolist()} stops={[cn[4] for cn in counts]}", flush=True)
        if HARDER[channel] == c:
            assert 3 <= int(Su.sum()) <= FRAMES - 3, (channel, point, int(Su.sum()))
    out["n_cases"] = len(CASES)
    assert by_index >= 1 and by_count >= 1, (by_index, by_count)
    print(f"  stops decided by the index bound: {by_index}, by the error count: {by_count}", flush=True)


def gen_edges(out):
    pts = (1.0, 30.0)
    base = [0.0, 1e-300, -1e-300, 1.0, -1.0, 1e300, -1e300, np.inf, -np.inf, np.nan]
    extra = []
    for x in pts:
        extra += zero_makers(biawgn_scalars(x, 1.0, False)[1])
    zs = np.array(base + extra)
    z = np.repeat(zs, 2)
    w = np.tile(np.array([0, 1], np.ubyte), zs.size)
    coef = np.empty((2, 2)); vs = np.empty(2); llr = np.empty((2, 2, z.size))
    for p, x in enumerate(pts):
        for h in (0, 1):
            coef[p, h], vs[p] = biawgn_scalars(x, 1.0, bool(h))
            llr[p, h] = biawgn_llr(coef[p, h], vs[p], w, z, bool(h))
    assert np.isinf(coef[1, 1]) and np.isfinite(coef[0, 1])
    assert np.isnan(llr[1, 1][~np.isnan(z)]).any(), "no inf * 0 in the edge plane"
    print(f"  edge: {z.size} elements, zero makers {extra}, NaN at 30 dB hard: {int(np.isnan(llr[1, 1]).sum())}")
    out.update(edge_z=z, edge_w=w, edge_pts=np.array(pts), edge_coef=coef, edge_vsqrt=vs, edge_llr=llr)
    r = np.float64(0.07)
    us = np.array([0.0, r, np.nextafter(r, 0), np.nextafter(r, 1), 1 - 2.0 ** -53])
    u = np.repeat(us, 2)
    bw = np.tile(np.array([0, 1], np.ubyte), us.size)
    bc = np.log2(1 - r) - np.log2(r)
    bl, rx = bsc_llr(bc, r, bw, u)
    out.update(bsc_edge_r=r, bsc_edge_coef=bc, bsc_edge_u=u, bsc_edge_w=bw, bsc_edge_llr=bl, bsc_edge_rx=rx)


if __name__ == "__main__":
    out = {}
    gen_cases(out)
    gen_edges(out)
    path = os.path.join(HERE, "binary_channel.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"[golden] binary_channel.npz: {size} bytes", flush=True)
    assert size <= os.path.getsize(os.path.join(HERE, "interp.npz")), size
