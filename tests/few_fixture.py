"""Codes, frames and helpers shared by the few-frame decode tests (tests/test_few_cpu.py,
tests/test_gpu_few_frames.py); every case is computed once, shared and never modified.

* ``degree_case(D, variant)``: the regular (3, D) code of tests/test_gpu_degree_matrix.py and five
  of its first 64 frames, picked from the oracle's decode at 30 iterations: one replaced by its
  exact codeword (stops at iteration 0), the successful frames with the smallest and the largest
  stop iteration >= 1, and two more; in ``special`` one of those two carries inf, -inf, -0.0, 0.0,
  NaN on its first five variables (the batch's finite flag is then clear).
* ``mixed_code()``: V = 702, check classes of degrees 2, 3, 6, 7, 10, 11, 16 with 40, 65 (a wave
  plus one lane), 130, 60, 30, 1 and 20 checks, parallel edges, every sixth variable isolated,
  variable 0 a hub of degree 70.  ``mixed_case()``: frames of it picked in the same way.
"""
import functools

import numpy as np

import decode_fixture as DF
import oracle as O

MI = 30
MIS = (0, 1, 2, MI)
PAD = 7.0
SPECIAL5 = DF.SPECIAL5
ISOLATED4 = [-0.0, np.nan, np.inf, -np.inf]

MIXED_V = 702
MIXED_CLASSES = [(2, 40), (3, 65), (6, 130), (7, 60), (10, 30), (11, 1), (16, 20)]
MIXED_HUB_DEGREE = 70
MIXED_SEED = 2716
# per-frame noise sigma ~ U(lo, hi) of the mixed code's frames, picked on the CPU from the oracle
# alone: the pool's successful frames stop at several different iterations and some frames fail
MIXED_SIGMA = (0.55, 0.95)


def mixed_code():
    """(vid, cid): the sockets (hub x 70, every other connected variable x 3 or 4) shuffled by
    default_rng(seed) and dealt check-major to the classes' checks in a shuffled order."""
    return DF.hub_code(MIXED_V, MIXED_CLASSES, MIXED_HUB_DEGREE, MIXED_SEED)


def mixed_isolated():
    return np.array([v for v in range(MIXED_V) if v % 6 == 2])


def _pick(orc, word, synd, sig, llr, special_first5):
    """Five frames of the pool, in the order (latest stop, codeword, earliest stop, other, other
    [special]): the first three alone already meet assert_conditions."""
    s, it, _ = orc.decode_batch(llr, synd, MI)
    ok = np.flatnonzero((s != 0) & (it >= 1))
    assert ok.size >= 2, "the pool needs converging frames"
    lo, hi = ok[np.argmin(it[ok])], ok[np.argmax(it[ok])]
    assert it[lo] < it[hi]
    rest = [f for f in range(len(s)) if f not in (lo, hi)]
    cw, o1, o2 = rest[0], rest[1], rest[2]
    sel = np.array([hi, cw, lo, o1, o2])
    L = llr[sel].copy()
    L[1] = 2 / sig[cw] ** 2 * (1 - 2.0 * word[cw])  # the exact codeword: (1, 0)
    if special_first5:
        L[4, :5] = SPECIAL5
    S = synd[sel].copy()
    return L, S


def _finish(vid, cid, orc, L, S):
    L.setflags(write=False)
    S.setflags(write=False)
    ref = {}
    for mi in MIS:
        ref[mi] = orc.decode_batch(L, S, mi)
        for a in ref[mi]:
            a.setflags(write=False)
    return dict(vid=vid, cid=cid, orc=orc, llr=L, synd=S, ref=ref)


def assert_conditions(ref, frames=slice(None)):
    """From the oracle alone, before any GPU output: at 30 iterations at least two distinct stop
    iterations >= 1, at 2 at least one frame that ends unsuccessful."""
    s30, i30, _ = ref[MI]
    s30, i30 = s30[frames], i30[frames]
    assert len(set(i30[(s30 != 0) & (i30 >= 1)].tolist())) >= 2, (s30, i30)
    assert (ref[2][0][frames] == 0).any(), ref[2][0]
    assert (ref[MI][0][frames] != 0).any() and (ref[MI][1][frames] == 0).any()  # the codeword stops at 0


@functools.lru_cache(maxsize=None)
def degree_case(D, variant):
    base = DF.case_of(D, "clean")  # the degree matrix's case: its first 64 frames
    orc = base["orc"]
    llr, synd, word, sig = (base[k][:64] for k in ("llr", "synd", "word", "sig"))
    assert np.array_equal(synd[0], orc.eval_syndrome(word[0]))
    assert variant in ("clean", "special")
    L, S = _pick(orc, word, synd, sig, llr, variant == "special")
    assert np.isfinite(L).all() == (variant == "clean")
    return _finish(base["vid"], base["cid"], orc, L, S)


@functools.lru_cache(maxsize=None)
def mixed_case():
    """Five frames of the mixed code (order as _pick); frames 1.. carry -0.0, NaN, inf, -inf on
    their first four isolated variables (an isolated variable's LAPPR reaches no check; frame 0
    stays finite, so B = 1 runs the finite clamp and B = 3 the NaN-preserving one)."""
    vid, cid = mixed_code()
    orc = O.OracleCode(vid, cid)
    assert orc.vnum == MIXED_V and orc.cnum == sum(n for _, n in MIXED_CLASSES)
    pairs = np.stack([vid, cid], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs), "the code needs parallel edges"
    vdeg = np.bincount(vid, minlength=MIXED_V)
    assert vdeg[0] == MIXED_HUB_DEGREE > 64 and (vdeg[mixed_isolated()] == 0).all()
    assert abs(mixed_isolated().size - MIXED_V / 6) < 2
    rng = np.random.default_rng(MIXED_SEED + 1)
    llr, synd, word, sig = DF.draw_frames(orc, rng, 48, MIXED_SIGMA)
    L, S = _pick(orc, word, synd, sig, llr, False)
    L[1:, mixed_isolated()[:4]] = ISOLATED4
    return _finish(vid, cid, orc, L, S)


def write_edges(path, vid, cid):
    """The edge-list file tests/native/few_layout_check.cpp reads."""
    with open(path, "w") as f:
        f.write(f"{len(vid)}\n")
        for v, c in zip(vid, cid):
            f.write(f"{int(v)} {int(c)}\n")
