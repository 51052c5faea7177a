"""The frame-resident decode past one pass of its 512 threads, variables with no edge, and the
boundaries at which a code changes path.

* ``k_resident`` (decode_small.hip) holds a frame's messages and posteriors in 8 (E + V) bytes of
  dynamic LDS, at most 36 KiB, so V up to 2304 and C up to 1152: more than one pass of its check
  loop (512 checks a pass) and of its variable loop (1024 variables a trip), the ``lreg == false``
  path (V > 1024: LAPPRs re-read per iteration, the register path of regular variable degrees <= 3
  off), the wave-uniform ``break`` of a partial last check pass, the syndrome bit read from memory
  in later passes, and a last variable trip with one variable per lane.  RESIDENT lists codes that
  reach each of these.
* Variables with no edge: the reference allows them (vnum = max(e_to_v) + 1) and copies their
  input to the output with no addition, so -0.0 and NaN keep their bits.  ``irr_c6_1100`` and the
  two repack codes have ~ 1/6 isolated variables carrying -0.0, NaN, inf, -inf in frames that
  iterate to the end, converge at some t >= 1, and are exact codewords.
* Which path ran is read from the profiling counters (launch names ``resident_dD``, ``iter_dD``,
  ``check1_dD``, ``check_dD``) at the LDS cap of ``resident_code`` and at ``max_dv <= 64`` of
  ``iter_code``.
* Irregular variable degrees under the two-stream schedule's column repack on small codes.

Every frame of every run is compared with the oracle (oracle/qamr_oracle.c): success flag,
iteration count, final LAPPRs bit for bit, padding columns untouched.
"""
import functools

import numpy as np
import pytest

import decode_fixture as DF
from decode_fixture import (LD, MI, NEVER, REPACK_DEFAULTS, REPACK_RUNS, assert_path, assert_repack_counts,
                            decode_and_compare, deal_sockets, knobs, launches, oracle_of, predict_repack, profiled,
                            to_device)

pytestmark = pytest.mark.gpu

SPECIALS = np.array([-0.0, np.nan, np.inf, -np.inf])

# knobs the schedules below touch, with their defaults (every run sets all of them)
DEFAULTS = dict(split=3, resident=1, fused_iter=1, iter_streams=2)
# (label, knobs, path): default knobs, one launch per iteration (or the flat schedule where
# iter_code refuses the code), lock-step frame-parallel
SCHEDULES = [("default", {}, "resident"),
             ("resident off", dict(resident=0), "iter"),
             ("flat", dict(resident=0, fused_iter=0), "check")]


def dealt_code(dv, dc, rng):
    """deal_sockets with no socket left over, so variable v has degree dv[v]; the last variable
    has an edge (the reference sizes the code by max(e_to_v) + 1)."""
    dv = np.asarray(dv)
    assert dv.sum() % dc == 0 and dv[-1] >= 1
    vid, cid = deal_sockets(dv, dc, rng)
    assert np.array_equal(np.bincount(vid, minlength=dv.size), dv)
    return vid, cid


def irregular_code(N, dc, seed):
    """Variable degrees integers(0, 6): about N / 6 variables have no edge.  The last variable
    keeps at least one (the reference sizes the code by max(e_to_v) + 1); the first variables of
    degree >= 2 give up one socket each until the sockets are a multiple of dc."""
    rng = np.random.default_rng(seed)
    dv = rng.integers(0, 6, N)
    dv[-1] = max(dv[-1], 1)
    for v in np.flatnonzero(dv >= 2)[:dv.sum() % dc]:
        dv[v] -= 1
    return dealt_code(dv, dc, rng)


def hub_code(N, hub, dc, seed):
    """Variable 0 has degree hub, the others degree 2."""
    return dealt_code(np.r_[hub, np.full(N - 1, 2)], dc, np.random.default_rng(seed))


def _regular(*a):
    from qamr import codes

    return codes.regular_code(*a)


# name -> (graph, check degree, V, C, sigma range); E + V <= 4608 = the LDS cap of resident_code
RESIDENT = {
    # two full check passes; lreg false; second variable trip with one variable per lane
    "v2c3_1536": (lambda: _regular(1536, 2, 3, 1), 3, 1536, 1024, (0.7, 1.1)),
    # partial second check pass (238 checks): waves 4..7 leave, wave 3 is half live
    "v2c4_1500": (lambda: _regular(1500, 2, 4, 2), 4, 1500, 750, (0.5, 0.8)),
    # three check passes and three variable trips, D = 2, variable degree 1 (a tree)
    "v1c2_2304": (lambda: _regular(2304, 1, 2, 3), 2, 2304, 1152, (0.5, 0.8)),
    # regular variable degree 3 but V > 1024: the register path must switch itself off
    "v3c9_1152": (lambda: _regular(1152, 3, 9, 4), 9, 1152, 384, (0.5, 0.8)),
    # ~ 180 isolated variables, generic variable loop, V > 1024
    "irr_c6_1100": (lambda: irregular_code(1100, 6, 5), 6, 1100, None, (0.5, 0.8)),
}


def plant_specials(orc, vid, llr, word, sig, lo, hi, mi):
    """In frames [lo, hi): make one frame an exact codeword, then put -0.0, NaN, inf, -inf on the
    first four isolated variables of that frame, of the first frame that iterates to the end and
    of the first frame that converges at some t >= 1 (the oracle's decode of the frames as drawn
    says which: an isolated variable's LAPPR reaches no check, so planting changes no other
    value).  Returns (frames, isolated variables)."""
    iso = np.flatnonzero(np.bincount(vid, minlength=orc.vnum) == 0)[:SPECIALS.size]
    assert iso.size == SPECIALS.size
    synd = np.stack([orc.eval_syndrome(w) for w in word[lo:hi]])
    succ, its, _ = orc.decode_batch(llr[lo:hi], synd, mi)
    to_end = lo + int(np.flatnonzero(succ == 0)[0])
    conv = lo + int(np.flatnonzero((succ != 0) & (its >= 1))[0])
    cw = lo + int(np.flatnonzero((np.arange(lo, hi) != to_end) & (np.arange(lo, hi) != conv))[0])
    llr[cw] = 2 / sig[cw] ** 2 * (1 - 2.0 * word[cw])
    frames = np.array([to_end, conv, cw])
    llr[np.ix_(frames, iso)] = SPECIALS
    return frames, iso


def assert_special_frames(case, mi):
    """From the oracle alone: the three planted frames are of the three kinds, and the reference
    returns the planted bits."""
    succ, its, fin = oracle_of(case, mi)
    for frames, iso in case["planted"]:
        to_end, conv, cw = frames
        assert succ[to_end] == 0 and its[to_end] == mi, (succ[to_end], its[to_end])
        assert succ[conv] == 1 and its[conv] >= 1, (succ[conv], its[conv])
        assert succ[cw] == 1 and its[cw] == 0, (succ[cw], its[cw])
        assert_planted_bits(fin, case, frames, iso)


def assert_planted_bits(fin, case, frames, iso):
    got = np.ascontiguousarray(fin[np.ix_(frames, iso)]).view(np.int64)
    want = np.ascontiguousarray(case["llr"][np.ix_(frames, iso)]).view(np.int64)
    assert np.array_equal(got, want), (got, want)


def make_case(vid, cid, n, sigma, seed, plant=()):
    """DF.make_case; ``plant``: the (lo, hi) frame ranges that get special values on isolated
    variables (the case's ``planted``: one (frames, isolated variables) per range)."""
    return DF.make_case(vid, cid, n, sigma, seed, lambda orc, llr, word, sig: [
        plant_specials(orc, vid, llr, word, sig, lo, hi, MI) for lo, hi in plant])


@functools.lru_cache(maxsize=None)
def resident_case(name):
    graph, D, V, C, sigma = RESIDENT[name]
    vid, cid = graph()
    case = make_case(vid, cid, 96, sigma, 5, plant=[(0, 96)] if name.startswith("irr") else ())
    orc = case["orc"]
    assert orc.vnum == V and (C is None or orc.cnum == C) and orc.ednum + V <= 4608, (orc.vnum, orc.cnum, orc.ednum)
    assert np.array_equal(np.unique(np.bincount(cid)), [D])
    return case


def iter_launches(mi, ld):
    """One chain of iter_dD launches per stream: iter_streams = 2 ranges of 64-frame tiles."""
    return (mi + 1) * min(2, ld // 64)


def run_schedules(case, D, shapes, mis, schedules=SCHEDULES):
    """Every (B, ld) of shapes x max_iterations x schedule: equal to the oracle, on the path named."""
    import qamr

    dec = qamr.Decoder(case["vid"], case["cid"])
    assert dec.max_check_degree == D
    for B, ld in shapes:
        L, S = to_device(case, B, ld)
        for label, run, path in schedules:
            with knobs(DEFAULTS, **run):
                for mi in mis:
                    tag = (B, ld, label, mi)
                    with profiled():
                        decode_and_compare(dec, L, S, B, mi, oracle_of(case, mi), tag)
                        n = launches(D)
                    print(tag, n)
                    assert_path(path, mi, n, iter_launches(mi, ld))
    return dec


SHAPES = [(96, 128), (1, 64)]


@pytest.mark.parametrize("name", list(RESIDENT))
def test_resident_shapes_vs_oracle(gpu, name):
    """B = 96 in ld = 128 and B = 1 in ld = 64, max_iterations 1, 2, 30, under default knobs (one
    resident_dD launch), resident = 0 (iter_dD) and resident = 0, fused_iter = 0 (check_dD).  On
    the CPU first: some frames succeed, some fail, at >= 5 distinct stop iterations (the tree
    v1c2_2304: every frame stops at iteration 1); irr_c6_1100: the planted frames are of the three
    kinds and the reference returns the planted bits (assert_bit_exact then holds the device to
    them; NaN by pattern)."""
    case = resident_case(name)
    succ, its, _ = oracle_of(case, MI)
    if name == "v1c2_2304":
        assert succ.all() and (its == 1).all(), (succ.sum(), np.unique(its))
    else:
        assert 0 < succ.sum() < 96 and np.unique(its[succ != 0]).size >= 5, (succ.sum(), np.unique(its[succ != 0]))
    assert_special_frames(case, MI)
    run_schedules(case, RESIDENT[name][1], SHAPES, (1, 2, MI))


def test_isolated_variables_keep_input_bits(gpu):
    """irr_c6_1100, max_iterations = 30, the three schedules: at the isolated variables of the
    frame that iterates to the end, the frame that converges at t >= 1 and the codeword frame the
    output holds the input's bits (-0.0's sign, the NaN's payload, inf, -inf)."""
    import torch
    import qamr

    case = resident_case("irr_c6_1100")
    assert_special_frames(case, MI)
    (frames, iso), = case["planted"]
    dec = qamr.Decoder(case["vid"], case["cid"])
    L, S = to_device(case, 96, 128)
    for label, run, _ in SCHEDULES:
        with knobs(DEFAULTS, **run):
            fin, _, _ = dec.decode_device(L, S, 96, MI)
            torch.cuda.synchronize()
        assert_planted_bits(fin[:, :96].cpu().numpy().T, case, frames, iso)


def test_resident_lds_boundary(gpu):
    """resident_code (decode_small.hip): a code is frame-resident when 8 (E + V) + kResStaticLds <=
    min(80 KiB, the device's LDS per workgroup), kResStaticLds = 8192 + 8 * 576 * 8 = 45056, so
    E + V <= 4608.  Control first: regular_code(1008) (E + V = 4032) is resident (it would not be
    on a device that gives a workgroup less LDS than the rule assumes).  regular_code(1539, 2, 3)
    has E + V = 4617 and must take one launch per iteration instead, and equal the oracle."""
    assert 8 * 4608 + 45056 == 80 * 1024 == 81920
    control = make_case(*_regular(1008), 96, (0.5, 0.8), 5)
    assert control["orc"].ednum + control["orc"].vnum == 4032
    run_schedules(control, 6, SHAPES[:1], (2,), SCHEDULES[:1])
    over = make_case(*_regular(1539, 2, 3, 6), 96, (0.7, 1.1), 5)
    assert over["orc"].ednum + over["orc"].vnum == 4617 and 8 * 4617 + 45056 > 81920
    succ, _, _ = oracle_of(over, MI)
    assert 0 < succ.sum() < 96
    run_schedules(over, 3, SHAPES, (1, 2, MI), [("default", {}, "iter")] + SCHEDULES[1:])


@pytest.mark.parametrize("hub", [64, 66])
def test_max_var_degree_boundary(gpu, hub):
    """iter_code (decode_small.hip) takes max_dv <= 64.  401 variables, variable 0 of degree 64, the
    others of degree 2, dealt 6 per check (E = 864, C = 144): resident = 0 runs iter_d6.  400
    variables, variable 0 of degree 66, dealt 3 per check (E = 864, C = 288): resident = 0 runs
    the flat schedule (check_d3, no iter_d3).  Both are frame-resident under default knobs (a 64-
    and a 66-trip inner variable loop)."""
    N, dc = (401, 6) if hub == 64 else (400, 3)
    case = make_case(*hub_code(N, hub, dc, hub), 96, (0.5, 0.8), 5)
    orc = case["orc"]
    assert (orc.vnum, orc.ednum, orc.cnum) == (N, 864, 864 // dc)
    assert np.bincount(case["vid"]).max() == hub == np.bincount(case["vid"])[0]
    assert oracle_of(case, MI)[0].sum() > 0
    dec = run_schedules(case, dc, SHAPES[:1], (1, 2, MI),
                        [SCHEDULES[0], ("resident off", dict(resident=0), "iter" if hub == 64 else "check"), SCHEDULES[2]])
    assert dec.max_var_degree == hub


# ------------------------------------------------- irregular variables under the column repack
REPACK = {"irr6": (6, 21, (0.5, 0.8)), "irr12": (12, 22, (0.35, 0.6))}   # check degree, seed, sigma


@functools.lru_cache(maxsize=None)
def repack_case(name):
    dc, seed, sigma = REPACK[name]
    vid, cid = irregular_code(900, dc, seed)
    # special values in one frame of each kind in each range, inside the first 450 frames
    return make_case(vid, cid, LD, sigma, 1000 + seed, plant=[(0, 256), (256, 450)])


def assert_repack_inputs(name, case, B):
    """From the graph and the oracle alone: one check degree, variable degrees 0..5 with 100..200
    isolated; then assert_repack_counts (both ranges' running counts reach 80 % of their width,
    >= 5 distinct stops, both ranges are predicted to repack and end narrower than 256)."""
    assert np.array_equal(np.unique(np.bincount(case["cid"])), [REPACK[name][0]])
    deg = np.bincount(case["vid"], minlength=900)
    assert deg.size == 900 and deg.max() == 5 and 100 <= (deg == 0).sum() <= 200, np.bincount(deg)
    return assert_repack_counts(case, B, MI)


@pytest.mark.parametrize("name", list(REPACK))
def test_irregular_var_repack_vs_oracle(gpu, name):
    """900 variables of degrees 0..5 (~ 150 isolated), dealt 6 and 12 per check, ld = 512 with
    split_min_blocks = 0: B = 512 and 450 at max_iterations = 30 under the knob sets of the repack
    file's RUNS (REPACK_RUNS).  Every frame equals the oracle; with the default knobs the repack stats equal the
    prediction from the oracle's counts; with the repack or the lists off, and in lock-step,
    "never".  The planted frames (three kinds in each range) keep their special bits."""
    import qamr

    case = repack_case(name)
    dc = REPACK[name][0]
    assert_special_frames(case, MI)
    want = {B: assert_repack_inputs(name, case, B) for B in (LD, 450)}
    ref = oracle_of(case, MI)
    dec = qamr.Decoder(case["vid"], case["cid"])
    for B in (LD, 450):
        L, S = to_device(case, B, LD)
        for r, run in enumerate(REPACK_RUNS):
            tag = (name, B, run)
            with knobs(REPACK_DEFAULTS, **{"resident": 0, **run}), profiled():
                decode_and_compare(dec, L, S, B, MI, ref, tag)
                n = launches(dc)
                stats = dec.repack_stats(LD, MI)
            print(tag, n, "repack stats", stats, "predicted", want[B])
            assert_path("iter" if r == 6 and dc == 6 else "check", MI, n, iter_launches(MI, LD))
            if r == 0:
                assert stats == want[B] == predict_repack(ref[0], ref[1], B, MI), (tag, stats, want[B])
            elif r in (1, 4, 6):
                assert stats == NEVER, (tag, stats)
