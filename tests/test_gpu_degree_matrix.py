"""Check degrees 2..16 in every decode schedule, in both clamp variants.

The decoder (decoder.hip, decode_small.hip) instantiates its check update per degree: ``k_check<D>`` for D = 2..16 (the
frame-parallel sweep of the lock-step and two-stream schedules, with the repack's transition
mapping), and ``check_narrow<D>``, ``k_iter<D>`` and ``k_resident<D>`` for D = 2..10
(kPackMaxDeg); the packed update's rounds (strict_pack.hpp) are laid out at compile time from D,
so every D is its own code.  Here one regular (3, D) code of V ~ 770 per degree decodes 512 frames
(ld = 512) in each schedule that can run it:

1. two-stream (``split_min_blocks = 0``, ``resident = 0``) with the device-decided repack, its
   transition sweeps and, for D <= 10, the narrow sweeps;
2. two-stream with ``repack = 0``; 3. with ``compact = 0``;
4. lock-step frame-parallel (``split = 1``, ``fused_iter = 0``, ``resident = 0``);
5. D <= 10: one launch per iteration (``resident = 0``, ``split = 1``; ``iter_streams`` 2, 1);
6. D <= 10: frame-resident, default knobs.

Every frame of every run is compared with the oracle (oracle/qamr_oracle.c): success flag,
iteration count, final LAPPRs bit for bit, padding columns untouched.  Which path ran is read from
the profiling counters (the launches are named ``resident_dD``, ``iter_dD``, ``check1_dD``,
``check_dD``), in the same run whose outputs are compared.  The inputs are conditioned on the CPU
as in tests/test_gpu_repack_small_codes.py; the codes and frames are ``case_of`` of
tests/decode_fixture.py (tests/few_fixture.py takes its frames from them).
"""
import pytest

from decode_fixture import (LD, MI, NEVER, assert_path, assert_repack_inputs, case_of, decode_and_compare, knobs, launches,
                            oracle_of, predict_repack, profiled, to_device, v_of)

pytestmark = pytest.mark.gpu

DEGREES = tuple(range(2, 17))
PACK_MAX = 10   # decode_dev.hpp kPackMaxDeg: narrow sweeps, k_iter and k_resident exist up to here

# the knobs the runs touch and their defaults (every run sets all of them)
DEFAULTS = dict(split=3, compact=1, repack=1, split_min_blocks=1024, resident=1, fused_iter=1, iter_streams=2)
# run -> (knobs, path, max_iterations); "path" names the launches that must have run
TWO_STREAM = dict(split_min_blocks=0, resident=0)
LOCKSTEP = dict(split=1, fused_iter=0, resident=0)
ITER = dict(split=1, resident=0)


def runs_of(D):
    runs = [("two-stream", TWO_STREAM, "check", (1, 2, 3, MI)),
            ("repack off", dict(TWO_STREAM, repack=0), "check", (MI,)),
            ("lists off", dict(TWO_STREAM, compact=0), "check", (MI,)),
            ("lock-step", LOCKSTEP, "check", (1, 2, 3, MI))]
    if D <= PACK_MAX:
        runs += [("iter x2", dict(ITER, iter_streams=2), "iter", (MI,)),
                 ("iter x1", dict(ITER, iter_streams=1), "iter", (MI,)),
                 ("resident", {}, "resident", (1, 2, 3, MI))]
    return runs


def assert_inputs(D, case):
    """Conditions on the inputs, from the graph and the oracle alone (before any GPU output):
    those of assert_repack_inputs (each range's running count reaches 80 % of its width, >= 5
    distinct stop iterations, both ranges are predicted to repack and end narrower than 256) and,
    for a packed degree, a predicted final width of 64 in at least one range, so check_narrow<D>
    must run."""
    V = v_of(D)
    reps, widths = assert_repack_inputs(V, [(D, 3 * V // D)], case, LD, MI)
    if D <= PACK_MAX:
        assert min(widths) == 64, widths
    return reps, widths


@pytest.mark.parametrize("variant", ["clean", "special"])
@pytest.mark.parametrize("D", DEGREES)
def test_degree_matrix_vs_oracle(gpu, D, variant):
    """``clean``: all LAPPRs finite (the finite flag set: the one-instruction clamp).  ``special``:
    frames 0..3 and 256..259 are codewords (stop at iteration 0), frames 8 and 300 carry inf, -inf,
    -0.0, 0.0, NaN (flag clear: the NaN-preserving clamp).  The two-stream run's repack stats equal
    the prediction from the oracle's counts at every max_iterations; with the repack or the lists
    off they are "never"."""
    import qamr

    case = case_of(D, variant)
    assert_inputs(D, case)
    dec = qamr.Decoder(case["vid"], case["cid"])
    assert dec.max_check_degree == D
    L, S = to_device(case, LD, LD)
    for label, run, path, mis in runs_of(D):
        with knobs(DEFAULTS, **run):
            for mi in mis:
                tag = (D, variant, label, mi)
                ref = oracle_of(case, mi)
                with profiled():
                    decode_and_compare(dec, L, S, LD, mi, ref, tag)
                    n = launches(D)
                print(tag, n)
                assert_path(path, mi, n, (mi + 1) * {**DEFAULTS, **run}["iter_streams"])
                if label == "two-stream":
                    stats, want = dec.repack_stats(LD, mi), predict_repack(ref[0], ref[1], LD, mi)
                    print(tag, "repack stats", stats, "predicted", want)
                    assert stats == want, (tag, stats, want)
                elif label in ("repack off", "lists off"):
                    assert dec.repack_stats(LD, mi) == NEVER, tag
