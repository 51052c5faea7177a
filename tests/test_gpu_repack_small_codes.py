"""The column repack of the two-stream schedule on small codes with check degrees 11..16.

The repack tests of tests/test_gpu_timed_schedule.py all run the N=64800 DVB-S2-profile code
(check degrees 7 and one 6); the tests of other degrees run B = 70 (ld = 128), which never takes
``run_split2`` (it needs ld % 512 == 0).  Here V ~ 768 codes of variable degree 3 run at B <= 512
(ld = 512, two ranges of 256 columns) with knob ``split_min_blocks = 0``, so every decode takes
``run_split2`` with the device-decided repack (k_repack_rows), its transition sweeps (the first
variable and check sweep after a repack read the messages at the frames' old columns of the old
column set) and the narrow sweeps, on

* one unpacked class: ``reg11``, ``reg12``, ``reg16`` (degree > kPackMaxDeg = 10: the unpacked
  strict update, no narrow check sweep);
* ``side12``: ~90 % of the edges in degree-6 checks, ~10 % in degree-12 checks, which therefore
  run as the side class on the variable stream;
* ``half7_13``: half the edges in degree 7 (packed, narrow sweeps), half in degree 13, both in
  the main check sweep;
* ``mix12_16_5``: 45 % / 45 % / 10 % of the edges in degrees 12 / 16 / 5;
* the control ``reg7`` (knob ``resident = 0``): the packed path at the same shape.

Every frame of every run is compared with the oracle (oracle/qamr_oracle.c): success flag,
iteration count and final LAPPRs bit for bit.  The inputs are conditioned on the CPU: from the
oracle's (success, iterations) alone each range's running-frame count drops to at most 80 % of
its 256 columns before the last decision point, and the repacks the device must then decide
(``predict_repack`` of tests/decode_fixture.py: the rule of decode_repack.hip repack_go applied to
the oracle's counts) are compared
with ``Decoder.repack_stats``.
"""
import numpy as np
import pytest

from conftest import assert_bit_exact

from decode_fixture import (CODES, LD, MI, NEVER, H, assert_repack_inputs, decode_and_compare, knobs, oracle_of, running,
                            small_case, to_device)
from decode_fixture import REPACK_DEFAULTS as DEFAULTS
from decode_fixture import REPACK_RUNS as RUNS

pytestmark = pytest.mark.gpu


def _decode_runs(name, variant, B):
    import qamr

    case = small_case(name, variant)
    want = assert_repack_inputs(*CODES[name], case, B, MI)
    dec = qamr.Decoder(case["vid"], case["cid"])
    L, S = to_device(case, B, LD)
    base = dict(resident=0) if name == "reg7" else {}
    for mi in (1, 2, 3, MI):
        ref = oracle_of(case, mi)
        for r, run in enumerate(RUNS if mi == MI else (RUNS[0], RUNS[6])):
            tag = (name, variant, B, mi, run)
            with knobs(DEFAULTS, **{**base, **run}):
                try:
                    decode_and_compare(dec, L, S, B, mi, ref, tag)
                finally:
                    stats = dec.repack_stats(LD, mi)
                    print(tag, "repack stats", stats)
            if mi != MI:
                continue
            if r == 0:
                print(tag, "predicted", want)
                (rep0, rep1), (w0, w1) = stats
                assert rep0 >= 1 and rep1 >= 1, stats        # each range repacked
                assert w0 < H and w1 < H, stats              # and ended narrower
                last = running(ref[0], ref[1], B, mi - 2)    # count at the last decision point
                if min(last) <= 64:   # the narrow sweeps ran (beside the unpacked classes)
                    assert min(w0, w1) <= 64, (stats, last)
                assert stats == want, (stats, want)
            elif r in (1, 4, 6):
                assert stats == NEVER, (tag, stats)          # repack off / no lists / lock-step


@pytest.mark.parametrize("variant", ["clean", "special"])
@pytest.mark.parametrize("name", list(CODES))
def test_repack_small_codes_vs_oracle(gpu, name, variant):
    """B = 512, max_iterations 1, 2, 3 (default knobs with split_min_blocks = 0, and lock-step)
    and 30 (the seven knob sets of RUNS): all 512 frames equal the oracle's in every run; at 30
    with the default knobs both ranges repacked, ended narrower than 256 columns and exactly as
    the oracle's counts predict; with the repack or the lists off, and in lock-step, never.
    ``clean``: all LAPPRs finite (the finite flag set: packed classes run the one-instruction
    clamp).  ``special``: frames 0..3 and 256..259 are codewords (stop at iteration 0), frames 8
    and 300 carry inf, -inf, -0.0, 0.0, NaN (flag clear: the NaN-preserving clamp)."""
    _decode_runs(name, variant, LD)


@pytest.mark.parametrize("B", [450, 257])
@pytest.mark.parametrize("name", ["reg12", "side12"])
def test_repack_small_codes_ragged_batch(gpu, name, B):
    """The first B frames of the clean case in ld = 512: range 1 starts with 194 live columns of
    256 (below the threshold before any frame stops) or holds a single frame; the same runs and
    assertions, and the padding columns [B, ld) of the output keep the caller's values (the
    decode's first variable sweep used to copy the input's padding columns into them)."""
    _decode_runs(name, "clean", B)


def test_repack_small_code_graph_replay(gpu):
    """reg12, clean, max_iterations = 30, captured into a HIP graph on a side stream and
    replayed (as test_repack_decode_is_asynchronous_and_capturable does for the DVB-S2 code):
    the replay equals the oracle on all frames and the device repacked inside the graph."""
    import torch
    import qamr

    case = small_case("reg12", "clean")
    want = assert_repack_inputs(*CODES["reg12"], case, LD, MI)
    s2, i2, f2 = oracle_of(case, MI)
    dec = qamr.Decoder(case["vid"], case["cid"])
    L, S = to_device(case, LD, LD)
    with knobs(split_min_blocks=0):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dec.decode_device(L, S, LD, MI)  # warm-up: allocates this stream's workspace
        torch.cuda.synchronize()
        fin = torch.full_like(L, np.nan)
        succ = torch.zeros(LD, dtype=torch.uint8, device="cuda")
        its = torch.zeros(LD, dtype=torch.int32, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dec.decode_device(L, S, LD, MI, fin, succ, its)
        g.replay()
        torch.cuda.synchronize()
        stats = dec.repack_stats(LD, MI, stream=s)
    assert np.array_equal(succ.cpu().numpy(), s2) and np.array_equal(its.cpu().numpy(), i2)
    assert_bit_exact(fin.cpu().numpy().T, f2)
    assert min(stats[0]) >= 1 and stats == want, (stats, want)
