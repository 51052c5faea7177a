"""Check degrees above 16 in every decode path that can run them, and every degree against the
reference's own records.

Degrees above the templated range 2..16 run one runtime-degree kernel (decoder.hip
``k_check_generic``: the forward values parked in the HBM scratch ``fb``), always in the lock-step
schedule (``decode_batch_device``: the two-stream schedule needs ``max_deg <= 16``).  What runs
where:

* ``test_high_degree_matrix``: the regular (3, D) codes of ``HIGH_DEGREES`` (17, 18, 22, 27, 30, 33,
  65, 100, 255; V ~ 800) and the high-degree mixed code (classes of degrees 7, 12, 17, 30, 64; a
  class of 65 checks and one of a single check, parallel edges, isolated variables, a hub), 512
  frames at ld = 512 (four 128-column tiles; with ``check_ft`` 64 / 256 eight / two), clean and
  special (codewords that stop at iteration 0; inf, -inf, -0.0, 0.0, NaN) variants, in the runs
  of ``RUNS``: default knobs at max_iterations 0, 1, 2, 3, 30; ``split_min_blocks = 0`` (the
  two-stream schedule asked for: a code with a degree above 16 stays lock-step, one launch per
  class and sweep); the active-frame lists off; ``nt`` off; 16 checks per thread with a ragged
  last workgroup (``min_blocks = 0``) at 1 and 30; frame tiles of 64 and 256 columns;
  ``check_tail`` off.  Every frame of every run equals the oracle
  (success, iterations, final LAPPRs bit for bit, padding untouched); the counters of the same
  run show ``check1_dD`` / ``check_dD`` and no ``resident_*`` / ``iter_*`` launch, and the
  decode never repacked.  The default run at 30 iterations is also compared with
  tests/golden/decoder_degrees.npz, the compiled reference's own records, with no oracle between.
* ``test_templated_degrees_vs_reference_records``: D = 2..16 with default knobs (frame-resident for
  D <= 10, lock-step above) against the same records.
* ``test_high_degree_ragged_batches``: B = 1, 65, 450 in ld = 512 and B = ld = 64, 128, 256.
* ``test_high_degree_few_frames_take_the_frame_parallel_path``: decode_frames_device and
  decode_batch at B = 1, 5, 16.
* ``test_high_degree_graph_capture``, ``test_process_check_node_special_values`` (degrees 17 and
  100; special values, magnitudes 1e-310 .. 1e300, both syndrome bits).

tests/test_gpu_degrees.py keeps single checks of degree 17 .. 255 among low-degree ones at
ld = 64 / 128 and the workspace's closed form (which lists the mixed code too).  The inputs are
conditioned on the CPU, from the oracle alone (tests/test_decode_fixture_cpu.py); the oracle is
pinned to the reference's records in tests/test_decoder_degrees_cpu.py.
"""
import numpy as np
import pytest

from conftest import assert_bit_exact, golden

import oracle as O
from decode_fixture import (HIGH_DEGREES, LD, MI, NEVER, SPECIAL5, GoldenDegrees, assert_golden_inputs, assert_golden_records,
                            assert_high_conditions, case_of, decode_and_compare, high_case, high_classes, knobs, launches,
                            oracle_of, profiled, scattered_code, to_device)

pytestmark = pytest.mark.gpu

KEYS = HIGH_DEGREES + ("mix",)
# the knobs the runs touch (and those that route a decode) and their defaults: every run sets all
DEFAULTS = dict(split=3, compact=1, nt=1, min_blocks=2048, check_ft=128, check_per=16, check_tail=4, repack=1,
                split_min_blocks=1024, resident=1, fused_iter=1)
# (label, knobs, max_iterations)
RUNS = [
    ("default", {}, (0, 1, 2, 3, MI)),          # split = 3 must stay lock-step
    # a degree <= 16 code would now take the two-stream schedule (a launch per half: check1 = 2)
    ("split asked", dict(split_min_blocks=0), (2, MI)),
    ("lists off", dict(compact=0), (MI,)),
    ("nt off", dict(nt=0), (MI,)),
    ("per 16", dict(min_blocks=0), (1, MI)),    # 32 checks per workgroup: a ragged last one
    ("ft 64", dict(check_ft=64, check_per=3, min_blocks=0), (MI,)),   # eight frame tiles, 12 checks per workgroup
    ("ft 256", dict(check_ft=256), (MI,)),      # two frame tiles, one check per workgroup
    ("tail off", dict(check_tail=0), (MI,)),    # the runtime-degree kernel ignores it either way
]


@pytest.fixture(scope="module")
def gold():
    return GoldenDegrees(golden("decoder_degrees.npz"))


def golden_name(key, variant):
    return f"himix-{variant}" if key == "mix" else f"deg{key}-{variant}"


def assert_lockstep_launches(key, mi, tag):
    """From the counters of the decode just run: every class's first sweep ran as check1_dD when
    max_iterations >= 1 and its later sweeps as check_dD when > 1, once per sweep (one class launch
    covers all frame tiles); nothing frame-resident or one-launch-per-iteration ran."""
    for d, _ in high_classes(key):
        n = launches(d)
        print(tag, f"d{d}", n)
        assert n == dict(resident=0, iter=0, check1=min(mi, 1), check=max(mi - 1, 0)), (tag, d, n)


@pytest.mark.parametrize("variant", ["clean", "special"])
@pytest.mark.parametrize("key", KEYS)
def test_high_degree_matrix(gpu, gold, key, variant):
    import qamr

    case = high_case(key, variant)
    assert_high_conditions(case, variant)
    name = golden_name(key, variant)
    assert_golden_inputs(gold, name, case)
    dec = qamr.Decoder(case["vid"], case["cid"])
    assert dec.max_check_degree == max(d for d, _ in high_classes(key)) > 16
    L, S = to_device(case, LD, LD)
    for label, run, mis in RUNS:
        with knobs(DEFAULTS, **run):
            for mi in mis:
                tag = (key, variant, label, mi)
                with profiled():
                    got = decode_and_compare(dec, L, S, LD, mi, oracle_of(case, mi), tag)
                    assert_lockstep_launches(key, mi, tag)
                assert dec.repack_stats(LD, mi) == NEVER, tag
                if label == "default" and mi == MI:   # the reference's own records, no oracle between
                    assert_golden_records(gold, name, mi, *got, tag=tag)


@pytest.mark.parametrize("variant", ["clean", "special"])
@pytest.mark.parametrize("D", range(2, 17))
def test_templated_degrees_vs_reference_records(gpu, gold, D, variant):
    """Default knobs: D <= 10 decodes frame-resident, D > 10 lock-step (a half's check launch is
    far below split_min_blocks).  Success, iterations and every frame's digest at 30 iterations
    equal what the compiled reference returned."""
    import qamr
    import torch

    case = case_of(D, variant)
    name = golden_name(D, variant)
    assert_golden_inputs(gold, name, case)
    dec = qamr.Decoder(case["vid"], case["cid"])
    L, S = to_device(case, LD, LD)
    with knobs(DEFAULTS):
        with profiled():
            fin, succ, its = dec.decode_device(L, S, LD, MI)
            torch.cuda.synchronize()
            n = launches(D)
    print((D, variant), n)
    assert n["iter"] == 0 and (n["resident"], n["check1"]) == ((1, 0) if D <= 10 else (0, 1)), n
    assert_golden_records(gold, name, MI, succ.cpu().numpy(), its.cpu().numpy(), fin.cpu().numpy().T)


@pytest.mark.parametrize("B,ld", [(1, 512), (65, 512), (450, 512), (64, 64), (128, 128), (256, 256)])
@pytest.mark.parametrize("key", [30, "mix"])
def test_high_degree_ragged_batches(gpu, key, B, ld):
    """The first B frames of the special variant in ld columns (the padding columns' LAPPRs and
    syndromes zero): every frame equals the oracle's decode of it, the output's columns [B, ld)
    keep 7.0.  ld = 64, 128, 256: frame tiles of 64, 128 and 128 columns and other sizes of the fb
    scratch; B = 1: only a codeword; 65: a wavefront plus one lane; 450: a partly filled last tile."""
    import qamr

    case = high_case(key, "special")
    dec = qamr.Decoder(case["vid"], case["cid"])
    L, S = to_device(case, B, ld)
    with knobs(DEFAULTS):
        for mi in (1, MI):
            tag = (key, B, ld, mi)
            with profiled():
                decode_and_compare(dec, L, S, B, mi, oracle_of(case, mi), tag)
                assert_lockstep_launches(key, mi, tag)


def _few_counters():
    from qamr import _lib

    return {k: _lib.profile_query(k)[1] for k in ("few_check", "few_var", "few_var_init")}


@pytest.mark.parametrize("B", [1, 5, 16])
def test_high_degree_few_frames_take_the_frame_parallel_path(gpu, B):
    """B <= few_max frames of a code with a check degree above 16 never take the few-frame
    schedule: decode_frames_device (frame-major tensors) and decode_batch (host arrays) run the
    lock-step frame-parallel decode, and every frame equals the oracle's."""
    import qamr
    import torch

    case = case_of(30, "special")
    dec = qamr.Decoder(case["vid"], case["cid"])
    s2, i2, f2 = (a[:B] for a in oracle_of(case, MI))
    Lh, Sh = np.array(case["llr"][:B]), np.array(case["synd"][:B])
    with knobs(dict(DEFAULTS, few_max=16)):
        fin = torch.full((B + 1, Lh.shape[1]), 7.0, dtype=torch.float64, device="cuda")
        with profiled():
            _, succ, its = dec.decode_frames_device(torch.from_numpy(Lh).cuda(), torch.from_numpy(Sh).cuda(), MI, final=fin)
            torch.cuda.synchronize()
            assert _few_counters() == dict(few_check=0, few_var=0, few_var_init=0)
            assert_lockstep_launches(30, MI, ("frames", B))
        assert np.array_equal(succ.cpu().numpy(), s2) and np.array_equal(its.cpu().numpy(), i2)
        assert_bit_exact(fin[:B].cpu().numpy(), f2)
        assert bool((fin[B] == 7.0).all())
        with profiled():
            s1, i1, f1 = dec.decode_batch(Lh, Sh, MI)
            assert _few_counters() == dict(few_check=0, few_var=0, few_var_init=0)
            assert_lockstep_launches(30, MI, ("host", B))
        assert np.array_equal(s1, s2) and np.array_equal(i1, i2)
        assert_bit_exact(f1, f2)


def test_high_degree_graph_capture(gpu):
    """The default decode of the degree-30 code (lock-step on the caller's stream: no parallel
    branches) captured in a graph after an eager call: the replay equals the eager decode bit for
    bit, and the oracle."""
    import qamr
    import torch

    case = case_of(30, "special")
    dec = qamr.Decoder(case["vid"], case["cid"])
    L, S = to_device(case, LD, LD)
    with knobs(DEFAULTS):
        ref = [x.clone() for x in dec.decode_device(L, S, LD, MI)]  # eager (also allocates)
        fin = torch.full_like(L, 7.0)
        succ = torch.zeros(LD, dtype=torch.uint8, device="cuda")
        its = torch.zeros(LD, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            dec.decode_device(L, S, LD, MI, fin, succ, its)
        fin.fill_(7.0)
        succ.zero_()
        its.zero_()
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(succ, ref[1]) and torch.equal(its, ref[2])
    assert torch.equal(fin.view(torch.int64), ref[0].view(torch.int64))
    s2, i2, f2 = oracle_of(case, MI)
    assert np.array_equal(succ.cpu().numpy(), s2) and np.array_equal(its.cpu().numpy(), i2)
    assert_bit_exact(fin.cpu().numpy().T, f2)


def _node_messages(rng, d):
    """v2c vectors of a degree-d check.  ``strong``: every |m| >= 4, so every output is an ordinary
    non-zero double; on that base one subnormal (1e-310), two of them, +-1e3 and +-1e300, and all six
    magnitudes; each special value alone on the first, a middle and the last edge; all five at
    once on shuffled edges (also among weak messages, whose box-plus underflows at d = 100)."""
    def strong():
        return rng.choice([-1.0, 1.0], d) * (4.0 + 3.0 * np.abs(rng.standard_normal(d)))

    def put(m, values):
        m[rng.permutation(d)[:len(values)]] = values
        return m

    weak = rng.standard_normal(d) * rng.choice([0.5, 3.0, 20.0], d)
    out = [("strong", strong()), ("weak", weak), ("one subnormal", put(strong(), [1e-310])),
           ("two subnormals", put(strong(), [1e-310, -1e-310])), ("huge", put(strong(), [1e3, -1e3, 1e300, -1e300])),
           ("all magnitudes", put(strong(), [1e-310, -1e-310, 1e3, -1e3, 1e300, -1e300]))]
    for v in SPECIAL5:
        for pos in (0, d // 2, d - 1):
            m = put(strong(), [1e-310, 1e3, -1e300])
            m[pos] = v
            out.append((f"{v!r} at {pos}", m))
    out += [("all five", put(strong(), SPECIAL5)), ("all five among weak", put(weak.copy(), SPECIAL5))]
    return out


@pytest.mark.parametrize("d", [17, 100])
def test_process_check_node_special_values(gpu, d):
    """process_check_node (decode_api.hip k_check_nodes, a kernel of its own) on a check of degree
    d against the oracle's, bit for bit, for both syndrome bits; the messages of every other edge
    stay as they were."""
    import qamr

    rng = np.random.default_rng(1000 + d)
    V = 120
    vid, cid = scattered_code(rng, [d] + [3] * 40, V)
    dec = qamr.Decoder(vid, cid)
    orc = O.OracleCode(vid, cid)
    E, C = vid.size, int(cid.max()) + 1
    own = np.flatnonzero(cid == 0)
    other = np.flatnonzero(cid != 0)
    assert own.size == d
    for bit in (0, 1):
        synd = rng.integers(0, 2, C).astype(np.uint8)
        synd[0] = bit
        for label, m in _node_messages(rng, d):
            v2c = rng.standard_normal(E)
            v2c[own] = m
            c0 = rng.standard_normal(E)
            c1, c2 = c0.copy(), c0.copy()
            dec.process_check_node(0, synd, c1, v2c)
            orc.process_check_node(0, synd, c2, v2c)
            try:
                assert_bit_exact(c1, c2)
            except AssertionError as e:
                raise AssertionError(f"degree {d}, syndrome bit {bit}, {label}: {e}") from None
            assert_bit_exact(c1[other], c0[other])
            if label == "strong":   # the update is not vacuous: every own message is new, finite, non-zero
                assert np.isfinite(c2[own]).all() and (c2[own] != c0[own]).all() and (c2[own] != 0).all()
