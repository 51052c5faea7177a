"""The few-frame decode schedule (decode_few.hip run_few: k_few_check, k_few_var) and the frame-major
device entry point qr_decode_frames_device / Decoder.decode_frames_device.

Every frame of every decode is compared with the oracle (oracle/qamr_oracle.c): success flag,
iteration count and final LAPPRs bit for bit; the output is allocated with one extra row filled
with a pad value that must stay untouched.  Which path ran is read from the profiling counters of
the same decode: the few-frame launches are named ``few_check`` / ``few_var`` / ``few_var_init``,
the frame-parallel ones ``check1_dD`` / ``check_dD`` / ``iter_dD`` / ``resident_dD``.  Knobs are
set explicitly (``few_max = 8`` unless a case says otherwise) under decode_fixture.knobs.

1. degree matrix: regular (3, D) codes, D = 2..16, finite and special inputs, 5 frames with a
   codeword, an early and a late stop, at max_iterations 0, 1, 2, 30;
2. seven degree classes in one code (one of 1 check, one of 65, one of 130), parallel edges,
   isolated variables with special values, a hub variable of degree 70; B = 1 and 3;
3. the N = 64 800 code, B = 1 and 3 at 50 iterations, also through Decoder.decode / decode_batch;
4. routing: B > few_max, few_max = 0, a degree-17 check and a frame-resident code fall back;
5. a captured decode replayed on new inputs.
"""
import numpy as np
import pytest

from conftest import assert_bit_exact

import few_fixture as F
import oracle as O
from decode_fixture import knobs, profiled

pytestmark = pytest.mark.gpu

FRAME_PARALLEL = ("check", "check1", "iter", "resident")


def _counters():
    """Launch counts by profile name: the few-frame ones, and the frame-parallel ones summed over
    the plain name and every degree suffix."""
    from qamr import _lib

    n = {k: _lib.profile_query(k)[1] for k in ("few_check", "few_var", "few_var_init")}
    for k in FRAME_PARALLEL:
        n[k] = _lib.profile_query(k)[1] + sum(_lib.profile_query(f"{k}_d{d}")[1] for d in range(2, 33))
    return n


def _assert_few(n, mi, classes=1):
    """run_few ran alone: 2 parity sweeps (1 at max_iterations 0) + mi check sweeps, one launch per
    class each; mi variable sweeps after the first."""
    assert all(n[k] == 0 for k in FRAME_PARALLEL), n
    assert n["few_check"] == ((2 if mi > 0 else 1) + mi) * classes, (n, mi)
    assert n["few_var_init"] == 1 and n["few_var"] == mi, (n, mi)


def _assert_frame_parallel(n):
    assert n["few_check"] == 0 and n["few_var"] == 0 and n["few_var_init"] == 0, n
    assert n["check1"] + n["iter"] + n["resident"] > 0, n


def _decode(dec, llr, synd, mi, ref, tag, **kw):
    """One decode_frames_device of the given frames into an output of B + 1 rows; returns the
    launch counters of the decode."""
    import torch

    B = llr.shape[0]
    L = torch.from_numpy(np.array(llr)).cuda()   # (copies: the cases are read-only)
    S = torch.from_numpy(np.array(synd)).cuda()
    fin =torch.full((B + 1, llr.shape[1]), F.PAD, dtype=torch.float64, device="cuda")
    with profiled():
        _, succ, its = dec.decode_frames_device(L, S, mi, final=fin, **kw)
        torch.cuda.synchronize()
        n = _counters()
    s2, i2, f2 = ref
    print(tag, n, succ.cpu().numpy(), its.cpu().numpy())
    assert np.array_equal(succ.cpu().numpy(), s2), tag
    assert np.array_equal(its.cpu().numpy(), i2), tag
    assert_bit_exact(fin[:B].cpu().numpy(), f2)
    assert bool((fin[B] == F.PAD).all()), tag
    return n


# ------------------------------------------------------------------ 1. degree matrix
@pytest.mark.parametrize("variant", ["clean", "special"])
@pytest.mark.parametrize("D", range(2, 17))
def test_few_degree_matrix_vs_oracle(gpu, D, variant):
    import qamr

    case = F.degree_case(D, variant)
    F.assert_conditions(case["ref"])
    dec = qamr.Decoder(case["vid"], case["cid"])
    assert dec.max_check_degree == D
    with knobs(few_max=8, resident=0):
        for mi in F.MIS:
            n = _decode(dec, case["llr"], case["synd"], mi, case["ref"][mi], (D, variant, mi))
            _assert_few(n, mi)


# ------------------------------------------------------------------ 2. several classes
@pytest.mark.parametrize("B", [1, 3])
def test_few_mixed_classes_vs_oracle(gpu, B):
    import qamr

    case = F.mixed_case()
    F.assert_conditions(case["ref"], slice(0, 3))
    dec = qamr.Decoder(case["vid"], case["cid"])
    assert dec.max_check_degree == 16 and dec.max_var_degree == F.MIXED_HUB_DEGREE
    iso = F.mixed_isolated()[:4]
    with knobs(few_max=8, resident=1):  # several classes: never frame-resident
        for mi in F.MIS:
            ref = tuple(a[:B] for a in case["ref"][mi])
            if B > 1:  # the isolated variables keep their input bits
                assert_bit_exact(ref[2][1:, iso], np.tile(F.ISOLATED4, (B - 1, 1)))
            n = _decode(dec, case["llr"][:B], case["synd"][:B], mi, ref, ("mixed", B, mi))
            _assert_few(n, mi, classes=len(F.MIXED_CLASSES))


# ------------------------------------------------------------------ 3. N = 64 800
def _dvbs2_frames(dec, snr, seed, cols):
    """Frames of a 4-PAM batch formed as tests/test_gpu_timed_schedule.py forms its batches
    (SofteningPipeline.generate + demap), frame-major on the host."""
    import torch
    from qamr.pipeline import SofteningPipeline

    pipe = SofteningPipeline(dec, bps=2, snr_db=snr, batch=64, max_iterations=50)
    b = pipe.generate(torch.Generator(device="cuda").manual_seed(seed))
    lappr = pipe.demap(b)
    torch.cuda.synchronize()
    ct = torch.as_tensor(cols, device=lappr.device)
    return lappr[:, ct].T.contiguous().cpu().numpy(), b.synd[:, ct].T.contiguous().cpu().numpy()


def test_few_dvbs2_vs_oracle(gpu):
    """Three frames of a 4.0 dB batch (they converge) decode as B = 3, one of a 3.0 dB batch (it
    runs all 50 iterations) as B = 1: through decode_frames_device, and through the drop-in's
    Decoder.decode / decode_batch (qr_decode_host), which take the same path."""
    import qamr
    from qamr import codes

    vid, cid = codes.dvbs2_like_half()
    dec = qamr.Decoder(vid, cid)
    orc = O.OracleCode(vid, cid)
    L3, S3 = _dvbs2_frames(dec, 4.0, 340, [0, 31, 63])
    L1, S1 = _dvbs2_frames(dec, 3.0, 130, [5])
    ref3, ref1 = orc.decode_batch(L3, S3, 50), orc.decode_batch(L1, S1, 50)
    print("oracle", ref3[0], ref3[1], ref1[0], ref1[1])
    assert ref3[0].all() and len(set(ref3[1].tolist())) >= 2 and ref1[1][0] == 50
    with knobs(few_max=8):
        _assert_few(_decode(dec, L3, S3, 50, ref3, "dvbs2 B=3"), 50, classes=2)
        _assert_few(_decode(dec, L1, S1, 50, ref1, "dvbs2 B=1"), 50, classes=2)
        with profiled():
            s3, i3, f3 = dec.decode_batch(L3, S3, 50)
            s1, i1, f1 = dec.decode(L1[0], S1[0], 50)
            n = _counters()
        assert n["few_check"] == 2 * 52 * 2 and all(n[k] == 0 for k in FRAME_PARALLEL), n
    assert np.array_equal(s3, ref3[0]) and np.array_equal(i3, ref3[1])
    assert_bit_exact(f3, ref3[2])
    assert (s1, i1) == (int(ref1[0][0]), int(ref1[1][0]))
    assert_bit_exact(f1, ref1[2][0])


# ------------------------------------------------------------------ 4. routing
def _with_degree17(vid, cid):
    """The code plus one check of degree 17 on variables 0..16."""
    c = int(cid.max()) + 1
    return np.concatenate([vid, np.arange(17)]).astype(np.int64), np.concatenate([cid, np.full(17, c)]).astype(np.int64)


def test_few_routing(gpu):
    import qamr

    case = F.degree_case(7, "clean")
    dec = qamr.Decoder(case["vid"], case["cid"])
    L, S, ref = case["llr"], case["synd"], case["ref"][F.MI]
    first = lambda k: tuple(a[:k] for a in ref)  # noqa: E731
    with knobs(few_max=4, resident=0):  # B above few_max: frame-parallel
        _assert_frame_parallel(_decode(dec, L, S, F.MI, ref, "few_max=4 B=5"))
        _assert_few(_decode(dec, L[:4], S[:4], F.MI, first(4), "few_max=4 B=4"), F.MI)
    with knobs(few_max=0, resident=0):  # off: every B
        for B in (1, 5):
            _assert_frame_parallel(_decode(dec, L[:B], S[:B], F.MI, first(B), f"few_max=0 B={B}"))
    with knobs(few_max=8, resident=1):  # a frame-resident code keeps k_resident
        n = _decode(dec, L, S, F.MI, ref, "resident=1")
        _assert_frame_parallel(n)
        assert n["resident"] == 1 and n["check1"] == 0 and n["iter"] == 0, n
    # one check of degree 17 (the runtime-degree kernel's): today's path, at B = 1 too
    vid17, cid17 = _with_degree17(case["vid"], case["cid"])
    orc17 = O.OracleCode(vid17, cid17)
    S17 = np.concatenate([S, np.zeros((S.shape[0], 1), np.uint8)], 1)
    dec17 = qamr.Decoder(vid17, cid17)
    assert dec17.max_check_degree == 17
    with knobs(few_max=8, resident=0):
        for B in (1, 5):
            r = orc17.decode_batch(L[:B], S17[:B], F.MI)
            _assert_frame_parallel(_decode(dec17, L[:B], S17[:B], F.MI, r, f"degree 17 B={B}"))


def test_few_max_survives_sizing(gpu):
    """The workspace size covers both routes: sized with the few-frame path off, the decode runs
    with it on (and the other way round) on that same workspace."""
    import qamr

    case = F.mixed_case()
    dec = qamr.Decoder(case["vid"], case["cid"])
    with knobs(few_max=0):
        need0 = dec.frames_workspace_bytes(5, F.MI)
        with knobs(few_max=8):
            assert dec.frames_workspace_bytes(5, F.MI) == need0
            n = _decode(dec, case["llr"], case["synd"], F.MI, case["ref"][F.MI], "sized off, run on")
            _assert_few(n, F.MI, classes=len(F.MIXED_CLASSES))
        _assert_frame_parallel(_decode(dec, case["llr"], case["synd"], F.MI, case["ref"][F.MI], "sized on, run off"))


# ------------------------------------------------------------------ 5. graph capture
def test_few_decode_graph_capture(gpu):
    """One decode_frames_device call (B = 2, the mixed code) captured after an eager call; the
    inputs are then replaced in place and the replay equals the oracle on the new inputs."""
    import qamr
    import torch

    case = F.mixed_case()
    dec = qamr.Decoder(case["vid"], case["cid"])
    V = case["llr"].shape[1]
    to = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    with knobs(few_max=8):
        L, S = to(case["llr"][3:5]), to(case["synd"][3:5])
        fin = torch.full((3, V), F.PAD, dtype=torch.float64, device="cuda")
        succ = torch.zeros(2, dtype=torch.uint8, device="cuda")
        its = torch.zeros(2, dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dec.decode_frames_device(L, S, F.MI, fin, succ, its)  # eager: allocates this stream's workspace
        torch.cuda.synchronize()
        assert np.array_equal(its.cpu().numpy(), case["ref"][F.MI][1][3:5])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dec.decode_frames_device(L, S, F.MI, fin, succ, its)
        L.copy_(to(case["llr"][0:2]))
        S.copy_(to(case["synd"][0:2]))
        fin.fill_(F.PAD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
    s2, i2, f2 = (a[0:2] for a in case["ref"][F.MI])
    assert np.array_equal(succ.cpu().numpy(), s2) and np.array_equal(its.cpu().numpy(), i2)
    assert_bit_exact(fin[:2].cpu().numpy(), f2)
    assert bool((fin[2] == F.PAD).all())
