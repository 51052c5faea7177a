"""The memory contract of the entries that take a caller's workspace (include/qamr.h): the library
writes nothing outside the bytes it asked for, reads nothing inside them that the same call has not
written, leaves its inputs alone, and refuses a base that is not 256-byte aligned before any launch.

No parity test can see a violation: every other workspace of the suite comes from ``torch.empty``
through ``Decoder._workspace``, where the caching allocator's rounding absorbs an overrun and a
stale read sees zeros or what the same decode of the same case left.  Here every call runs on a
workspace of exactly the size the library asked for, between two guards, prepared by
tests/workspace_fixture.py: "zero", "typed" (NaNs of a known payload, set flags, valid-but-wrong
columns, counts and RangeSel states) and "leftover" (the bytes a repacking decode of another code at
another max_iterations left in its workspace).  Within a row the fills run in that order, so a
stale read shows first under a fill whose every value is in range.

Every result is compared with the oracle (or the entry's own reference) bit for bit; there is no
tolerance anywhere.  The cases are the shared, cached ones of decode_fixture, few_fixture and the
other GPU test files; the codes have V = 700 .. 1200, a test is a few decodes.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import assert_bit_exact, golden

import few_fixture
import workspace_fixture as W
from decode_fixture import (LD, MI, PAD, REPACK_DEFAULTS, assert_path, assert_repack_counts, case_of, himix_case, knobs,
                            launches, oracle_of, predict_repack, profiled, small_case, to_device)

pytestmark = pytest.mark.gpu

# every knob the rows touch, with its default: a run sets all of them
KNOBS = dict(REPACK_DEFAULTS, fused_iter=1, iter_streams=2)
TWO_STREAM = dict(split_min_blocks=0)
DECODE_LAUNCH_NAMES = ("status", "var", "var_init", "repack", "repack_out", "few_check", "few_var", "few_var_init")


def never(ld):
    """repack stats of a decode that never repacked"""
    return (0, 0), (ld // 2, ld // 2)


@functools.lru_cache(maxsize=None)
def _decoder(name):
    import qamr

    case = _CASES[name]()
    return case, qamr.Decoder(case["vid"], case["cid"])


def _resident_case():
    """130 frames of the RESIDENT code v3c9_1152 of tests/test_gpu_resident_shapes.py (its own
    cached case has 96): regular variable degree 3, V > 1024."""
    import test_gpu_resident_shapes as RS

    graph, D, V, Cn, sigma = RS.RESIDENT["v3c9_1152"]
    case = RS.make_case(*graph(), 130, sigma, 5)
    assert D == 9 and case["orc"].vnum == V and case["orc"].cnum == Cn
    return case


_CASES = {
    "reg7": lambda: small_case("reg7", "special"),
    "reg12": lambda: small_case("reg12", "special"),
    "mix12_16_5": lambda: small_case("mix12_16_5", "special"),
    "himix": lambda: himix_case("special"),
    "deg17": lambda: case_of(17, "special"),
    "resident": functools.lru_cache(maxsize=None)(_resident_case),
    "few": few_fixture.mixed_case,
}
DONOR_MI = 12


@functools.lru_cache(maxsize=None)
def donor(name):
    """The workspace a decode of (code ``name``, special, B = 512, max_iterations = 12) has just left,
    as a device copy: the donor of "leftover".  From the oracle alone, first: both ranges repack."""
    import torch

    case, dec = _decoder(name)
    ref = oracle_of(case, DONOR_MI)
    want = predict_repack(ref[0], ref[1], LD, DONOR_MI)
    assert min(want[0]) >= 1 and max(want[1]) < LD // 2, want
    L, S = to_device(case, LD, LD)
    with knobs(KNOBS, **TWO_STREAM):
        need = dec.workspace_bytes(LD, DONOR_MI)
        whole, view = W.guarded(need, W.guard_bytes(LD))
        W.fill(view, "zero")
        stats = W.decode_raw(dec, L, S, LD, DONOR_MI, whole, view, W.guard_bytes(LD), ref, ("donor", name))
    assert stats == want, (stats, want)
    torch.cuda.synchronize()
    return view.clone()


def donor_for(name):
    """Another case than the row's, at another max_iterations than any row's."""
    return donor("mix12_16_5" if name == "reg12" else "reg12")


def run_row(name, B, ld, mi, run, fills, D, path, expect_repack=False, base_only=False, untouched=False):
    """One row of the matrix under every fill of ``fills``: W.decode_raw's assertions, the repack
    stats (``expect_repack``: decode_fixture.predict_repack of the oracle's counts; else "never"),
    the path that ran.  base_only: the decode gets the base part of the workspace alone.
    untouched: everything but the RangeSel block is as filled afterwards."""
    import torch
    import test_gpu_resident_shapes as RS

    case, dec = _decoder(name)
    ref = oracle_of(case, mi)
    leftover = donor_for(name) if "leftover" in fills else None
    L, S = to_device(case, B, ld)
    guard = W.guard_bytes(ld)
    pct = {**KNOBS, **run}["repack_pct"]
    want = predict_repack(ref[0], ref[1], B, mi, pct) if expect_repack else never(ld)
    with knobs(KNOBS, **run):
        m = W.decode_ws_map(case["vid"], case["cid"], ld, mi, {**KNOBS, **run}["repack"])
        assert dec.workspace_bytes(ld, mi) == W.map_bytes(m), "tests/workspace_fixture.py decode_ws_map drifted"
        need = W.base_bytes(m) if base_only else W.map_bytes(m)
        for how in fills:
            tag = (name, B, ld, mi, run, how, "base only" if base_only else "")
            print(tag)
            whole, view = W.guarded(need, guard)
            W.fill(view, how, m, ld, leftover)
            before = view.clone() if untouched else None
            with profiled():
                stats = W.decode_raw(dec, L, S, B, mi, whole, view, guard, ref, tag)
                n = launches(D)
            assert stats == want, (tag, stats, want)
            if mi == 0:
                # no iteration: at most the first check sweep of range 0, which the two-stream
                # schedule issues ahead of its loop (its messages are never read)
                assert n["resident"] == n["iter"] == n["check"] == 0 and n["check1"] <= (run is TWO_STREAM), (tag, n)
            else:
                assert_path(path, mi, n, RS.iter_launches(mi, ld))
            if untouched:
                off = W.entry(m, "counts")[1]
                keep = torch.ones(need, dtype=torch.bool, device="cuda")
                keep[off + 16:off + 64] = False   # rsel = ints [4, 16) of the count block
                assert torch.equal(view[keep], before[keep]), f"{tag}: the decode wrote outside the RangeSel block"
    return want


# ------------------------------------------------------------------ the decode matrix
def test_a_frame_resident_touches_only_the_range_state(gpu):
    """B = 130 in ld = 192: one resident_d9 launch; of the workspace only the RangeSel block
    changes, and it reads "never repacked" over any fill."""
    run_row("resident", 130, 192, MI, {}, W.FILLS, 9, "resident", untouched=True)


def test_b_one_launch_per_iteration_second_message_buffer(gpu):
    """reg7, lock-step, resident off: the iter_d7 chain on c2v / c2v2, B = 450 in ld = 512."""
    case, _ = _decoder("reg7")
    assert "c2v2" in [e[0] for e in W.decode_ws_map(case["vid"], case["cid"], LD, MI, 1)]
    run_row("reg7", 450, LD, MI, dict(split=1, resident=0), W.FILLS, 7, "iter")


@pytest.mark.parametrize("compact, B", [(1, 450), (0, 512), (1, 512), (0, 450)])
def test_c_lock_step_with_and_without_lists(gpu, compact, B):
    """reg12 in lock-step (run_flat): alist and acount with knob compact on, neither with it off."""
    run_row("reg12", B, LD, MI, dict(split=1, compact=compact), W.FILLS, 12, "check")


@pytest.mark.parametrize("B", [512, 450, 257])
@pytest.mark.parametrize("name", ["reg12", "mix12_16_5"])
def test_d_two_stream_with_repack(gpu, name, B):
    """The two-stream schedule with the device-decided repack, max_iterations = 30: both column
    sets, fid, the transit and the narrow sweeps.  From the oracle alone, before any GPU call:
    range 0 of every (case, B) here is predicted to repack three times, 256 -> 192 or 128 -> .. ->
    64 columns (and range 1 as often at B = 512 and 450), so consecutive repacks write both column
    sets as destinations -- (reg12 special, B = 512) predicts ((3, 3), (64, 64)) at the default
    repack_pct = 80, no other B or threshold had to be looked for; assert_repack_counts holds
    at B = 512."""
    case, _ = _decoder(name)
    ref = oracle_of(case, MI)
    reps, widths = predict_repack(ref[0], ref[1], B, MI)
    assert max(reps) >= 2, (name, B, reps)
    if B == LD:
        assert assert_repack_counts(case, B, MI) == (reps, widths)
        assert min(reps) >= 2
    got = run_row(name, B, LD, MI, TWO_STREAM, W.FILLS, 12, "check", expect_repack=True)
    assert got == (reps, widths)


@pytest.mark.parametrize("B", [512, 450, 257])
@pytest.mark.parametrize("name", ["reg12", "mix12_16_5"])
def test_e_base_part_only_runs_without_the_repack(gpu, name, B):
    """Knob repack on, but the caller hands over the base part alone: "a workspace without the
    work set runs the same decode without the repack" -- the same results, stats "never", and
    the guard directly behind the base part intact."""
    run_row(name, B, LD, MI, TWO_STREAM, W.FILLS, 12, "check", base_only=True)


@pytest.mark.parametrize("B", [512, 450, 257])
@pytest.mark.parametrize("name", ["reg12", "mix12_16_5"])
def test_f_two_stream_repack_off(gpu, name, B):
    """Knob repack off: the size and the layout without the work set."""
    run_row(name, B, LD, MI, dict(TWO_STREAM, repack=0), W.FILLS, 12, "check")


@pytest.mark.parametrize("name, B, ld", [("himix", 450, 512), ("deg17", 1, 64), ("deg17", 64, 64)])
def test_g_runtime_degrees_f_scratch(gpu, name, B, ld):
    """The F scratch of the runtime-degree classes; ld = 64 is the only width at which the u8
    arrays (active, one unsat row) have slack behind them."""
    case, _ = _decoder(name)
    m = W.decode_ws_map(case["vid"], case["cid"], ld, MI, 1)
    assert "fb" in [e[0] for e in m] and (ld != 64 or W.entry(m, "active")[2] == 256 > ld)
    run_row(name, B, ld, MI, {}, W.FILLS, 17, "check")


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("mi", [0, 1])
def test_h_unsat_rows_at_zero_and_one_iterations(gpu, mi, split):
    """unsat has max_it + 2 rows: the last-row memset of max_iterations = 0, the single sweep of 1."""
    run = dict(split=1) if split == 1 else TWO_STREAM
    run_row("reg12", LD, LD, mi, run, W.FILLS, 12, "check", expect_repack=split == 3)


# ------------------------------------------------------------------ qr_decode_frames_device
def _run_frames(name, llr, synd, ref, mi, run, fills, few):
    from test_gpu_few_frames import _assert_few, _assert_frame_parallel, _counters

    case, dec = _decoder(name)
    B = llr.shape[0]
    ld = -(-B // 64) * 64
    guard = W.guard_bytes(ld)
    leftover = donor_for(name) if "leftover" in fills else None
    with knobs(KNOBS, **run):
        need = dec.frames_workspace_bytes(B, mi)
        for how in fills:
            tag = ("frames", name, B, mi, run, how)
            print(tag)
            whole, view = W.guarded(need, guard)
            W.fill(view, how, donor=leftover)
            with profiled():
                W.frames_raw(dec, llr, synd, mi, whole, view, guard, ref, tag)
                n = _counters()
            if few:
                _assert_few(n, mi, classes=len(few_fixture.MIXED_CLASSES))
            else:
                _assert_frame_parallel(n)


@pytest.mark.parametrize("B", [1, 16])
def test_i_frames_few_route(gpu, B):
    """The few-frame schedule on the caller's arrays, B = 1 and 16 (the five frames of
    few_fixture.mixed_case in turn: a frame's results do not depend on its neighbours).  Its layout
    cannot be cross-checked by size, so "zero" and "leftover" only."""
    case, _ = _decoder("few")
    few_fixture.assert_conditions(case["ref"], slice(0, 3))
    pick = np.arange(B) % case["llr"].shape[0]
    ref = tuple(a[pick] for a in case["ref"][few_fixture.MI])
    _run_frames("few", case["llr"][pick], case["synd"][pick], ref, few_fixture.MI, dict(few_max=16),
                ("zero", "leftover"), True)


@pytest.mark.parametrize("B", [17, 65])
def test_i_frames_transposed_route(gpu, B):
    """More frames than few_max: the stage arrays in front of the inner decode's workspace, ld = 64
    (B = 17) and 128 (B = 65)."""
    case, _ = _decoder("reg12")
    ref = tuple(a[:B] for a in oracle_of(case, MI))
    assert 0 < ref[0].sum() < B and np.isnan(case["llr"][:B]).any()
    _run_frames("reg12", case["llr"][:B], case["synd"][:B], ref, MI, dict(few_max=8), ("zero", "leftover"), False)


# ------------------------------------------------------------------ graph replay
def test_graph_replay_over_refilled_workspace(gpu):
    """Row d (reg12, B = 512) captured on a side stream, as test_repack_small_code_graph_replay does:
    the replay, the replay after a "typed" refill of the workspace and the replay after a "zero"
    refill all equal the oracle and repack as predicted."""
    import torch

    case, dec = _decoder("reg12")
    ref = oracle_of(case, MI)
    want = assert_repack_counts(case, LD, MI)
    L, S = to_device(case, LD, LD)
    guard = W.guard_bytes(LD)
    with knobs(KNOBS, **TWO_STREAM):
        m = W.decode_ws_map(case["vid"], case["cid"], LD, MI, 1)
        need = dec.workspace_bytes(LD, MI)
        assert need == W.map_bytes(m)
        whole, view = W.guarded(need, guard)
        W.fill(view, "zero")
        fin, succ, its = W.outputs(tuple(L.shape), LD)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            W.decode_call(dec, L, S, LD, MI, view, fin, succ, its)   # eager: the code's second stream exists
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            W.decode_call(dec, L, S, LD, MI, view, fin, succ, its)
        for how in (None, "typed", "zero"):
            if how:
                W.fill(view, how, m, LD)
            fin.fill_(PAD)
            succ.fill_(W.SENT_SUCC)
            its.fill_(W.SENT_ITERS)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            tag = ("replay", how)
            W.assert_guards(whole, guard, need, tag)
            W.assert_sentinels(succ, its, LD, tag)
            assert np.array_equal(succ[:LD].cpu().numpy(), ref[0]) and np.array_equal(its[:LD].cpu().numpy(), ref[1]), tag
            assert_bit_exact(fin.cpu().numpy().T, ref[2])
            W.assert_no_fill_payload(fin.cpu().numpy(), tag)
            assert W.repack_stats_raw(dec, LD, MI, view) == want, tag


# ------------------------------------------------------------------ alignment
def _assert_no_launch(names):
    from qamr import _lib

    n = {k: _lib.profile_query(k)[1] for k in names}
    assert not any(n.values()), n


def test_misaligned_workspace_is_refused_before_any_launch(gpu):
    """A base 128 bytes past a 256-byte boundary (every element still naturally aligned: no offset
    that is not a multiple of 16 is ever passed): ValueError from all four entries, every output
    still at its sentinel, the workspace as filled, no launch in the profile counters."""
    import torch
    from qamr import _lib
    from qamr._lib import dptr
    from qamr.mutual_information import P_xhat, _prepare
    from mapper_fixture import mapper, mc_inputs
    from test_gpu_lappr_info import frames, to_fi

    case, dec = _decoder("reg12")
    guard = W.guard_bytes(LD)
    lib = _lib.load()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    decode_names = DECODE_LAUNCH_NAMES + tuple(f"{k}_d12" for k in ("parity", "check1", "check", "iter", "resident"))

    def refused(need, call, names, outputs):
        whole, view = W.guarded(need + 128, guard)
        W.fill(view, "zero")
        off = view[128:]
        assert off.data_ptr() % 256 == 128 and off.numel() == need
        with profiled():
            with pytest.raises(ValueError, match="256-byte aligned"):
                _lib.check(call(off))
            torch.cuda.synchronize()
            _assert_no_launch(names)
        W.assert_guards(whole, guard, need + 128, "misaligned")
        assert not bool(view.any()), "the workspace was written"
        for t, v in outputs:
            assert bool((t == v).all()), "an output was written"

    # qr_decode_batch_device, lock-step and two-stream
    L, S = to_device(case, LD, LD)
    for run in (dict(split=1), TWO_STREAM):
        with knobs(KNOBS, **run):
            fin, succ, its = W.outputs(tuple(L.shape), LD)
            refused(dec.workspace_bytes(LD, MI),
                    lambda ws: lib.qr_decode_batch_device(dec.handle, LD, LD, dptr(L), dptr(S), MI, dptr(fin), dptr(succ),
                                                          dptr(its), dptr(ws), ws.numel(), sp),
                    decode_names, [(fin, PAD), (succ, W.SENT_SUCC), (its, W.SENT_ITERS)])
    # qr_decode_frames_device, the transposed route (its transposes come before the inner decode) and the few route
    fcase, fdec = _decoder("few")
    for d, llr, synd, few_max in ((dec, case["llr"][:17], case["synd"][:17], 8),
                                  (fdec, fcase["llr"][:1], fcase["synd"][:1], 8)):
        B = llr.shape[0]
        Lf, Sf = torch.from_numpy(np.array(llr)).cuda(), torch.from_numpy(np.array(synd)).cuda()
        with knobs(KNOBS, few_max=few_max):
            fin, succ, its = W.outputs((B, llr.shape[1]), B)
            refused(d.frames_workspace_bytes(B, MI),
                    lambda ws: lib.qr_decode_frames_device(d.handle, B, dptr(Lf), dptr(Sf), MI, dptr(fin), dptr(succ),
                                                           dptr(its), dptr(ws), ws.numel(), sp),
                    decode_names, [(fin, PAD), (succ, W.SENT_SUCC), (its, W.SENT_ITERS)])
    # qr_mi_montecarlo_device with the terms in the workspace
    fx = golden("mi.npz")
    pa, nm = mapper(fx, MI_CASE)
    _prepare(nm, P_xhat(nm))
    x, y = mc_inputs(fx, MI_CASE, 64, 3)
    info = torch.full((3, 64), PAD, dtype=torch.float64, device="cuda")
    need = C.c_size_t(0)
    _lib.check(lib.qr_mi_workspace_size(64, x.shape[0], C.byref(need)))
    refused(need.value,
            lambda ws: lib.qr_mi_montecarlo_device(nm.handle, 7, 3, 64, x.shape[0], dptr(x), dptr(y), dptr(info), None,
                                                   dptr(ws), ws.numel(), sp),
            ("mi_terms", "mi_sum"), [(info, PAD)])
    # qr_lappr_info_device
    Lh, wh = frames(2, 300, 3, 11)
    Lt, wt = to_fi(Lh, 64, float("nan")), to_fi(wh, 64, 255)
    al = np.array([1.0, 0.5])
    loss = torch.full((4, 64), PAD, dtype=torch.float64, device="cuda")
    errors = torch.full((2, 64), -7, dtype=torch.int32, device="cuda")
    total = torch.full((4,), PAD, dtype=torch.float64, device="cuda")
    terr = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.qr_lappr_info_workspace_size(2, 64, 300, 2, C.byref(need)))
    refused(need.value,
            lambda ws: lib.qr_lappr_info_device(2, 3, 64, 300, dptr(Lt), dptr(wt), 2, _lib.ptr(al), dptr(loss),
                                                dptr(errors), dptr(total), dptr(terr), dptr(ws), ws.numel(), sp),
            ("lappr_info", "lappr_info_total"), [(loss, PAD), (errors, -7), (total, PAD), (terr, -7)])


# ------------------------------------------------------------------ qr_mi_montecarlo_device
MI_CASE = "c3_"   # 4-PAM, sigma^2 = 0.501, of tests/golden/mi.npz


@pytest.mark.parametrize("B, ld", [(3, 64), (65, 128)])
def test_mi_montecarlo_workspace(gpu, B, ld):
    """The terms live in the workspace (d_terms = NULL), which is one f64 array [3][S][ld]: the
    totals equal the fixture's for the full mask and two subsets, a disabled quantity is 0.0 / S,
    and afterwards the workspace holds the enabled planes' terms in columns [0, B) and, everywhere
    else (disabled planes, padding columns), exactly what the fill put there."""
    import torch
    from qamr import _lib
    from qamr._lib import dptr
    from qamr.mutual_information import P_xhat, _prepare
    from mapper_fixture import expected_terms, mapper, mc_inputs

    fx = golden("mi.npz")
    assert int(fx[MI_CASE + "bps"]) == 2
    pa, nm = mapper(fx, MI_CASE)
    _prepare(nm, P_xhat(nm))
    x, y = mc_inputs(fx, MI_CASE, ld, B)
    Sq = x.shape[0]
    exp_t, exp_i = expected_terms(fx, MI_CASE, B), fx[MI_CASE + "totals"][:B].T
    lib = _lib.load()
    need = C.c_size_t(0)
    _lib.check(lib.qr_mi_workspace_size(ld, Sq, C.byref(need)))
    assert need.value == W.A256(3 * Sq * ld * 8)
    m = [("terms", 0, need.value, "f64")]
    guard = W.guard_bytes(ld)
    xc, yc = x.clone(), y.clone()
    last = donor("reg12")
    for mask in (7, 0b101, 0b010):
        for how in W.FILLS:
            tag = ("mi", B, ld, mask, how)
            whole, view = W.guarded(need.value, guard)
            W.fill(view, how, m, ld, last)
            before = view.clone()
            info = torch.full((3, ld), PAD, dtype=torch.float64, device="cuda")
            _lib.check(lib.qr_mi_montecarlo_device(nm.handle, mask, B, ld, Sq, dptr(x), dptr(y), dptr(info), None,
                                                   dptr(view), need.value,
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            W.assert_guards(whole, guard, need.value, tag)
            W.assert_inputs_intact([(x, xc), (y, yc)], tag)
            got = info.cpu().numpy()
            assert (got[:, B:] == PAD).all(), tag
            terms = view[:3 * Sq * ld * 8].view(torch.float64).reshape(3, Sq, ld)
            was = before[:3 * Sq * ld * 8].view(torch.int64).reshape(3, Sq, ld)
            for q in range(3):
                if (mask >> q) & 1:
                    assert_bit_exact(got[q, :B], exp_i[q])
                    assert_bit_exact(terms[q, :, :B].cpu().numpy(), exp_t[q])
                    assert torch.equal(terms[q, :, B:].view(torch.int64), was[q, :, B:]), (tag, q, "padding columns")
                else:
                    assert_bit_exact(got[q, :B], np.full(B, 0.0 / Sq))
                    assert torch.equal(terms[q].view(torch.int64), was[q]), (tag, q, "a disabled plane was written")
            W.assert_no_fill_payload(got, tag)
            last = view


# ------------------------------------------------------------------ qr_npstream_frames_device
@pytest.mark.parametrize("slack_pct", [0, None], ids=["mean_only", "default_slack"])
@pytest.mark.parametrize("S, B, ld", [(7, 200, 256), (504, 130, 192)])
def test_npstream_frames_workspace(gpu, S, B, ld, slack_pct):
    """Two shapes of tests/test_gpu_npstream.py on a guarded workspace of exactly the size asked for,
    "zero" and "leftover" (the prefix counts in it become ranks and store slots: no typed fill):
    numpy's symbols, samples and state, and seek_frame -- which reads the workspace -- still gives
    numpy's state.  np_slack_pct = 0 sizes the first range at the mean consumption, so about
    every other call tops up: over the seeds of test_frames_top_up at least one does (counter
    np_chain), and the extended range stays inside the size it was given."""
    import qamr
    from qamr import NumpyStream, _lib
    from test_gpu_npstream import A4, P_SHAPED, SIGMA, assert_state_is_numpys, host, host_frames

    need = C.c_size_t(0)
    _lib.check(_lib.load().qr_npstream_frames_workspace_size(S, B, C.byref(need)))
    guard = W.guard_bytes(ld)
    last = donor("reg12")
    topped = 0
    seeds = (31, 32, 33, 34, 35, 36) if slack_pct == 0 and S == 504 else (21,)
    for seed in seeds:
        for how in ("zero", "leftover"):
            tag = ("npstream", S, B, ld, slack_pct, seed, how)
            np.random.seed(seed)
            np.random.bytes(4 * 3)
            ns = NumpyStream()
            whole, view = W.guarded(need.value, guard)
            W.fill(view, how, donor=last)
            ns._ws = view   # NumpyStream.frames takes a workspace it already holds when it is large enough
            with knobs(**({} if slack_pct is None else dict(np_slack_pct=slack_pct))), profiled():
                x, y, fw = ns.frames(P_SHAPED, A4, SIGMA, S, B, ld=ld)
                n_chain = qamr.profile_query("np_chain")[1]
            assert ns._ws is view
            W.assert_guards(whole, guard, need.value, tag)
            xr, yr, states = host_frames(P_SHAPED, S, B)
            end = np.random.get_state()
            assert np.array_equal(host(x)[:, :B].T, xr), tag
            assert_bit_exact(host(y)[:, :B].T, yr)
            assert not host(x)[:, B:].any() and not host(y)[:, B:].view(np.int64).any(), tag
            assert_state_is_numpys(ns)
            for w in (B // 2, B - 1, 0):
                ns.seek_frame(w)
                np.random.set_state(states[w])
                assert_state_is_numpys(ns)
            np.random.set_state(end)
            W.assert_guards(whole, guard, need.value, tag)
            assert 1 <= n_chain <= 9, tag
            topped += n_chain >= 2
            last = view
        if topped:
            break
    if len(seeds) > 1:
        # about every other call needs more than the mean range: six seeds that all fit have probability 2^-6
        assert topped >= 1


# ------------------------------------------------------------------ qr_lappr_info_device
@pytest.mark.parametrize("S, bps, B, A", [(257, 8, 65, 3), (513, 2, 3, 16)])
def test_lappr_info_workspace_fills(gpu, S, bps, B, A):
    """run_raw of tests/test_gpu_lappr_info.py (guards on both sides; its own cases run "typed") under
    "zero" and "leftover", the donor the typed run's workspace of the other shape's size."""
    import lappr_info_fixture as F
    from test_gpu_lappr_info import check_against, frames, run_raw

    L, w = frames(bps, S, B, 7000 + S + 10 * bps + B)
    alphas = F.SCALES[:A]
    ld = -(-B // 64) * 64
    ref = F.evaluate(L, w, bps, alphas)
    last = donor("reg12")
    for how in ("zero", "typed", "leftover"):
        check_against(ref, run_raw(L, w, bps, alphas, ld, fill=how, donor=last), A, bps, B, ld)
        last = run_raw.last_view


# ------------------------------------------------------------------ debug build
CONTRACT = ["test_a_frame_resident_touches_only_the_range_state", "test_b_one_launch_per_iteration_second_message_buffer",
            "test_c_lock_step_with_and_without_lists", "test_d_two_stream_with_repack",
            "test_e_base_part_only_runs_without_the_repack", "test_f_two_stream_repack_off",
            "test_g_runtime_degrees_f_scratch", "test_h_unsat_rows_at_zero_and_one_iterations", "test_i_frames_few_route",
            "test_i_frames_transposed_route", "test_graph_replay_over_refilled_workspace",
            "test_misaligned_workspace_is_refused_before_any_launch", "test_mi_montecarlo_workspace",
            "test_npstream_frames_workspace", "test_lappr_info_workspace_fills"]


def test_debug_build_index_checks_over_the_fills(gpu):
    """Every test above in a child process on libqamr_debug.so: a stale read of a list entry, a frame id or
    a count that the typed fill keeps in range can still give the right result by luck; the QR_DCHECK index
    checks (ascending list entries inside the range, frame ids, row-group slots, prefix counts) then count
    it -- conftest's autouse fixture fails any test after which one did."""
    from debug_rerun import rerun_on_debug_build

    rerun_on_debug_build([f"tests/test_gpu_workspace_contract.py::{t}" for t in CONTRACT], 45, timeout=600)
