"""GPU tests of the layered (serial-check) decode schedule (csrc/decode_layered.hip) against its
definition restated in Python (tests/layered_fixture.py): success, iterations and final LAPPRs are
bit-exact, the padding columns of the output keep the caller's values.  The conditions on the
inputs are asserted from the restatement first."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_bit_exact, golden

import decode_fixture as DF
import few_fixture as FF
import layered_fixture as LF
import workspace_fixture as W

pytestmark = pytest.mark.gpu

PAD = DF.PAD
SHAPES = [(64, 64), (37, 128), (65, 128)]   # B = 37: a wave that is all padding; 65: a wave with one live frame


def _decoder(case):
    import qamr

    return qamr.Decoder(case["vid"], case["cid"])


def _frames(case, B):
    """Frame indices of a B-frame batch: the case's frames, repeated from the first when B is larger."""
    return np.arange(B) % case["llr"].shape[0]


def _upload(case, B, ld):
    import torch

    idx = _frames(case, B)
    V, Cn = case["orc"].vnum, case["orc"].cnum
    L = torch.zeros((V, ld), dtype=torch.float64, device="cuda")
    L[:, :B] = torch.from_numpy(case["llr"][idx].T.copy()).cuda()
    S = torch.zeros((Cn, ld), dtype=torch.uint8, device="cuda")
    S[:, :B] = torch.from_numpy(case["synd"][idx].T.copy()).cuda()
    return L, S


def _compare(case, B, mi, fin, succ, its, tag):
    """The device's outputs of the first B frames equal the restatement's; the padding keeps PAD."""
    s2, i2, f2 = (a[_frames(case, B)] for a in LF.layered_of(case, mi))
    print(tag, "successes", int(s2.sum()), "iterations", sorted(set(i2.tolist())))
    assert np.array_equal(succ[:B].cpu().numpy(), s2), tag
    assert np.array_equal(its[:B].cpu().numpy(), i2), tag
    assert_bit_exact(fin[:, :B].cpu().numpy().T, f2)
    assert bool((fin[:, B:] == PAD).all()), tag


def _decode_and_compare(dec, case, B, ld, mi, tag):
    import torch

    L, S = _upload(case, B, ld)
    fin = torch.full(tuple(L.shape), PAD, dtype=torch.float64, device="cuda")
    out, succ, its = dec.decode_layered_device(L, S, B, mi, final_fi=fin)
    torch.cuda.synchronize()
    assert out is fin and succ.numel() == B and its.numel() == B
    _compare(case, B, mi, fin, succ, its, tag)


# ------------------------------------------------------------------ 1, 2: the N = 1008 code
@pytest.mark.parametrize("B, ld", SHAPES)
@pytest.mark.parametrize("mi", LF.MIS)
def test_main_case_vs_definition(gpu, mi, B, ld):
    case = LF.main_case()
    LF.assert_main_conditions(case)
    _decode_and_compare(_decoder(case), case, B, ld, mi, ("main", mi, B, ld))


@pytest.mark.parametrize("mi", LF.MIS)
def test_special_frames_vs_definition(gpu, mi):
    """Exact codewords stop at (1, 0) with a plain copy; inf, -inf, -0.0, 0.0 and NaN travel as in
    the definition."""
    case = LF.special_case()
    LF.assert_special_conditions(case)
    _decode_and_compare(_decoder(case), case, 16, 64, mi, ("special", mi))


# ------------------------------------------------------------------ 3: every check degree
@pytest.mark.parametrize("D", range(2, 17))
def test_degree_matrix_vs_definition(gpu, D):
    case = LF.degree_case(D)
    dec = _decoder(case)
    with DF.profiled():
        for mi in LF.DEGREE_MIS:
            _decode_and_compare(dec, case, 8, 64, mi, ("degree", D, mi))
        from qamr import _lib

        n_all, n_d = _lib.profile_query("layer_check")[1], _lib.profile_query(f"layer_check_d{D}")[1]
    layers = LF.graph_of(case["vid"], case["cid"])["n_layers"]
    assert n_all == n_d == layers * sum(LF.DEGREE_MIS), (n_all, n_d, layers)   # one launch per layer and iteration


# ------------------------------------------------------------------ 4: mixed classes
def test_mixed_classes_vs_definition(gpu):
    """few_fixture.mixed_code(): seven classes, one of a single check, a hub of degree 70 (dozens of
    tiny layers), isolated variables, parallel edges."""
    case = LF.mixed_case()
    LF.assert_mixed_conditions(case, 24)
    G = LF.graph_of(case["vid"], case["cid"])
    assert G["repeat"].any() and len(set(np.bincount(case["cid"]).tolist())) == 7
    _decode_and_compare(_decoder(case), case, 16, 64, LF.MI, "mixed")


def test_mix12_16_5_vs_definition(gpu):
    """decode_fixture.small_code("mix12_16_5"): a packed class (5) and two unpacked ones (12, 16)."""
    case = LF.mix12_case()
    LF.assert_mixed_conditions(case, 2)
    assert set(np.bincount(case["cid"]).tolist()) == {5, 12, 16}
    _decode_and_compare(_decoder(case), case, 16, 64, LF.MI, "mix12_16_5")


# ------------------------------------------------------------------ 5: Hamming(7,4)
def test_hamming_reference_vectors(gpu):
    """The reference's two vectors (test_decoder.py:237-266): the codeword stops at (1, 0) unchanged;
    the one-bit-error word decodes to the reference's hard decision; both equal the restatement."""
    import oracle as O
    import qamr
    from qamr import codes

    vid, cid = codes.load_edge_csv(os.path.join(GOLDEN, "hamming_7-4.csv"))
    g = golden("hamming.npz")
    dec, orc, G = qamr.Decoder(vid, cid), O.OracleCode(vid, cid), LF.graph_of(vid, cid)
    ok, it, r = dec.decode_layered(g["correct_lappr"], g["correct_synd"], 20)
    assert ok == 1 and it == 0
    assert_bit_exact(r, g["correct_lappr"])
    for mi in (0, 1, 2, 20):
        (s2, i2, f2), _ = LF.layered_decode(orc, G, g["one_bit_lappr"], g["one_bit_synd"], mi)
        ok, it, r = dec.decode_layered(g["one_bit_lappr"], g["one_bit_synd"], mi)
        assert (ok, it) == (s2, i2), mi
        assert_bit_exact(r, f2)
    assert ok == 1 and np.array_equal((np.asarray(r) < 0).astype(int), [0, 1, 1, 0, 1, 0, 0])


# ------------------------------------------------------------------ 6: the layers
def _codes():
    from qamr import codes

    yield "reg1008", codes.regular_code(1008, 3, 6, 0), LF.REG1008_LAYER_SIZES
    yield "dvbs2", codes.dvbs2_like_half(), LF.DVBS2_LAYER_SIZES
    yield "mixed", FF.mixed_code(), None
    yield "mix12_16_5", DF.small_code("mix12_16_5"), None
    yield "hamming", codes.load_edge_csv(os.path.join(GOLDEN, "hamming_7-4.csv")), None
    for D in range(2, 17):
        yield f"deg{D}", codes.regular_code(DF.v_of(D), 3, D, seed=100 + D), None


def test_layers_equal_python_first_fit(gpu):
    import qamr

    for name, (vid, cid), sizes in _codes():
        layer_of, n = qamr.Decoder(vid, cid).layers()
        ref, n_ref = LF.first_fit(vid, cid)
        assert layer_of.dtype == np.int32 and n == n_ref and np.array_equal(layer_of, ref), name
        if sizes is not None:
            assert LF.layer_sizes(layer_of, n) == sizes, name


# ------------------------------------------------------------------ 7: refusals
def _raw(dec, L, S, B, ld, mi, view, fin, succ, its, nbytes=None):
    """qr_decode_layered_device on the caller's workspace view: the status code."""
    from qamr import _lib
    from qamr._lib import dptr

    return _lib.load().qr_decode_layered_device(dec.handle, int(B), int(ld), dptr(L), dptr(S), int(mi), dptr(fin),
                                                dptr(succ), dptr(its), dptr(view),
                                                view.numel() if nbytes is None else nbytes, W._stream_ptr())


def _launch_names(D):
    return ("layer_check", f"layer_check_d{D}", "layer_parity", "status", "var_init", "parity", f"parity_d{D}")


def test_refusals_before_any_launch(gpu):
    import qamr
    import torch
    from qamr import _lib

    case = LF.main_case()
    dec = _decoder(case)
    L, S = _upload(case, 64, 128)
    need = dec.layered_workspace_bytes(128, 5)
    raw = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    view = raw[-raw.data_ptr() % 256:][:need]
    # a code with one degree-17 check (check 0), checks 1..8 of degree 2
    vid17 = np.concatenate([np.arange(17), np.arange(16)]).astype(np.int64)
    cid17 = np.concatenate([np.zeros(17), 1 + np.arange(16) // 2]).astype(np.int64)
    dec17 = qamr.Decoder(vid17, cid17)
    assert dec17.max_check_degree == 17
    L17 = torch.zeros((17, 64), dtype=torch.float64, device="cuda")
    S17 = torch.zeros((9, 64), dtype=torch.uint8, device="cuda")
    with DF.profiled():
        def refused(rc, want, fin, succ, its):
            torch.cuda.synchronize()
            assert rc == want, (rc, _lib.last_error())
            assert bool((fin == PAD).all()) and bool((succ == W.SENT_SUCC).all()) and bool((its == W.SENT_ITERS).all())

        fin, succ, its = W.outputs((17, 64), 4)
        ws17 = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
        refused(_raw(dec17, L17, S17, 4, 64, 5, ws17, fin, succ, its), _lib.QR_EUNSUPPORTED, fin, succ, its)
        with pytest.raises(_lib.QamrError):
            dec17.decode_layered_device(L17, S17, 4, 5)
        with pytest.raises(_lib.QamrError):
            dec17.decode_layered(np.zeros(17), np.zeros(9, np.uint8), 5)
        layer_of, n = dec17.layers()   # the layers exist for any code
        assert n == 2 and layer_of[0] == 0
        fin, succ, its = W.outputs(tuple(L.shape), 64)
        refused(_raw(dec, L, S, 64, 128, 5, view, fin, succ, its, nbytes=need - 1), _lib.QR_EVALUE, fin, succ, its)
        refused(_raw(dec, L, S, 64, 128, 5, raw[(-raw.data_ptr() % 256) + 128:][:need], fin, succ, its), _lib.QR_EVALUE,
                fin, succ, its)
        refused(_raw(dec, L, S, 129, 128, 5, view, fin, succ, its), _lib.QR_EVALUE, fin, succ, its)    # B > ld
        refused(_raw(dec, L, S, 0, 128, 5, view, fin, succ, its), _lib.QR_EVALUE, fin, succ, its)
        refused(_raw(dec, L, S, 64, 96, 5, view, fin, succ, its), _lib.QR_EVALUE, fin, succ, its)      # ld % 64
        refused(_raw(dec, L, S, 64, 128, -1, view, fin, succ, its), _lib.QR_EVALUE, fin, succ, its)    # max_iterations
        for name in _launch_names(6) + _launch_names(17):
            assert _lib.profile_query(name)[1] == 0, name
    with pytest.raises(ValueError):
        dec.layered_workspace_bytes(128, -1)
    with pytest.raises(ValueError):
        dec.layered_workspace_bytes(96, 5)
    with pytest.raises(ValueError):
        dec.decode_layered_device(L, S, 64, -1)
    with pytest.raises(ValueError):
        dec.decode_layered_batch(case["llr"][:3], case["synd"][:3], -1)


# ------------------------------------------------------------------ 8: asynchronous, capturable
def test_asynchronous_and_graph_capture(gpu):
    """The call returns while the stream is still busy with the work queued before it, and a
    torch.cuda.graph capture of it, replayed on refilled inputs, gives the eager results."""
    import torch

    case = LF.main_case()
    dec = _decoder(case)
    B, ld, mi = 37, 128, LF.MI
    L, S = _upload(case, B, ld)
    fin = torch.full(tuple(L.shape), PAD, dtype=torch.float64, device="cuda")
    succ = torch.zeros(B, dtype=torch.uint8, device="cuda")
    its = torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dec.decode_layered_device(L, S, B, mi, fin, succ, its)   # eager: allocates this stream's workspace
    torch.cuda.synchronize()
    _compare(case, B, mi, fin, succ, its, "eager")
    with torch.cuda.stream(s):
        torch.cuda._sleep(100_000_000)    # the GPU spins for tens of milliseconds ahead of the decode
        dec.decode_layered_device(L, S, B, mi, fin, succ, its)
        end = torch.cuda.Event()
        end.record(s)
        pending = not end.query()
    torch.cuda.synchronize()
    assert pending, "decode_layered_device waited for the GPU"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        dec.decode_layered_device(L, S, B, mi, fin, succ, its)
    # other frames in the same buffers: frames 20.. of the case
    idx = 20 + np.arange(B)
    L[:, :B] = torch.from_numpy(case["llr"][idx].T.copy()).cuda()
    S[:, :B] = torch.from_numpy(case["synd"][idx].T.copy()).cuda()
    fin.fill_(PAD)
    succ.fill_(9)
    its.fill_(-5)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    s2, i2, f2 = (a[idx] for a in LF.layered_of(case, mi))
    assert len(set(i2.tolist())) >= 4 and 0 < s2.sum() < B
    assert np.array_equal(succ.cpu().numpy(), s2) and np.array_equal(its.cpu().numpy(), i2)
    assert_bit_exact(fin[:, :B].cpu().numpy().T, f2)
    assert bool((fin[:, B:] == PAD).all())


# ------------------------------------------------------------------ 9: host arrays
def test_host_entries_equal_the_device_entry(gpu):
    import torch

    case = LF.main_case()
    dec = _decoder(case)
    L, S = _upload(case, 3, 64)
    fin, succ, its = dec.decode_layered_device(L, S, 3, LF.MI)
    torch.cuda.synchronize()
    s1, i1, f1 = dec.decode_layered_batch(case["llr"][:3], case["synd"][:3], LF.MI)
    assert s1.dtype == np.uint8 and i1.dtype == np.int32 and f1.shape == (3, case["orc"].vnum)
    assert np.array_equal(s1, succ.cpu().numpy()) and np.array_equal(i1, its.cpu().numpy())
    assert_bit_exact(f1, fin[:, :3].cpu().numpy().T)
    ok, it, r = dec.decode_layered(case["llr"][1], case["synd"][1], LF.MI)
    assert isinstance(ok, int) and isinstance(it, int) and (ok, it) == (int(s1[1]), int(i1[1]))
    assert_bit_exact(r, f1[1])
    s2, i2, f2 = LF.layered_of(case, LF.MI)
    assert np.array_equal(s1, s2[:3]) and np.array_equal(i1, i2[:3])
    assert_bit_exact(f1, f2[:3])
    with pytest.raises(ValueError):
        dec.decode_layered(case["llr"][1][:-1], case["synd"][1], LF.MI)


# ------------------------------------------------------------------ 10: the schedule keyword
def test_pipeline_schedule_layered(gpu):
    """SofteningPipeline(schedule="layered") on the N = 1008 code, 4-PAM, one 64-frame batch: its
    decode outputs equal decode_layered_device on the same LAPPRs (and the restatement on the first
    four frames), its counters follow from them; the flooding default is unchanged."""
    import oracle as O
    import torch
    from qamr import _lib, codes
    from qamr.pipeline import SofteningPipeline, count_errors_device

    vid, cid = codes.regular_code(1008, 3, 6, 0)
    import qamr

    dec = qamr.Decoder(vid, cid)
    B, mi = 64, 30
    pipe = SofteningPipeline(dec, bps=2, snr_db=4.0, batch=B, max_iterations=mi, schedule="layered")
    assert pipe.schedule == "layered"
    with DF.profiled():
        b, lappr, fin, succ, its = pipe.run_batch(torch.Generator(device="cuda").manual_seed(77))
        torch.cuda.synchronize()
        assert _lib.profile_query("layer_check")[1] > 0 and _lib.profile_query("check1_d6")[1] == 0
    fin = fin.clone()   # the decoder's next call reuses nothing of it, but keep the pipeline's result apart
    f2, s2, i2 = dec.decode_layered_device(lappr, b.synd, B, mi)
    torch.cuda.synchronize()
    assert torch.equal(succ, s2) and torch.equal(its, i2)
    assert torch.equal(fin[:, :B].view(torch.int64), f2[:, :B].view(torch.int64))
    sn, itn = succ.cpu().numpy(), its.cpu().numpy()
    print("pipeline: successes", int(sn.sum()), "iterations", sorted(set(itn.tolist())))
    assert 0 < sn.sum() < B, (sn, itn)   # 4.0 dB: the code's waterfall, some frames converge and some do not
    orc, G = O.OracleCode(vid, cid), LF.graph_of(vid, cid)
    Lh, Sh = lappr[:, :4].cpu().numpy().T.copy(), b.synd[:, :4].cpu().numpy().T.copy()
    for f in range(4):
        (s3, i3, f3), _ = LF.layered_decode(orc, G, Lh[f], Sh[f], mi)
        assert (int(sn[f]), int(itn[f])) == (s3, i3)
        assert_bit_exact(fin[:, f].cpu().numpy(), f3)
    want = torch.zeros(5, dtype=torch.int64, device="cuda")
    ferr = torch.empty(B, dtype=torch.int32, device="cuda")
    count_errors_device(False, B, pipe.ld, pipe.K, f2, b.word, s2, i2, ferr, want)
    torch.cuda.synchronize()
    got = pipe.counters.cpu().numpy()
    assert np.array_equal(got, want.cpu().numpy())
    assert got[2] == int(sn.sum()) and got[3] == int(itn[sn != 0].sum()) and got[4] == B
    with pytest.raises(ValueError):
        SofteningPipeline(dec, bps=2, snr_db=3.0, batch=B, schedule="bogus")
    assert SofteningPipeline(dec, bps=2, snr_db=3.0, batch=B).schedule == "flooding"


def test_simulators_schedule_layered(gpu):
    """Simulator and BinaryChannelSimulator with schedule="layered": one batch's (success,
    iterations) equal decode_layered_device on the inputs the hook saw; "bogus" is ValueError in
    every constructor and function that takes the keyword."""
    import qamr
    import torch
    from qamr import codes, sim
    from qamr.noisemapper import NoiseMapper
    from qamr.pipeline import noise_variance
    from qamr.sim_binary import BinaryChannelSimulator

    vid, cid = codes.regular_code(1008, 3, 6, 0)
    dec = qamr.Decoder(vid, cid)
    seen = {}

    def hook(l, s, w, b):
        seen["in"] = (l.clone(), s.clone(), b)

    def same(succ, its, mi):
        l, s, b = seen["in"]
        _, s2, i2 = dec.decode_layered_device(l, s, b, mi)
        torch.cuda.synchronize()
        assert torch.equal(succ, s2[:b]) and torch.equal(its, i2[:b])
        assert 0 < int(s2.sum())

    S1 = sim.Simulator(dec, 2, "softening", 30, 1.0, 64, schedule="layered")
    nm = NoiseMapper(S1.pa, noise_variance(S1.pa, 3.0), S1.cfg, device=0)
    gen = torch.Generator(device="cuda").manual_seed(5)
    _, succ, its, delta = S1.batch_results(nm, 64, gen, S1.pa.variance * 10 ** -0.3, hook)
    same(succ, its, 30)
    S2 = BinaryChannelSimulator(dec, "biawgn", 30, 1.0, 64, schedule="layered")
    _, succ, its, delta = S2.batch_results(2.0, 64, torch.Generator(device="cuda").manual_seed(6), hook)
    same(succ, its, 30)
    for make in (lambda: sim.Simulator(dec, 2, schedule="bogus"),
                 lambda: BinaryChannelSimulator(dec, "bsc", schedule="bogus"),
                 lambda: sim.simulate_softening_snr_dB(3.0, dec, 2, S1.cfg, 5, 4, 1, schedule="bogus"),
                 lambda: sim.simulate_direct_snr_dB(3.0, dec, 2, 5, 4, 1, schedule="bogus"),
                 lambda: sim.simulate_hard_reverse_snr_dB(3.0, dec, 2, 5, 4, 1, schedule="bogus")):
        with pytest.raises(ValueError):
            make()
    row = sim.simulate_direct_snr_dB(6.0, dec, 2, 10, 8, 1, batch=8, schedule="layered")
    assert row[0] == 6.0 and 0.0 <= row[2] <= 1.0


def test_cli_schedule_flag_round_trips():
    from qamr import sim_bsc, sim_decode, sim_direct, sim_reconciliation

    for mod in (sim_reconciliation, sim_decode, sim_direct, sim_bsc):
        p = mod.build_parser()
        assert p.parse_args(["edges.csv"]).schedule == "flooding"
        assert p.parse_args(["edges.csv", "--schedule", "layered"]).schedule == "layered"
        with pytest.raises(SystemExit):
            p.parse_args(["edges.csv", "--schedule", "bogus"])


# ------------------------------------------------------------------ 11: the workspace contract
@pytest.mark.parametrize("which, B, ld", [("main", 37, 128), ("special", 16, 64)])
def test_workspace_contract(gpu, which, B, ld):
    """Guards on both sides of a workspace of exactly the size asked for, filled on entry with NaNs
    of a known payload: the results are the restatement's, no output carries the payload, the
    guards, the inputs and the entries of success / iters past B are intact."""
    import torch

    case = LF.main_case() if which == "main" else LF.special_case()
    dec = _decoder(case)
    mi = LF.MI
    need = dec.layered_workspace_bytes(ld, mi)
    E = case["vid"].size
    assert need % 256 == 0 and need >= 8 * E * ld + ld + (mi + 2) * ld + 256
    guard = W.guard_bytes(ld)
    whole, view = W.guarded(need, guard)
    assert W.NAN_BITS < 1 << 63
    view.view(torch.int64)[:] = W.NAN_BITS
    L, S = _upload(case, B, ld)
    Lc, Sc = L.clone(), S.clone()
    fin, succ, its = W.outputs(tuple(L.shape), B)
    rc = _raw(dec, L, S, B, ld, mi, view, fin, succ, its)
    torch.cuda.synchronize()
    assert rc == 0
    W.assert_guards(whole, guard, need, which)
    W.assert_inputs_intact([(L, Lc), (S, Sc)], which)
    W.assert_sentinels(succ, its, B, which)
    _compare(case, B, mi, fin, succ, its, which)
    W.assert_no_fill_payload(fin.cpu().numpy(), which)
