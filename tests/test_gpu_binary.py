"""GPU tests of the binary-channel code evaluation: the two LLR kernels and the `final < 0` count
of csrc/binary_channel.hip against the reference's stored values, the chain LLR -> syndrome ->
decode -> count on the fixture's inputs, BinaryChannelSimulator.run_point against the oracle and
the sequential loop, and the three CLIs.  All on the N = 1008 regular code, B <= 96."""
import ctypes as C

import numpy as np
import pytest

from binary_fixture import FRAMES, K, MAXITER, N, cases, fixture, result_tuple, sequential
from conftest import assert_bit_exact

import oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = -12345.6789
SHAPES = [(16, 64, 0), (70, 128, 54)]      # (B, ld, first column of the fixture's frames)


def vp(t):
    return C.c_void_p(t.data_ptr())


def plane(rows, B, ld, col0, dtype, pad):
    """Frame-innermost [V][ld] device tensor: column j < B holds rows[(j - col0) % len(rows)], so
    the frames sit at columns col0 .. col0 + len(rows) - 1; columns >= B hold `pad`."""
    import torch

    rows = np.asarray(rows)
    host = np.full((rows.shape[1], ld), pad, dtype=rows.dtype)
    for j in range(B):
        host[:, j] = rows[(j - col0) % rows.shape[0]]
    return torch.from_numpy(host).to(device="cuda", dtype=dtype)


def launch_llr(channel, coef, vsqrt_or_r, B, ld, word, noise, out, rx=None):
    from qamr import _lib

    L = _lib.load()
    V = word.shape[0]
    if channel == "bsc":
        _lib.check(L.qr_bsc_llr_device(coef, vsqrt_or_r, B, ld, V, vp(word), vp(noise), vp(out),
                                       None if rx is None else vp(rx), None))
    else:
        _lib.check(L.qr_biawgn_llr_device(int(channel == "biawgn_hard"), coef, vsqrt_or_r, B, ld, V, vp(word),
                                          vp(noise), vp(out), None))


def run_llr(channel, coef, vsqrt_or_r, rows_w, rows_n, B, ld, col0, with_rx=False):
    """The kernel on a plane built from per-frame rows; returns (llr [ld][V], rx or None) on the
    host after checking that the padding columns kept their sentinel."""
    import torch

    word = plane(rows_w, B, ld, col0, torch.uint8, 0)
    noise = plane(rows_n, B, ld, col0, torch.float64, np.nan)
    out = torch.full((word.shape[0], ld), SENTINEL, dtype=torch.float64, device="cuda")
    rx = torch.full((word.shape[0], ld), 7, dtype=torch.uint8, device="cuda") if with_rx else None
    launch_llr(channel, coef, vsqrt_or_r, B, ld, word, noise, out, rx)
    torch.cuda.synchronize()
    got = out.cpu().numpy().T
    assert np.all(got[B:] == SENTINEL), "padding columns were written"
    if rx is not None:
        rx = rx.cpu().numpy().T
        assert np.all(rx[B:] == 7)
    return got, rx


@pytest.mark.parametrize("B,ld,col0", SHAPES)
@pytest.mark.parametrize("c", range(7))
def test_llr_kernels_bit_exact_on_the_fixture(gpu, c, B, ld, col0):
    case = cases()[c]
    second = case.point if case.channel == "bsc" else case.vsqrt
    got, rx = run_llr(case.channel, case.coef, second, case.word, case.noise, B, ld, col0, case.channel == "bsc")
    assert_bit_exact(got[col0:col0 + 4], case.llr)                  # the reference's stored values
    ref = case.numpy_llr()                                          # all 16 frames, numpy's form
    for j in range(B):
        assert_bit_exact(got[j], ref[(j - col0) % FRAMES])
    if rx is not None:
        for j in range(B):
            f = (j - col0) % FRAMES
            assert np.array_equal(rx[j], case.word[f] ^ (case.noise[f] < case.point))


@pytest.mark.parametrize("B,ld,col0", SHAPES)
def test_llr_kernels_bit_exact_on_the_edge_planes(gpu, B, ld, col0):
    g = fixture()
    z, w = g["edge_z"], g["edge_w"]
    n = z.size
    # frame f = the list rotated by f: every element meets every lane of the first columns
    rows_w = np.array([np.roll(w, f) for f in range(n)])
    rows_z = np.array([np.roll(z, f) for f in range(n)])
    for p in range(2):
        for h, channel in enumerate(("biawgn", "biawgn_hard")):
            got, _ = run_llr(channel, float(g["edge_coef"][p, h]), float(g["edge_vsqrt"][p]), rows_w, rows_z, B, ld, col0)
            for j in range(B):
                assert_bit_exact(got[j], np.roll(g["edge_llr"][p, h], (j - col0) % n))
    assert np.isnan(g["edge_llr"][1, 1][~np.isnan(z)]).any()        # inf * 0 was among them
    u, bw, r = g["bsc_edge_u"], g["bsc_edge_w"], float(g["bsc_edge_r"])
    m = u.size
    rows_w = np.array([np.roll(bw, f) for f in range(m)])
    rows_u = np.array([np.roll(u, f) for f in range(m)])
    got, rx = run_llr("bsc", float(g["bsc_edge_coef"]), r, rows_w, rows_u, B, ld, col0, True)
    for j in range(B):
        assert_bit_exact(got[j], np.roll(g["bsc_edge_llr"], (j - col0) % m))
        assert np.array_equal(rx[j], np.roll(g["bsc_edge_rx"], (j - col0) % m))


def test_count_errors_neg_on_a_handcrafted_plane(gpu):
    """NaN, +-0.0 and +-inf among the finals: the new entry counts ((final < 0) ^ word), the existing
    one still counts with `>= 0 decides 0` (a NaN decides 1 there)."""
    import torch
    from qamr import _lib

    L = _lib.load()
    B, ld = 70, 128
    rng = np.random.default_rng(77)
    fin = rng.standard_normal((N, ld))
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf])
    mask = rng.random((N, ld)) < 0.2
    fin[mask] = special[rng.integers(0, special.size, int(mask.sum()))]
    fin[:5, 3] = special                 # every special value against both word bits, inside K = V - C
    fin[5:10, 3] = special
    word = rng.integers(0, 2, (N, ld)).astype(np.uint8)
    word[:5, 3], word[5:10, 3] = 0, 1
    succ = rng.integers(0, 2, B).astype(np.uint8)
    its = rng.integers(1, 31, B).astype(np.int32)
    d_fin, d_word = torch.from_numpy(fin).cuda(), torch.from_numpy(word).cuda()
    d_succ, d_its = torch.from_numpy(succ).cuda(), torch.from_numpy(its).cuda()
    rules = {"qr_count_errors_neg_device": (fin < 0), "qr_count_errors_device": ~(fin >= 0)}
    assert not np.array_equal(rules["qr_count_errors_neg_device"], rules["qr_count_errors_device"])
    for name, ones in rules.items():
        for Kk in (N, N - 504):
            exp = (ones.astype(np.uint8) ^ word)[:Kk, :B].sum(0)
            ferr = torch.full((ld,), -1, dtype=torch.int32, device="cuda")
            cnt = torch.tensor([1, 2, 3, 4, 5], dtype=torch.int64, device="cuda")      # accumulated into
            _lib.check(getattr(L, name)(B, ld, Kk, vp(d_fin), vp(d_word), vp(d_succ), vp(d_its), vp(ferr), vp(cnt),
                                        None))
            torch.cuda.synchronize()
            got = ferr.cpu().numpy()
            assert np.array_equal(got[:B], exp), (name, Kk)
            assert np.all(got[B:] == -1)
            s64 = succ.astype(np.int64)
            assert cnt.cpu().numpy().tolist() == [1 + int(exp.sum()), 2 + int((exp > 0).sum()), 3 + int(s64.sum()),
                                                  4 + int((its * s64).sum()), 5 + B], (name, Kk)


@pytest.fixture(scope="module")
def code():
    import qamr
    from qamr import codes

    vid, cid = codes.regular_code(N)
    return qamr.Decoder(vid, cid), O.OracleCode(vid, cid)


@pytest.mark.parametrize("c", range(7))
def test_end_to_end_from_the_fixture_inputs(gpu, code, c):
    """LLR kernel -> qr_syndrome_device -> decode_device -> qr_count_errors_neg_device on the stored
    words and noise: the reference's per-frame results for all 16 frames, its finals for the first 4."""
    import torch
    from qamr import _lib

    dec, _ = code
    case = cases()[c]
    L = _lib.load()
    B, ld = FRAMES, 64
    word = plane(case.word, B, ld, 0, torch.uint8, 0)
    noise = plane(case.noise, B, ld, 0, torch.float64, 0.0)
    llr = torch.zeros((N, ld), dtype=torch.float64, device="cuda")
    launch_llr(case.channel, case.coef, case.point if case.channel == "bsc" else case.vsqrt, B, ld, word, noise, llr)
    synd = torch.zeros((N - K, ld), dtype=torch.uint8, device="cuda")
    _lib.check(L.qr_syndrome_device(dec.handle, B, ld, vp(word), vp(synd), None))
    fin, succ, its = dec.decode_device(llr, synd, B, MAXITER)
    out = {}
    for Kk in (K, N):
        ferr = torch.empty(B, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(5, dtype=torch.int64, device="cuda")
        _lib.check(L.qr_count_errors_neg_device(B, ld, Kk, vp(fin), vp(word), vp(succ), vp(its), vp(ferr), vp(cnt),
                                                None))
        out[Kk] = (ferr, cnt)
    torch.cuda.synchronize()
    assert np.array_equal(synd[:, :B].cpu().numpy().T, case.synd)
    assert np.array_equal(succ.cpu().numpy(), case.success) and np.array_equal(its.cpu().numpy(), case.iters)
    assert np.array_equal(out[K][0].cpu().numpy(), case.err_k) and np.array_equal(out[N][0].cpu().numpy(), case.err_n)
    s64 = case.success.astype(np.int64)
    for Kk, e in ((K, case.err_k), (N, case.err_n)):
        assert out[Kk][1].cpu().numpy().tolist() == [int(e.sum()), int((e > 0).sum()), int(s64.sum()),
                                                     int((case.iters * s64).sum()), B]
    assert_bit_exact(fin[:, :4].cpu().numpy().T, case.final)


# thresholds from the fixture's harder points: about 4.7 (soft, -1.5 dB), 15 (hard, 0 dB) bit errors
# per frame over K and 12 (BSC, 0.07) over N, so the count is met after some 80 frames of 300: past
# the index bounds (15 and 20) and, at batch 48, inside the second batch
@pytest.mark.parametrize("channel,point,min_errors", [("biawgn", -1.5, 400), ("biawgn_hard", 0.0, 1200),
                                                      ("bsc", 0.07, 1000)])
def test_run_point_is_the_sequential_loop(gpu, code, channel, point, min_errors):
    """run_point stops at the script's frame, not at a batch boundary: the GPU's own frames (captured
    through the hook), re-decoded by the oracle and counted with `final < 0`, run through a plain
    sequential loop, give the returned tuple."""
    import torch
    from qamr.sim_binary import BinaryChannelSimulator

    dec, orc = code
    loops, batch = 300, 48
    sim = BinaryChannelSimulator(dec, channel, max_iterations=MAXITER, batch=batch)
    seen = []

    def hook(bidx, llr, synd, word, B):
        torch.cuda.synchronize()
        seen.append((bidx, llr[:, :B].cpu().numpy().T.copy(), synd[:, :B].cpu().numpy().T.copy(),
                     word[:, :B].cpu().numpy().T.copy()))

    got = sim.run_point(point, loops, min_errors, seed=4, hook=hook)
    per = []
    for bidx, Lr, Sy, W in sorted(seen, key=lambda t: t[0]):
        for f in range(0, Lr.shape[0], 11):
            assert np.array_equal(Sy[f], orc.eval_syndrome(W[f]))
        s, i, fin = orc.decode_batch(Lr, Sy, MAXITER)
        e = ((fin < 0).astype(np.uint8) ^ W)[:, :sim.K].sum(1)
        per += [(int(e[k]), int(s[k]), int(i[k])) for k in range(Lr.shape[0])]
    assert sim.K == (N if channel == "bsc" else K)
    ref = sequential(sim.stop_rule(loops, min_errors), per, min(loops, len(per)))
    print(f"{channel} {point}: stop after {ref[4]} frames, counters {ref}, tuple {got}")
    assert got == result_tuple(point, ref, sim.K), (got, ref)
    assert ref[4] < loops and ref[4] % batch != 0, ref      # the stop fell inside a batch
    assert len(per) == -(-ref[4] // batch) * batch          # and no batch ran after it


@pytest.mark.parametrize("cli,column,argv", [
    ("sim_decode", "EbN0dB", ["--snr", "-1.5", "0.5", "--nsnr", "2"]),
    ("sim_direct", "EsN0dB", ["--snr", "0", "2", "--nsnr", "2", "--hard"]),
    ("sim_bsc", "f", ["--rber", "0.07", "0.03", "--rpoints", "2"]),
])
def test_cli_two_point_sweep(gpu, tmp_path, cli, column, argv):
    import importlib

    from qamr import codes

    vid, cid = codes.regular_code(N)
    p = tmp_path / "code.csv"
    codes.save_edge_csv(str(p), vid, cid)
    out = tmp_path / "out.csv"
    main = importlib.import_module(f"qamr.{cli}").main
    # a count no run can reach: all 128 frames of both points are decoded
    rows = main([str(p), "--out", str(out), "--batch", "64", "--simloops", "128", "--minerr", "100000000"] + argv)
    assert len(rows) == 2 and rows[1][2] <= rows[0][2] and rows[0][2] > 0    # FER: harder point first
    lines = open(out).read().splitlines()
    assert lines[0] == f",{column},ber,fer,iters" and len(lines) == 3
    assert [ln.split(",")[0] for ln in lines[1:]] == ["0", "1"]
    assert float(lines[1].split(",")[3]) == rows[0][2]
