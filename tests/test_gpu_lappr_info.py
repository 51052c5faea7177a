"""The LAPPR information rate on the GPU (csrc/lappr_info.hip; DESIGN.md "LAPPR information rate"): every output
bit-exact against the host evaluator of tests/lappr_info_fixture.py (libm per element, the normative sum order).

Inputs: LAPPRs the oracle demapped, with Bob's bits.  The oracle's search costs M hypotheses per symbol, so a
pool of symbols is demapped once per constellation (2-, 4- and 16-PAM) and the frames of a case draw their
symbols from the pool with a seeded index; at 8 bits per symbol a symbol is two 16-PAM symbols' LAPPRs side by
side (the oracle's 256-PAM search takes minutes; the estimator reads elements, not constellations)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from conftest import assert_bit_exact

import lappr_info_fixture as F
import workspace_fixture as W

pytestmark = pytest.mark.gpu

POOL = {1: (1, 1.0, 3000), 2: (2, 3.0, 3000), 4: (4, 13.0, 1500), 8: (4, 13.0, 1500)}   # bps -> oracle bps, dB, symbols


@functools.lru_cache(None)
def pool(obps, snr_db, n):
    """(lappr [n, obps], bits [n, obps]) of n oracle-demapped symbols."""
    L, w = F.oracle_frames(obps, snr_db, n, 1, 900 + obps)
    return L.reshape(n, obps), w.reshape(n, obps)


def frames(bps, S, B, seed, plant=True):
    """B frames of S symbols drawn from the pool, the specials planted (unless plant is false)
    -> (lappr [B, S * bps], word [B, S * bps])."""
    obps, snr, n = POOL[bps]
    pL, pw = pool(obps, snr, n)
    per = bps // obps
    idx = np.random.default_rng(seed).integers(0, n, (B, S * per))
    L = np.ascontiguousarray(pL[idx].reshape(B, S * bps))
    w = np.ascontiguousarray(pw[idx].reshape(B, S * bps))
    return (F.plant_specials(L, bps) if plant else L), w


def to_fi(a, ld, fill):
    """[B, V] host -> frame-innermost [V, ld] on the GPU, the padding columns filled with `fill`."""
    import torch

    B, V = a.shape
    t = torch.full((V, ld), fill, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    t[:, :B] = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
    return t


def info_ws_map(bps, ld, S, A):
    """The workspace of qr_lappr_info_device (lappr_info.hip info_workspace) in the form of
    workspace_fixture.decode_ws_map: the chunk sums wloss [A][bps][chunks][ld] fp64, then the chunk error
    counts werr [bps][chunks][ld] int32.  Both are summed and never used as indices, so any value is in range;
    the typed fill gives werr the "index" pattern, a wrong count."""
    rows = bps * -(-S // 256) * ld
    n0 = W.A256(8 * A * rows)
    return [("wloss", 0, n0, "f64"), ("werr", n0, W.A256(4 * rows), "index")]


def run_raw(L, w, bps, alphas, ld, fill="typed", donor=None):
    """qr_lappr_info_device on its own buffers: NaN LAPPRs and bits of 255 in the padding columns, every output
    one row longer than the interface says and pre-filled with a pad value -> the four padded host arrays.  The
    workspace lies between two guards and holds the given fill (tests/workspace_fixture.py) when the call
    starts; ``run_raw.last_view`` is the workspace view afterwards (a donor for "leftover")."""
    import torch

    from qamr import _lib
    from qamr._lib import dptr

    B, V = L.shape
    S, A = V // bps, len(alphas)
    Lt, wt = to_fi(L, ld, math.nan), to_fi(w, ld, 255)
    loss = torch.full((A * bps + 1, ld), F.PAD, dtype=torch.float64, device="cuda")
    errors = torch.full((bps + 1, ld), -7, dtype=torch.int32, device="cuda")
    total = torch.full((A * bps + 1,), F.PAD, dtype=torch.float64, device="cuda")
    terr = torch.full((bps + 1,), -7, dtype=torch.int64, device="cuda")
    lib = _lib.load()
    need = C.c_size_t(0)
    _lib.check(lib.qr_lappr_info_workspace_size(bps, ld, S, A, C.byref(need)))
    m = info_ws_map(bps, ld, S, A)
    assert W.map_bytes(m) == need.value
    guard = W.guard_bytes(ld)
    whole, ws = W.guarded(need.value, guard)
    W.fill(ws, fill, m, ld, donor)
    al = np.ascontiguousarray(alphas, np.float64)
    _lib.check(lib.qr_lappr_info_device(bps, B, ld, S, dptr(Lt), dptr(wt), A, _lib.ptr(al), dptr(loss), dptr(errors),
                                        dptr(total), dptr(terr), dptr(ws), need.value,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    W.assert_guards(whole, guard, need.value, "qr_lappr_info_device")
    run_raw.last_view = ws
    got = loss.cpu().numpy(), errors.cpu().numpy(), total.cpu().numpy(), terr.cpu().numpy()
    W.assert_no_fill_payload(got[0], "loss")
    W.assert_no_fill_payload(got[2], "total")
    return got


def check_against(ref, got, A, bps, B, ld):
    rloss, rerr, rtotal, rterr = ref
    loss, errors, total, terr = got
    assert_bit_exact(loss[:A * bps, :B].reshape(A, bps, B), rloss)
    assert np.array_equal(errors[:bps, :B], rerr)
    assert_bit_exact(total[:A * bps].reshape(A, bps), rtotal)
    assert np.array_equal(terr[:bps], rterr)
    # untouched: the padding columns, the extra row
    assert (loss[:, B:] == F.PAD).all() and (loss[A * bps] == F.PAD).all()
    assert (errors[:, B:] == -7).all() and (errors[bps] == -7).all()
    assert total[A * bps] == F.PAD and terr[bps] == -7


# (S, bps, B, A): every S, bps, B and A of the issue's lists; at most 4.0e5 terms (S bps B A) per case
CASES = [(1, 1, 1, 1), (255, 2, 3, 3), (256, 4, 64, 1), (257, 8, 65, 3), (513, 2, 3, 16), (513, 1, 64, 3),
         (256, 2, 1, 16), (257, 4, 3, 3), (255, 8, 64, 1), (1, 8, 65, 3), (513, 4, 65, 1), (255, 1, 65, 16)]
# k_lappr_info_total walks the frames in passes of 1024 and reuses its LDS array between them: B = 1025 is one
# frame into the second pass, B = 2049 one into the third
PASS_CASES = [(1, 1, 1025, 1), (3, 2, 2049, 3)]
CASES += PASS_CASES


@pytest.mark.parametrize("S,bps,B,A", CASES)
def test_bit_exact_against_the_evaluator(gpu, S, bps, B, A):
    assert S * bps * B * A <= 4.02e5
    L, w = frames(bps, S, B, 7000 + S + 10 * bps + B)
    alphas = F.SCALES[:A] if A > 1 else ((1.0,) if S != 256 else (0.5,))
    ld = -(-B // 64) * 64
    ref = F.evaluate(L, w, bps, alphas)
    n_special = int((~np.isfinite(ref[0])).sum())
    got = run_raw(L, w, bps, alphas, ld)
    check_against(ref, got, A, bps, B, ld)
    if S * bps >= len(F.SPECIALS):   # the planted inf / NaN reach the sums of the first and of the last frame
        assert n_special > 0 and not np.isfinite(ref[0][:, :, B - 1]).all()


@pytest.mark.parametrize("S,bps,B,A", PASS_CASES)
def test_totals_past_one_pass_on_finite_frames(gpu, S, bps, B, A):
    """The shapes of PASS_CASES without the planted specials (which put an inf or a NaN into the totals of the
    case above from the first or the last frame on, whatever the later passes add): every total is finite, so
    each pass's partial sum and the order of the chain over all B frames show in its last bits."""
    L, w = frames(bps, S, B, 7100 + B, plant=False)
    alphas = F.SCALES[:A] if A > 1 else (1.0,)
    ld = -(-B // 64) * 64
    ref = F.evaluate(L, w, bps, alphas)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[2]).all() and (ref[2] > 0).all()
    check_against(ref, run_raw(L, w, bps, alphas, ld), A, bps, B, ld)


def test_python_wrapper_equals_raw_entry(gpu):
    from qamr.mutual_information import lappr_information_device

    S, bps, B, A = 300, 2, 3, 3
    L, w = frames(bps, S, B, 11)
    alphas = (0.5, 0.8, 1.0)
    ref = F.evaluate(L, w, bps, alphas)
    r = lappr_information_device(to_fi(L, 64, math.nan), to_fi(w, 64, 255), B, bps, alphas)
    assert r.loss.shape == (A, bps, B) and r.errors.shape == (bps, B) and r.total.shape == (A, bps)
    assert_bit_exact(r.loss.cpu().numpy(), ref[0])
    assert np.array_equal(r.errors.cpu().numpy(), ref[1])
    assert_bit_exact(r.total.cpu().numpy(), ref[2])
    assert np.array_equal(r.total_errors.cpu().numpy(), ref[3])
    I, I_level, ber = r.rates(S)
    rI, rI_level = F.rates(ref[2], B, S)
    assert_bit_exact(I, rI)
    assert_bit_exact(I_level, rI_level)
    assert_bit_exact(ber, np.array([float(e) / float(B * S) for e in ref[3]]))


def test_host_entry_on_the_motivating_frame(gpu):
    """lappr_information on the CPU test's 4 000-symbol frame, Bob's side and the demapper on the GPU: the
    evaluator's numbers on the oracle's LAPPRs, and I(0.5) > 1.0 > I(1.0)."""
    import qamr
    from qamr.mutual_information import lappr_information

    x, y, olappr, oword, N0 = F.motivating_frame()
    nm = qamr.NoiseMapper(qamr.PAMAlphabet(2, 2.0), N0, F.alternating(4))
    _, nh, word = nm._bob_host(y)
    lappr = nm.demap_lappr_array(nh, x)
    assert np.array_equal(word, oword)
    assert_bit_exact(lappr, olappr)
    I, I_level, errors = lappr_information(lappr, word, 2, (0.5, 1.0))
    rloss, rerr, rtotal, rterr = F.evaluate(olappr[None], oword[None], 2, (0.5, 1.0))
    rI, rI_level = F.rates(rtotal, 1, 4000)
    assert_bit_exact(I, rI)
    assert_bit_exact(I_level, rI_level)
    assert errors.dtype == np.int64 and np.array_equal(errors, rterr)
    print(f"I(0.5) = {I[0]!r}, I(1.0) = {I[1]!r}")
    assert I[0] > 1.0 > I[1]


@pytest.mark.parametrize("demapper", ["search", "simplified"])
def test_scale_invariance(gpu, demapper):
    """The demapper's own alpha and the estimator's scale are the same multiplication: demap_device(alpha=a)
    estimated at scale 1.0 equals demap_device(alpha=1) estimated at scale a, bit for bit."""
    import qamr
    import torch
    from qamr.mutual_information import lappr_information_device

    S, B, ld = 300, 3, 64
    pa = qamr.PAMAlphabet(2, 2.0)
    N0 = pa.variance * 10 ** (-0.3) / 2
    nm = qamr.NoiseMapper(pa, N0, F.alternating(4))
    gen = torch.Generator(device="cuda").manual_seed(5)
    a = torch.tensor(pa.constellation, dtype=torch.float64, device="cuda")
    x = torch.randint(0, 4, (S, ld), generator=gen, device="cuda", dtype=torch.int64)
    y = a[x] + nm.noise_sigma * torch.randn((S, ld), generator=gen, device="cuda", dtype=torch.float64)
    _, nh, word = nm.bob_map_device(y, B)
    demap = nm.demap_simplified_device if demapper == "simplified" else nm.demap_device
    one = demap(nh, x, B, 1.0)
    for alpha in (0.6, 1.25):
        scaled = demap(nh, x, B, alpha)
        u = lappr_information_device(scaled, word, B, 2, (1.0,))
        v = lappr_information_device(one, word, B, 2, (alpha,))
        assert_bit_exact(u.loss.cpu().numpy(), v.loss.cpu().numpy())
        assert_bit_exact(u.total.cpu().numpy(), v.total.cpu().numpy())
        assert np.array_equal(u.errors.cpu().numpy(), v.errors.cpu().numpy())


def test_stream_and_graph_replay(gpu):
    """A non-default stream, then one captured call replayed on replaced inputs: the evaluator's numbers on
    the new inputs."""
    import torch
    from qamr.mutual_information import lappr_information_device

    S, bps, B = 257, 2, 3
    alphas = (0.5, 1.0, -1.0)
    L0, w0 = frames(bps, S, B, 21)
    L1, w1 = frames(bps, S, B, 22)
    Lt, wt = to_fi(L0, 64, math.nan), to_fi(w0, 64, 255)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r = lappr_information_device(Lt, wt, B, bps, alphas, stream=s)
    torch.cuda.synchronize()
    ref0 = F.evaluate(L0, w0, bps, alphas)
    assert_bit_exact(r.loss.cpu().numpy(), ref0[0])
    assert_bit_exact(r.total.cpu().numpy(), ref0[2])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r = lappr_information_device(Lt, wt, B, bps, alphas)
    Lt.copy_(to_fi(L1, 64, math.nan))
    wt.copy_(to_fi(w1, 64, 255))
    r.loss.fill_(F.PAD)
    r.total.fill_(F.PAD)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    ref1 = F.evaluate(L1, w1, bps, alphas)
    assert_bit_exact(r.loss.cpu().numpy(), ref1[0])
    assert np.array_equal(r.errors.cpu().numpy(), ref1[1])
    assert_bit_exact(r.total.cpu().numpy(), ref1[2])
    assert np.array_equal(r.total_errors.cpu().numpy(), ref1[3])


@pytest.mark.parametrize("mode", ["softening", "direct", "hard"])
def test_llr_source_is_what_simulator_frames_returns(gpu, mode):
    import qamr
    import torch
    from qamr import codes, sim

    vid, cid = codes.regular_code(1008)
    dec = qamr.Decoder(vid, cid)
    s = sim.Simulator(dec, 2, mode, alpha=0.8 if mode == "softening" else 1.0, batch=64)
    two_var = s.pa.variance * 10 ** (-0.35)
    nm = qamr.NoiseMapper(s.pa, two_var / 2, s.cfg if mode == "softening" else None)
    B = 5
    gen = lambda: torch.Generator(device="cuda").manual_seed(77)   # noqa: E731
    lappr, synd, word, ld = s.frames(nm, B, gen(), two_var)
    l2, w2 = sim.llr_source(nm, s.pa, s.S, B, gen(), mode, "search", s.alpha, two_var)
    torch.cuda.synchronize()
    assert ld == 64 and lappr.shape == l2.shape == (s.V, 64) and word.shape == w2.shape
    assert_bit_exact(lappr[:, :B].cpu().numpy(), l2[:, :B].cpu().numpy())
    assert np.array_equal(word[:, :B].cpu().numpy(), w2[:, :B].cpu().numpy())
    assert synd.shape == (s.C, 64)


def test_cli(gpu, tmp_path):
    """--symbols 512 --frames 64 --nsnr 2 --alphas 0.5 1: the header, one row per (point, alpha), the same file
    for the same seed, and every row what lappr_information_device gives on the same seeded frames."""
    import qamr
    import torch
    from qamr import sim, sim_lappr_information as cli
    from qamr.mutual_information import lappr_information_device

    argv = "--symbols 512 --frames 64 --nsnr 2 --snr 3 4 --alphas 0.5 1 --seed 3".split()
    outs = [str(tmp_path / f"o{i}.csv") for i in range(2)]
    for o in outs:
        cli.main(argv + ["--out", o])
    txt = open(outs[0]).read()
    assert txt == open(outs[1]).read()
    lines = txt.splitlines()
    assert lines[0] == "EsN0dB,alpha,I,I_0,I_1,ber_0,ber_1" and len(lines) == 1 + 2 * 2
    pa = qamr.PAMAlphabet(2, 2)
    row = 1
    for i, snr in enumerate((3.0, 4.0)):
        two_var = pa.variance * (10 ** (-snr / 10))
        nm = qamr.NoiseMapper(pa, two_var / 2, F.alternating(4))
        gen = torch.Generator(device="cuda").manual_seed(cli.point_seed(3, i))
        lappr, word = sim.llr_source(nm, pa, 512, 64, gen)
        I, I_level, ber = lappr_information_device(lappr, word, 64, 2, (0.5, 1.0)).rates(512)
        for a, alpha in enumerate((0.5, 1.0)):
            want = [snr, alpha, I[a], *I_level[a], *ber]
            assert lines[row] == ",".join(repr(float(v)) for v in want), (row, lines[row], want)
            row += 1
