"""Rate adaptation on the GPU (csrc/rate_adapt.hip; DESIGN.md "Rate adaptation"): the expand kernel bit-exact
against qamr.rate_adapt.expand_host, the row-listed error count against the oracle and against
qr_count_errors_device, both launches on a stream and in a replayed graph, Simulator(adapt=...) and blind_batch
against the oracle's decode of the same inputs, and the effect of shortening and puncturing on the 1008 code."""
import functools
import math

import numpy as np
import pytest

from conftest import assert_bit_exact

pytestmark = pytest.mark.gpu

LPAD, WPAD = -7.25, 0x5A          # what the outputs hold before a call
SPECIALS = (math.nan, math.inf, -math.inf, -0.0, 1e300, -1e300)


@functools.lru_cache(None)
def code1008():
    from qamr import codes
    from qamr.rate_adapt import untainted_order

    vid, cid = codes.regular_code(1008, 3, 6, seed=0)
    order, u = untainted_order(vid, cid, 0)
    return vid, cid, order, u


@functools.lru_cache(None)
def oracle_code():
    import oracle as O

    vid, cid, _, _ = code1008()
    return O.OracleCode(vid, cid)


def adaption(V, p, s):
    from qamr.rate_adapt import RateAdaption

    order = code1008()[2] if V == 1008 else np.array([4, 8, 1, 6, 0, 9, 3, 2, 7, 5])
    return RateAdaption.from_order(order, p, s)


def to_fi(a, ld, fill):
    """[B, rows] host -> frame-innermost [rows, ld] on the GPU, the padding columns filled with `fill`."""
    import torch

    B, V = a.shape
    t = torch.full((V, ld), fill, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    if V:
        t[:, :B] = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
    return t


def host_batch(a, B, seed):
    """(lappr_pay [B, n] with the specials planted in the first and the last frame, word_pay, fill with
    non-zero bytes other than 1)."""
    rng = np.random.default_rng(seed)
    lp = rng.normal(0, 5, (B, a.n))
    for i, v in enumerate(SPECIALS):
        lp[0, i % a.n] = v
        lp[B - 1, (a.n - 1 - i) % a.n] = v
    wp = rng.integers(0, 2, (B, a.n), dtype=np.uint8)
    fill = rng.integers(0, 2, (B, a.p + a.s), dtype=np.uint8) * rng.integers(1, 256, (B, a.p + a.s)).astype(np.uint8)
    return lp, wp, fill


def mixed_revealed(p, ld):
    return np.resize(np.array([0, 1, p, p + 5, -3], np.int32), ld)


def run_expand(a, lp, wp, fill, ld, revealed):
    """expand_device into sentinel-filled outputs one row longer than the interface says -> the two padded
    host arrays [V + 1, ld]."""
    import torch

    B = lp.shape[0]
    lt, wt, ft = to_fi(lp, ld, math.nan), to_fi(wp, ld, 255), to_fi(fill, ld, 255)
    lappr = torch.full((a.V + 1, ld), LPAD, dtype=torch.float64, device="cuda")
    word = torch.full((a.V + 1, ld), WPAD, dtype=torch.uint8, device="cuda")
    rev = None if revealed is None else torch.from_numpy(revealed).cuda()
    a.expand_device(lt, wt, ft, B, rev, out=(lappr[:a.V], word[:a.V]))
    torch.cuda.synchronize()
    return lappr.cpu().numpy(), word.cpu().numpy()


def check_expand(a, got, ref, B):
    lappr, word = got
    rl, rw = ref
    assert_bit_exact(lappr[:a.V, :B].T, rl)
    assert np.array_equal(np.signbit(lappr[:a.V, :B].T), np.signbit(rl))
    assert np.array_equal(word[:a.V, :B].T, rw)
    assert (lappr[:, B:] == LPAD).all() and (lappr[a.V] == LPAD).all()      # untouched: padding columns, extra row
    assert (word[:, B:] == WPAD).all() and (word[a.V] == WPAD).all()


@pytest.mark.parametrize("B", [1, 3, 64, 70, 300])
@pytest.mark.parametrize("V,p,s", [(1008, 0, 0), (1008, 100, 0), (1008, 0, 50), (1008, 60, 36), (10, 4, 4)])
def test_expand_bit_exact_against_expand_host(gpu, V, p, s, B):
    from qamr.pipeline import leading_dim
    from qamr.rate_adapt import expand_host

    a = adaption(V, p, s)
    ld = leading_dim(B)
    assert ld == {1: 64, 3: 64, 64: 64, 70: 128, 300: 512}[B]
    lp, wp, fill = host_batch(a, B, 1000 + V + 7 * p + s + B)
    for revealed in (None, mixed_revealed(p, ld)):
        ref = expand_host(a, lp, wp, fill, None if revealed is None else revealed[:B])
        got = run_expand(a, lp, wp, fill, ld, revealed)
        check_expand(a, got, ref, B)
        if p + s == 0:       # no filler: the outputs are the inputs
            assert_bit_exact(got[0][:V, :B].T, lp)
            assert np.array_equal(got[1][:V, :B].T, wp)
    if p and (s or B >= 3):   # the mixed vector: both kinds of filler among the frames (frame 0 reveals nothing)
        known = ref[0][:, a.fillers]
        assert (known == 0.0).any() and (np.abs(known) == 1e300).any()


@pytest.mark.parametrize("ld", [4096, 4352])
def test_expand_at_the_offset_shape(gpu, ld):
    """V = 64 800, B = ld, (p, s) = (6 480, 0), compared on the device with an index_select of the payload rows
    plus zero rows.  At ld = 4 096 (the shape the issue names) the last row's byte offset is V * ld * 8 =
    2 123 366 400, 1.1 % short of 2^31; at ld = 4 352 it is 2 256 076 800 and a 32-bit byte offset wraps in
    the last 3 118 rows."""
    import torch
    from qamr.rate_adapt import RateAdaption

    V, p, B = 64800, 6480, ld
    assert (V * 4352 * 8 > 2 ** 31) and (V * 4096 * 8 < 2 ** 31)
    a = RateAdaption.from_order(np.random.default_rng(5).permutation(V), p, 0)
    gen = torch.Generator(device="cuda").manual_seed(9)
    lp = torch.randn((a.n, ld), generator=gen, device="cuda", dtype=torch.float64)
    wp = torch.randint(0, 2, (a.n, ld), generator=gen, device="cuda", dtype=torch.uint8)
    fill = torch.randint(0, 2, (p, ld), generator=gen, device="cuda", dtype=torch.uint8)
    lappr, word = a.expand_device(lp, wp, fill, B)
    slot = torch.from_numpy(a.slot.astype(np.int64)).cuda()
    src = torch.where(slot >= 0, slot, a.n - 1 - slot)             # payload row k -> k, filler j -> n + j
    want = torch.index_select(torch.cat([lp, torch.zeros((p, ld), dtype=torch.float64, device="cuda")]), 0, src)
    assert torch.equal(lappr.view(torch.int64), want.view(torch.int64))
    del want
    want_w = torch.index_select(torch.cat([wp, fill]), 0, src)
    assert torch.equal(word, want_w)
    assert int(a.payload_rows[-1]) * ld * 8 > (2 ** 31 if ld == 4352 else 2 ** 30)


# ---------------------------------------------------------------------------------------------- row-listed count
def count_case(B=70, seed=4):
    """final / word [V, ld] with NaN finals, success, iters on the GPU, and their host copies."""
    import torch

    V, ld = 1008, 128
    rng = np.random.default_rng(seed)
    fin = rng.normal(0, 3, (B, V))
    fin[rng.random((B, V)) < 0.02] = math.nan
    fin[0, :8] = [math.nan, -0.0, 0.0, math.inf, -math.inf, 1e300, -1e300, math.nan]
    fin[5] = np.abs(fin[5])                 # a frame without an error
    word = rng.integers(0, 2, (B, V), dtype=np.uint8)
    word[5] = 0
    fin[5, np.isnan(fin[5])] = 1.0
    succ = rng.integers(0, 2, B, dtype=np.uint8)
    its = rng.integers(1, 51, B).astype(np.int32)
    dev = (to_fi(fin, ld, math.nan), to_fi(word, ld, 255), torch.from_numpy(succ).cuda(), torch.from_numpy(its).cuda())
    return V, ld, fin, word, succ, its, dev


def test_count_rows_against_the_oracle(gpu):
    import oracle as O
    import torch

    B = 70
    V, ld, fin, word, succ, its, (ft, wt, st, it) = count_case(B)
    a = adaption(1008, 60, 36)
    rows = a.payload_rows
    ferr = torch.full((B + 1,), -9, dtype=torch.int32, device="cuda")
    start = np.array([11, 22, 33, 44, 55], np.int64)
    counters = torch.from_numpy(np.append(start, -1)).cuda()
    a.count_errors_device(B, ld, ft, wt, st, it, ferr, counters)
    torch.cuda.synchronize()
    want = np.array([O.count_errors_from_lappr(fin[f, rows], word[f, rows]) for f in range(B)])
    assert want[5] == 0 and (want > 0).sum() == B - 1
    got = ferr.cpu().numpy()
    assert np.array_equal(got[:B], want) and got[B] == -9
    delta = [want.sum(), (want > 0).sum(), succ.sum(), (its.astype(np.int64) * succ).sum(), B]
    c = counters.cpu().numpy()
    assert np.array_equal(c[:5], start + np.array(delta, np.int64)) and c[5] == -1      # accumulated, not cleared


def test_count_rows_with_the_first_K_rows_equals_count_errors(gpu):
    import torch
    from qamr import _lib
    from qamr._lib import dptr
    from qamr.pipeline import count_errors_device

    B, K = 70, 504
    V, ld, fin, word, succ, its, (ft, wt, st, it) = count_case(B, seed=6)
    rows = torch.arange(K, dtype=torch.int32, device="cuda")
    out = []
    for listed in (False, True):
        ferr = torch.full((B,), -9, dtype=torch.int32, device="cuda")
        counters = torch.tensor([5, 4, 3, 2, 1], dtype=torch.int64, device="cuda")
        if listed:
            _lib.check(_lib.load().qr_count_errors_rows_device(B, ld, K, dptr(rows), dptr(ft), dptr(wt), dptr(st), dptr(it),
                                                               dptr(ferr), dptr(counters), None))
        else:
            count_errors_device(False, B, ld, K, ft, wt, st, it, ferr, counters)
        torch.cuda.synchronize()
        out.append((ferr.cpu().numpy(), counters.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][1][0] > 5 and out[0][1][4] == 1 + B


# ------------------------------------------------------------------------------------------- stream, graph replay
def test_stream_and_graph_replay(gpu):
    """Both launches on a non-default stream, then captured once and replayed on replaced inputs."""
    import oracle as O
    import torch
    from qamr.rate_adapt import expand_host

    a = adaption(1008, 60, 36)
    B, ld = 70, 128
    rev = mixed_revealed(a.p, ld)
    rows = a.payload_rows
    batches = [host_batch(a, B, 31), host_batch(a, B, 32)]
    refs = [expand_host(a, *b, rev[:B]) for b in batches]
    lt, wt, ft = (to_fi(x, ld, pad) for x, pad in zip(batches[0], (math.nan, 255, 255)))
    rt = torch.from_numpy(rev).cuda()
    succ = torch.ones(B, dtype=torch.uint8, device="cuda")
    its = torch.full((B,), 3, dtype=torch.int32, device="cuda")
    ferr = torch.zeros(B, dtype=torch.int32, device="cuda")
    counters = torch.zeros(5, dtype=torch.int64, device="cuda")
    bits = torch.zeros((a.V, ld), dtype=torch.uint8, device="cuda")     # the word the LAPPRs are counted against

    def want_errors(ref):
        return np.array([O.count_errors_from_lappr(ref[0][f, rows], np.zeros(rows.size, np.uint8)) for f in range(B)])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        lappr, word = a.expand_device(lt, wt, ft, B, rt, stream=s)
        a.count_errors_device(B, ld, lappr, bits, succ, its, ferr, counters, stream=s)
    torch.cuda.synchronize()
    assert_bit_exact(lappr[:, :B].cpu().numpy().T, refs[0][0])
    assert np.array_equal(word[:, :B].cpu().numpy().T, refs[0][1])
    assert np.array_equal(ferr.cpu().numpy(), want_errors(refs[0]))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        a.expand_device(lt, wt, ft, B, rt, out=(lappr, word))
        a.count_errors_device(B, ld, lappr, bits, succ, its, ferr, counters)
    for t, x, pad in zip((lt, wt, ft), batches[1], (math.nan, 255, 255)):
        t.copy_(to_fi(x, ld, pad))
    lappr.fill_(LPAD)
    word.fill_(WPAD)
    ferr.fill_(-1)
    counters.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_bit_exact(lappr[:, :B].cpu().numpy().T, refs[1][0])
    assert np.array_equal(word[:, :B].cpu().numpy().T, refs[1][1])
    assert (lappr[:, B:] == LPAD).all() and (word[:, B:] == WPAD).all()
    e = want_errors(refs[1])
    assert np.array_equal(ferr.cpu().numpy(), e)
    assert counters.cpu().numpy().tolist() == [e.sum(), (e > 0).sum(), B, 3 * B, B]


# ---------------------------------------------------------------------------------------------------- end to end
def make_sim(p, s, batch, **kw):
    import qamr
    from qamr import sim

    vid, cid, order, _ = code1008()
    dec = qamr.Decoder(vid, cid)
    adapt = None if p + s == 0 else adaption(1008, p, s)
    return sim.Simulator(dec, 2, "softening", 50, 1.0, batch, adapt=adapt, **kw)


def mapper(s, snr_db):
    import qamr

    two_var = s.pa.variance * 10 ** (-snr_db / 10)
    return qamr.NoiseMapper(s.pa, two_var / 2, s.cfg), two_var


def test_simulator_end_to_end_against_the_oracle(gpu):
    import oracle as O
    import torch

    B, snr = 96, 5.0
    s = make_sim(100, 100, B)
    a = s.adapt
    seen = {}

    def hook(bidx, lappr, synd, word, b):
        assert bidx == 0 and b == B
        seen["in"] = (lappr.clone(), synd.clone(), word.clone())

    got = s.run_snr(snr, B, 10 ** 9, seed=3, hook=hook)
    lappr, synd, word = seen["in"]
    fin, succ, its = s.dec.decode_device(lappr, synd, B, 50)
    torch.cuda.synchronize()
    L = np.ascontiguousarray(lappr[:, :B].cpu().numpy().T)
    w = np.ascontiguousarray(word[:, :B].cpu().numpy().T)
    sy = np.ascontiguousarray(synd[:, :B].cpu().numpy().T)
    # the fillers: punctured +0.0, shortened +-1e300 agreeing with the word
    assert (L[:, a.punctured] == 0.0).all() and not np.signbit(L[:, a.punctured]).any()
    assert np.array_equal(L[:, a.shortened], np.where(w[:, a.shortened] == 0, 1e300, -1e300))
    assert set(np.unique(w)) <= {0, 1} and 0.3 < w[:, a.fillers].mean() < 0.7
    orc = oracle_code()
    assert np.array_equal(sy, np.stack([orc.eval_syndrome(w[f]) for f in range(B)]))
    s2, i2, f2 = orc.decode_batch(L, sy, 50)
    assert np.array_equal(succ.cpu().numpy(), s2) and np.array_equal(its.cpu().numpy(), i2)
    assert_bit_exact(fin[:, :B].cpu().numpy().T, f2)
    errs = np.array([O.count_errors_from_lappr(f2[f, a.payload_rows], w[f, a.payload_rows]) for f in range(B)])
    ok = s2.astype(np.int64)
    want = (snr, errs.sum() / (B * a.n), (errs > 0).sum() / B, 0 if ok.sum() == 0 else (i2.astype(np.int64) * ok).sum() / ok.sum())
    assert got == want
    assert ok.sum() >= B // 2           # the rehearsal decoded 46 of 48 here


def test_adapt_needs_the_torch_stream(gpu):
    from qamr import sim

    with pytest.raises(ValueError):
        make_sim(100, 100, 64, stream="numpy")
    vid, cid, order, _ = code1008()
    with pytest.raises(ValueError):
        sim.simulate_softening_snr_dB(5.0, make_sim(0, 0, 64).dec, 2, np.array([0, 1, 0, 1], np.uint8), 50, 64, 100,
                                      stream="numpy", adapt=adaption(1008, 100, 100))


@pytest.mark.parametrize("mode", ["direct", "hard"])
def test_the_other_modes_take_an_adaptation(gpu, mode):
    """frames() in the direct and hard modes: the payload rows are what llr_source gives for n / bps symbols
    with the same generator, the fillers are drawn after them."""
    import qamr
    import torch
    from qamr import sim

    vid, cid, _, _ = code1008()
    a = adaption(1008, 60, 36)
    s = sim.Simulator(qamr.Decoder(vid, cid), 2, mode, batch=64, adapt=a)
    two_var = s.pa.variance * 10 ** (-0.5)
    nm = qamr.NoiseMapper(s.pa, two_var / 2, None)
    B = 5
    gen = lambda: torch.Generator(device="cuda").manual_seed(8)   # noqa: E731
    lappr, synd, word, ld = s.frames(nm, B, gen(), two_var)
    g = gen()
    l2, w2 = sim.llr_source(nm, s.pa, a.n // 2, B, g, mode, "search", 1.0, two_var)
    fill = torch.randint(0, 2, (a.p + a.s, ld), dtype=torch.uint8, generator=g, device="cuda")
    rows = torch.from_numpy(a.payload_rows).cuda()
    assert torch.equal(lappr[rows, :B].view(torch.int64), l2[:, :B].view(torch.int64))
    assert torch.equal(word[rows, :B], w2[:, :B])
    assert torch.equal(word[torch.from_numpy(a.fillers).cuda(), :B], fill[:, :B])
    assert synd.shape == (s.C, ld)


# -------------------------------------------------------------------------------------------------------- effect
def decoded_fraction(snr_db, p, s, frames=256, seed=11):
    import torch

    sm = make_sim(p, s, frames)
    nm, two_var = mapper(sm, snr_db)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    _, succ, _, _ = sm.batch_results(nm, frames, gen, two_var)
    return float(succ.to(torch.float64).mean())


def test_effect_of_shortening_and_puncturing(gpu):
    """Conditions the CPU rehearsal with the oracle stays inside with room (48 numpy frames per point: 3.0 dB
    0 % unadapted and 75 % at s = 200; 4.0 dB 48 % unadapted and 4 % at p = 100; 6.0 dB 100 % at p = 100)."""
    f = {k: decoded_fraction(*k) for k in ((3.0, 0, 0), (3.0, 0, 200), (4.0, 0, 0), (4.0, 100, 0), (6.0, 100, 0))}
    print({f"{k[0]} dB p={k[1]} s={k[2]}": v for k, v in f.items()})
    assert f[(3.0, 0, 0)] <= 0.10 and f[(3.0, 0, 200)] >= 0.50
    assert f[(4.0, 0, 0)] >= 0.30 and f[(4.0, 100, 0)] <= 0.15
    assert f[(6.0, 100, 0)] >= 0.95


# ---------------------------------------------------------------------------------------------------------- CLIs
def test_clis(gpu, tmp_path, capsys):
    """qamr.sim_rate_adapt: the header, one row per point, the same file for the same seed, blind rounds that
    only help; qamr.sim_reconciliation --punctured / --shortened: the rate line, the warning past u, the
    unchanged CSV schema, and the row Simulator(adapt=...) returns."""
    from qamr import codes, sim_rate_adapt, sim_reconciliation

    vid, cid, order, u = code1008()
    csv = str(tmp_path / "code.csv")
    codes.save_edge_csv(csv, vid, cid)
    argv = [csv] + "--snr 4.5 5.5 --nsnr 2 --punctured 100 --frames 96 --batch 64 --seed 2".split()
    outs = [str(tmp_path / f"o{i}.csv") for i in range(3)]
    plain = sim_rate_adapt.main(argv + ["--out", outs[0]])
    sim_rate_adapt.main(argv + ["--out", outs[1]])
    blind = sim_rate_adapt.main(argv + ["--out", outs[2], "--blind-rounds", "2", "--blind-step", "50"])
    lines = open(outs[0]).read().splitlines()
    assert open(outs[1]).read().splitlines() == lines
    assert lines[0] == "EsN0dB,fer,ber,iters,fer_round0,revealed_mean,rate_mean" and len(lines) == 3
    rate = (504 - 0) / (1008 - 100)
    for r, b in zip(plain, blind):
        assert r[5] == 0.0 and r[6] == rate                               # no round: nothing revealed
        assert b[4] == r[4] and b[1] <= r[1] and 0 <= b[5] <= 100 and b[6] == (504 - b[5]) / 908
    assert plain[0][4] > 0 and blind[0][5] > 0        # 4.5 dB, p = 100: some frames fail and get bits disclosed
    capsys.readouterr()
    out = str(tmp_path / "r.csv")
    rows = sim_reconciliation.main([csv, "--snr", "5", "5", "--nsnr", "1", "--simloops", "64", "--batch", "64", "--out", out,
                                    "--punctured", "140", "--shortened", "100", "--adapt-seed", "0"])
    cap = capsys.readouterr()
    assert "rate adaptation: p=140 s=100 payload n=768 rate=0.526042" in cap.out and f"u={u}" in cap.out
    assert "--punctured 140 > u = 132" in cap.err
    txt = open(out).read().splitlines()
    assert txt[0] == ",EsN0dB,ber,fer,iters" and len(txt) == 2
    s = make_sim(140, 100, 64)
    assert rows[0] == s.run_snr(5.0, 64, 100, 0)


# --------------------------------------------------------------------------------------------------------- blind
def test_blind_rounds_against_a_host_replay(gpu):
    import torch
    from qamr.rate_adapt import blind_batch, expand_host

    B, p, step, rounds = 128, 100, 50, 2
    s = make_sim(p, 0, B)
    a = s.adapt
    nm, two_var = mapper(s, 5.0)
    seen = {}

    def hook(lp, wp, fill, b):
        seen["pay"] = tuple(np.ascontiguousarray(t[:, :b].cpu().numpy().T) for t in (lp, wp, fill))

    gen = torch.Generator(device="cuda").manual_seed(21)
    r = blind_batch(s, nm, B, gen, two_var, rounds, step, hook=hook)
    torch.cuda.synchronize()
    lp, wp, fill = seen["pay"]
    orc = oracle_code()
    # the same loop on the host: expand_host and the oracle
    rev = np.zeros(B, np.int64)
    L, w = expand_host(a, lp, wp, fill, rev)
    synd = np.stack([orc.eval_syndrome(w[f]) for f in range(B)])
    succ, its, fin = orc.decode_batch(L, synd, 50)
    succ0 = succ.copy()
    total = its.astype(np.int64)
    attempts = np.ones(B, np.int64)
    for _ in range(rounds):
        idx = np.flatnonzero((succ == 0) & (rev < p))
        if idx.size == 0:
            break
        rev[idx] = np.minimum(rev[idx] + step, p)
        L, _ = expand_host(a, lp, wp, fill, rev)
        s2, i2, f2 = orc.decode_batch(L[idx], synd[idx], 50)
        succ[idx], its[idx], fin[idx] = s2, i2, f2
        total[idx] += i2
        attempts[idx] += 1
    out = {k: v.cpu().numpy() for k, v in r.items()}
    assert np.array_equal(out["success_round0"], succ0)
    assert np.array_equal(out["success"], succ) and np.array_equal(out["iterations"], its)
    assert np.array_equal(out["iterations_total"], total) and np.array_equal(out["attempts"], attempts)
    assert np.array_equal(out["revealed"], rev)
    assert_bit_exact(out["final"][:, :B].T, fin)
    assert np.array_equal(out["word"][:, :B].T, w)
    # the loop's own properties
    assert np.array_equal(rev, np.minimum(step * (attempts - 1), p))
    assert (attempts[succ0 == 1] == 1).all()                    # no frame that succeeded is decoded again
    assert succ.sum() >= succ0.sum()
    rescued = int(((succ0 == 0) & (succ == 1)).sum())
    print(f"blind: {int(succ0.sum())} of {B} after round 0, {int(succ.sum())} at the end, {rescued} rescued")
    assert rescued >= 1
