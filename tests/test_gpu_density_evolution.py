"""The sampled density evolution on the GPU (csrc/density_evolution.hip; DESIGN.md "Density evolution"): errors,
v2c and c2v bit for bit (NaN-aware) against the restatement of tests/de_fixture.py wherever it runs, and the
theory check of the (3, 6) ensemble's threshold on the GPU alone."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from conftest import assert_bit_exact

import de_fixture as F
import decode_fixture as DF

pytestmark = pytest.mark.gpu

SCOPES = ("de_population", "de_var", "de_check", "de_post")


def make_tables(tables):
    from qamr.density_evolution import DETables

    return DETables(*tables)


def run_raw(u, tables, M, T, seed, handle=None):
    """qr_de_evolve_device on its own buffers, every output one element longer than the interface says and
    pre-filled with a pad value -> (rc, errors, v2c, c2v) padded host arrays."""
    import torch

    from qamr import _lib
    from qamr._lib import dptr

    t = handle if handle is not None else make_tables(tables)
    ut = torch.from_numpy(np.array(u, np.float64)).cuda()   # a copy: the fixture's arrays are read-only
    v2c = torch.full((M + 1,), F.PAD, dtype=torch.float64, device="cuda")
    c2v = torch.full((M + 1,), F.PAD, dtype=torch.float64, device="cuda")
    errors = torch.full((T + 2,), F.PAD_ERRORS, dtype=torch.int64, device="cuda")
    rc = _lib.load().qr_de_evolve_device(t.handle, ut.numel(), dptr(ut), M, T, seed, dptr(v2c), dptr(c2v), dptr(errors),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, errors.cpu().numpy(), v2c.cpu().numpy(), c2v.cpu().numpy()


def check_against(ref, got, M, T):
    """ref = (errors [T + 1], v2c(T) or None, c2v(T)); the cells past the interface's sizes are untouched."""
    rerr, rv2c, rc2v = ref
    rc, errors, v2c, c2v = got
    assert rc == 0
    assert np.array_equal(errors[:T + 1], rerr), (errors[:T + 1].tolist(), rerr.tolist())
    assert errors[T + 1] == F.PAD_ERRORS and v2c[M] == F.PAD and c2v[M] == F.PAD
    assert_bit_exact(c2v[:M], rc2v)
    if T == 0:
        assert (v2c == F.PAD).all()                          # not written
        assert not np.signbit(c2v[:M]).any()                 # all +0.0
    else:
        assert_bit_exact(v2c[:M], rv2c)


# ------------------------------------------------------------------ A: the (3, 6) ensemble
@pytest.mark.parametrize("T", F.A_ITERS)
@pytest.mark.parametrize("M", F.A_SIZES)
def test_a_regular_ensemble(gpu, M, T):
    u, tables = F.a_inputs()
    check_against(F.at(F.a_ref(M), T), run_raw(u, tables, M, T, F.A_SEED), M, T)


# ------------------------------------------------------------------ B: divergent degrees inside one wave
@pytest.mark.parametrize("high_rate", [False, True], ids=["mixed", "high_rate"])
def test_b_divergent_degrees(gpu, high_rate):
    u, tables = F.b_inputs(high_rate)
    check_against(F.at(F.b_ref(high_rate), F.B_T), run_raw(u, tables, F.B_M, F.B_T, F.B_SEED), F.B_M, F.B_T)


# ------------------------------------------------------------------ C: special values
def test_c_special_values(gpu):
    u, tables, _ = F.c_inputs()
    for T in range(F.C_T + 1):                               # the first iterations too: where a -0.0 is still one
        check_against(F.at(F.c_ref(), T), run_raw(u, tables, F.C_M, T, F.C_SEED), F.C_M, T)


# ------------------------------------------------------------------ D: the signed population of a batch
@functools.lru_cache(None)
def d_batch(B):
    """An llr_source batch at 4-PAM 4.0 dB, S = 64, with NaN LAPPRs and a sentinel bit written over the padding
    columns -> (lappr [128, ld], word [128, ld]) on the GPU."""
    import qamr
    import torch
    from qamr import sim
    from qamr.pipeline import alternating_config

    pa = qamr.PAMAlphabet(2, 2)
    two_var = pa.variance * 10 ** (-0.4)
    nm = qamr.NoiseMapper(pa, two_var / 2, alternating_config(pa.order))
    lappr, word = sim.llr_source(nm, pa, 64, B, torch.Generator(device="cuda").manual_seed(31 + B))
    lappr[:, B:] = math.nan
    word[:, B:] = 255
    torch.cuda.synchronize()
    return lappr, word


@pytest.mark.parametrize("alpha", [1.0, 0.7])
@pytest.mark.parametrize("B", [1, 8, 65])
def test_d_signed_population(gpu, B, alpha):
    import torch
    from qamr.density_evolution import evolve_device, signed_population

    lappr, word = d_batch(B)
    rows, ld = lappr.shape
    assert rows == 128 and ld == (64 if B < 65 else 128)
    out = torch.full((rows * B + 1,), F.PAD, dtype=torch.float64, device="cuda")
    u = signed_population(lappr, word, B, alpha, out=out[:rows * B])
    torch.cuda.synchronize()
    want = F.signed_population(lappr[:, :B].cpu().numpy(), word[:, :B].cpu().numpy(), alpha)
    got = u.cpu().numpy()
    assert np.array_equal(got.view(np.int64), want.view(np.int64)) and not np.isnan(got).any()
    assert float(out[rows * B]) == F.PAD
    if B == 65:                                              # 8 320 LAPPRs: a few per cent of them point the wrong way
        assert 0 < (got < 0).sum() < got.size // 4
    assert torch.equal(signed_population(lappr, word, B, alpha), u)
    tables = make_tables(F.regular_tables())
    r = evolve_device(u, tables, F.D_M, F.D_T, F.D_SEED)
    rerr, rv2c, rc2v = F.at(F.evolve(want, *F.regular_tables(), F.D_M, F.D_T, F.D_SEED), F.D_T)
    assert r.errors.dtype == torch.int64 and np.array_equal(r.errors.cpu().numpy(), rerr)
    assert_bit_exact(r.v2c.cpu().numpy(), rv2c)
    assert_bit_exact(r.c2v.cpu().numpy(), rc2v)
    assert r.error_rate().tolist() == [e / F.D_M for e in rerr.tolist()]


# ------------------------------------------------------------------ E: refusals
def test_e_refusals(gpu):
    """Every bound and a null pointer: QR_EVALUE before any launch, the outputs still hold their sentinels and
    no de_* launch is counted."""
    import torch

    from qamr import _lib
    from qamr._lib import dptr

    lib = _lib.load()
    tables = make_tables(F.regular_tables())
    u = torch.zeros(8, dtype=torch.float64, device="cuda")
    M, T = 16, 2
    v2c = torch.full((M,), F.PAD, dtype=torch.float64, device="cuda")
    c2v = torch.full((M,), F.PAD, dtype=torch.float64, device="cuda")
    errors = torch.full((T + 1,), F.PAD_ERRORS, dtype=torch.int64, device="cuda")
    L = torch.zeros((4, 64), dtype=torch.float64, device="cuda")
    w = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    pop = torch.full((4 * 3,), F.PAD, dtype=torch.float64, device="cuda")
    ok = dict(tables=tables.handle, Mu=8, u=dptr(u), M=M, T=T, v2c=dptr(v2c), c2v=dptr(c2v), errors=dptr(errors))
    bad = [dict(Mu=0), dict(Mu=-1), dict(Mu=1 << 31), dict(M=0), dict(M=(1 << 30) + 1), dict(T=-1), dict(T=10001),
           dict(tables=None), dict(u=None), dict(v2c=None), dict(c2v=None), dict(errors=None)]
    okp = dict(B=3, ld=64, rows=4, lappr=dptr(L), word=dptr(w), alpha=1.0, u=dptr(pop))
    badp = [dict(B=0), dict(B=65), dict(ld=96), dict(rows=0), dict(rows=1 << 30), dict(alpha=math.nan), dict(alpha=math.inf),
            dict(lappr=None), dict(word=None), dict(u=None)]
    with DF.profiled():
        for spoil in bad:
            a = dict(ok, **spoil)
            rc = lib.qr_de_evolve_device(a["tables"], a["Mu"], a["u"], a["M"], a["T"], 5, a["v2c"], a["c2v"], a["errors"], None)
            assert rc == _lib.QR_EVALUE and _lib.last_error(), spoil
        for spoil in badp:
            a = dict(okp, **spoil)
            rc = lib.qr_de_population_device(a["B"], a["ld"], a["rows"], a["lappr"], a["word"], a["alpha"], a["u"], None)
            assert rc == _lib.QR_EVALUE and _lib.last_error(), spoil
        torch.cuda.synchronize()
        for name in SCOPES:
            assert _lib.profile_query(name)[1] == 0, name
    assert bool((v2c == F.PAD).all()) and bool((c2v == F.PAD).all()) and bool((errors == F.PAD_ERRORS).all())
    assert bool((pop == F.PAD).all())
    # table creation: a check degree of 1, a degree of 256
    for ev, ec, nv in (([3], [1], [3]), ([256], [6], [3]), ([3], [256], [3]), ([3], [6], [256])):
        h = C.c_void_p()
        a = [np.array(x, np.int32) for x in (ev, ec, nv)]
        assert lib.qr_de_tables_create(0, 1, _lib.ptr(a[0]), _lib.ptr(a[1]), 1, _lib.ptr(a[2]), C.byref(h)) == _lib.QR_EVALUE
        assert not h.value
    h = C.c_void_p()
    a = np.array([3], np.int32)
    assert lib.qr_de_tables_create(99, 1, _lib.ptr(a), _lib.ptr(a), 1, _lib.ptr(a), C.byref(h)) == _lib.QR_EVALUE   # no such device


# ------------------------------------------------------------------ F: asynchronous, capturable, deterministic
def test_f_asynchronous_and_graph_capture(gpu):
    """The call returns while the stream is still busy with the work queued before it, and a torch.cuda.graph
    capture of it, replayed on a refilled u, gives the eager result."""
    import torch
    from qamr.density_evolution import evolve_device

    u0, tables = F.a_inputs()
    u1 = F.biawgn(0.80, 1000, 55)
    M, T = 4096, 2
    t = make_tables(tables)
    ut = torch.from_numpy(np.array(u0)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        evolve_device(ut, t, M, T, F.A_SEED, stream=s)       # eager: the code objects are loaded
        torch.cuda.synchronize()
        torch.cuda._sleep(100_000_000)                       # the GPU spins for tens of milliseconds ahead of the call
        r = evolve_device(ut, t, M, T, F.A_SEED, stream=s)
        end = torch.cuda.Event()
        end.record(s)
        pending = not end.query()
    torch.cuda.synchronize()
    assert pending, "evolve_device waited for the GPU"
    rerr, rv2c, rc2v = F.at(F.a_ref(M), T)
    assert np.array_equal(r.errors.cpu().numpy(), rerr)
    assert_bit_exact(r.c2v.cpu().numpy(), rc2v)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r = evolve_device(ut, t, M, T, F.A_SEED)
    ut.copy_(torch.from_numpy(np.array(u1)).cuda())
    r.errors.fill_(F.PAD_ERRORS)
    r.v2c.fill_(F.PAD)
    r.c2v.fill_(F.PAD)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    eager = evolve_device(ut, t, M, T, F.A_SEED)
    torch.cuda.synchronize()
    assert torch.equal(r.errors, eager.errors) and not torch.equal(r.errors.cpu(), torch.from_numpy(np.array(rerr)))
    assert torch.equal(r.v2c.view(torch.int64), eager.v2c.view(torch.int64))
    assert torch.equal(r.c2v.view(torch.int64), eager.c2v.view(torch.int64))
    ref1 = F.at(F.evolve(u1, *tables, M, T, F.A_SEED), T)
    assert np.array_equal(r.errors.cpu().numpy(), ref1[0])
    assert_bit_exact(r.v2c.cpu().numpy(), ref1[1])
    assert_bit_exact(r.c2v.cpu().numpy(), ref1[2])


def test_f_deterministic_and_seeded(gpu):
    u, tables = F.a_inputs()
    t = make_tables(tables)
    a = run_raw(u, tables, 4096, 8, F.A_SEED, t)
    b = run_raw(u, tables, 4096, 8, F.A_SEED, t)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    c = run_raw(u, tables, 4096, 8, F.A_SEED + 1, t)
    assert c[0] == 0 and not np.array_equal(a[1], c[1])


@pytest.mark.parametrize("T", [0, 1, 5])
def test_f_launch_counts(gpu, T):
    """1 + 3T launches: T variable phases, T check phases, T + 1 decisions; one launch per population."""
    import torch

    from qamr import _lib
    from qamr.density_evolution import evolve_device, signed_population

    u, tables = F.a_inputs()
    t = make_tables(tables)
    ut = torch.from_numpy(np.array(u)).cuda()
    L = torch.ones((4, 64), dtype=torch.float64, device="cuda")
    w = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    with DF.profiled():
        evolve_device(ut, t, 64, T, 0)
        signed_population(L, w, 3)
        torch.cuda.synchronize()
        n = {name: _lib.profile_query(name)[1] for name in SCOPES}
    assert n == dict(de_population=1, de_var=T, de_check=T, de_post=T + 1) and sum(n.values()) - 1 == 1 + 3 * T


def test_host_entry_equals_the_restatement(gpu):
    from qamr.density_evolution import evolve

    u, tables = F.b_inputs()
    r = evolve(u, tables, F.B_M, F.B_T, F.B_SEED)
    rerr, rv2c, rc2v = F.at(F.b_ref(), F.B_T)
    assert isinstance(r.errors, np.ndarray) and r.errors.dtype == np.int64 and np.array_equal(r.errors, rerr)
    assert_bit_exact(r.v2c, rv2c)
    assert_bit_exact(r.c2v, rc2v)
    r0 = evolve(u, tables, F.B_M, 0, F.B_SEED)
    assert r0.v2c is None and not r0.c2v.any() and not np.signbit(r0.c2v).any() and np.array_equal(r0.errors, rerr[:1])
    assert r0.first_zero() is None or r0.errors[0] == 0


def test_cli(gpu, tmp_path):
    """The N = 1008 code, two points, two scales: the header, one row per (point, alpha), the same file for the
    same seed, and every row what evolve_device gives on the same seeded frames."""
    import qamr
    import torch
    from qamr import codes, sim, sim_density_evolution as cli
    from qamr.density_evolution import degree_tables, evolve_device, signed_population
    from qamr.pipeline import alternating_config
    from qamr.sim_lappr_information import point_seed

    vid, cid = codes.regular_code(1008, 3, 6, 0)
    edgefile = str(tmp_path / "reg1008.csv")
    codes.save_edge_csv(edgefile, vid, cid)
    argv = [edgefile] + "--snr 3 4 --nsnr 2 --alphas 0.7 1.0 --iterations 8 --population 4096 --frames 8 --seed 3".split()
    outs = [str(tmp_path / f"o{i}.csv") for i in range(2)]
    for o in outs:
        cli.main(argv + ["--out", o])
    txt = open(outs[0]).read()
    assert txt == open(outs[1]).read()
    lines = txt.splitlines()
    assert lines[0] == cli.HEADER and len(lines) == 1 + 2 * 2
    pa = qamr.PAMAlphabet(2, 2)
    tables = make_tables(degree_tables(vid, cid))
    row = 1
    for i, snr in enumerate((3.0, 4.0)):
        two_var = pa.variance * (10 ** (-snr / 10))
        nm = qamr.NoiseMapper(pa, two_var / 2, alternating_config(pa.order))
        gen = torch.Generator(device="cuda").manual_seed(point_seed(3, i))
        lappr, word = sim.llr_source(nm, pa, 504, 8, gen)
        for alpha in (0.7, 1.0):
            r = evolve_device(signed_population(lappr, word, 8, alpha), tables, 4096, 8, 3)
            assert lines[row] == cli.format_row(cli.row(snr, alpha, r)), (row, lines[row])
            row += 1


# ------------------------------------------------------------------ G: the (3, 6) threshold
@functools.lru_cache(None)
def g_run(sigma):
    import torch
    from qamr.density_evolution import evolve_device

    u = torch.from_numpy(np.array(F.biawgn(sigma, 1 << 18, 7))).cuda()
    r = evolve_device(u, make_tables(F.regular_tables()), 1 << 16, 100, 7)
    return r, r.errors.cpu().numpy()


def test_g_below_the_threshold_converges(gpu):
    """sigma = 0.84 < sigma* = 0.8809 (Richardson-Urbanke): no error left within 40 iterations (a float sketch of
    the definition at M = 2^17 reached 0 at iteration 17)."""
    r, errors = g_run(0.84)
    print("sigma 0.84: first zero", r.first_zero(), "errors", errors[:24].tolist())
    assert r.first_zero() is not None and r.first_zero() <= 40


def test_g_above_the_threshold_stalls(gpu):
    """sigma = 0.92 > sigma*: the error rate never falls below 0.05 in 100 iterations (the sketch: 0.087)."""
    r, errors = g_run(0.92)
    print("sigma 0.92: min rate", errors.min() / (1 << 16))
    assert errors.min() / (1 << 16) >= 0.05 and r.first_zero() is None
