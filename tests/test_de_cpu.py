"""CPU-side checks of the sampled density evolution (DESIGN.md "Density evolution"): the random indices' known
answers, the degree tables of the project's codes, the exported entries, the refusals that precede any device
call, the built kernels, the CLI's arguments, and the conditions of the GPU cases from the restatement alone
(tests/de_fixture.py)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import de_fixture as F
import few_fixture as FF

sys.path.insert(0, os.path.join(ROOT, "scripts"))

ENTRIES = ("qr_de_tables_create", "qr_de_tables_destroy", "qr_de_population_device", "qr_de_evolve_device",
           "qr_de_evolve_host")


# ------------------------------------------------------------------ random indices
def test_rnd_known_answers():
    import qamr.density_evolution as de

    assert [int(z) for z in F.z_of(0, np.arange(3, dtype=np.uint64))] == \
        [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]           # SplitMix64's first three
    for rnd in (F.rnd, de.rnd):
        assert [rnd(7, 1, 0, j, 2, 4096) for j in range(4)] == [1256, 864, 3515, 187]
        assert [rnd(0, 0, 2, j, 0, 1008) for j in range(3)] == [492, 756, 720]
    assert F.rnd_vec(7, 1, 0, np.arange(4), 2, 4096).tolist() == [1256, 864, 3515, 187]
    assert F.rnd_vec(0, 0, 2, np.arange(3), 0, 1008).tolist() == [492, 756, 720]


def test_rnd_vector_form_equals_the_integer_form():
    rng = np.random.default_rng(3)
    for seed, t, phase, k, n in ((0, 0, 0, 0, 1), ((1 << 64) - 1, 10000, 2, 256, (1 << 31) - 1), (12345, 77, 1, 255, 1 << 30),
                                 (1 << 63, 1, 0, 2, 1000)):
        j = np.concatenate([rng.integers(0, 1 << 30, 50), [0, (1 << 30) - 1]])
        want = [F.rnd(seed, t, phase, int(x), k, n) for x in j]
        assert F.rnd_vec(seed, t, phase, j, k, n).tolist() == want
        assert all(0 <= v < n for v in want)


# ------------------------------------------------------------------ degree tables
def test_degree_tables_hamming():
    from qamr import codes
    from qamr.density_evolution import degree_tables

    vid, cid = codes.load_edge_csv(os.path.join(GOLDEN, "hamming_7-4.csv"))
    ev, ec, nv = degree_tables(vid, cid)
    assert ev.dtype == ec.dtype == nv.dtype == np.int32
    assert nv.tolist() == [1, 1, 1, 2, 2, 2, 3]
    assert ec.tolist() == [4] * 12
    assert ev.tolist() == [1, 2, 2, 3, 1, 2, 2, 3, 1, 2, 2, 3]
    assert degree_tables(vid, cid, 9)[2].tolist() == [1, 1, 1, 2, 2, 2, 3, 0, 0]
    with pytest.raises(ValueError):
        degree_tables(vid, cid, 6)
    with pytest.raises(ValueError):
        degree_tables(vid, cid[:-1])


def test_degree_tables_regular_and_mixed():
    from qamr import codes
    from qamr.density_evolution import degree_tables

    ev, ec, nv = degree_tables(*codes.regular_code(1008, 3, 6, 0))
    assert ev.size == ec.size == 3024 and nv.size == 1008
    assert (ev == 3).all() and (ec == 6).all() and (nv == 3).all()
    vid, cid = FF.mixed_code()
    ev, ec, nv = degree_tables(vid, cid, FF.MIXED_V)
    assert nv.size == FF.MIXED_V and nv.sum() == vid.size == ev.size
    assert (nv[FF.mixed_isolated()] == 0).all() and nv.max() == FF.MIXED_HUB_DEGREE == 70
    assert int((ev == 70).sum()) == 70                      # the hub's edges, from the edge perspective
    for d in np.unique(ev):                                 # edges at variables of degree d: d per such variable
        assert int((ev == d).sum()) == d * int((nv == d).sum())
    cdeg = np.bincount(cid)
    for d in np.unique(ec):
        assert int((ec == d).sum()) == d * int((cdeg == d).sum())
    assert np.array_equal(ec, cdeg[cid]) and np.array_equal(ev, nv[vid])


# ------------------------------------------------------------------ entries
def test_symbols_and_signatures():
    from qamr import _lib

    L = _lib.load()
    for name in ENTRIES:
        assert hasattr(L, name) and name in _lib.SIGNATURES
    txt = open(os.path.join(ROOT, "include", "qamr.h")).read()
    assert "typedef struct qr_de_tables qr_de_tables;" in txt and "ctr(t, phase, j, k) = ((t*4 + phase) * 2^32 + j) * 512 + k" in txt


def test_reexported_by_the_reference_package_name():
    import qamr.density_evolution as de
    import qamreconciliation
    import qamreconciliation.density_evolution as rde

    assert qamreconciliation.density_evolution is rde
    for name in ("degree_tables", "DETables", "signed_population", "evolve_device", "evolve"):
        assert getattr(rde, name) is getattr(de, name)


def _create(ev, ec, nv, Ne=None, Nv=None, out=True):
    from qamr import _lib

    ev, ec, nv = (None if a is None else np.ascontiguousarray(a, np.int32) for a in (ev, ec, nv))
    h = C.c_void_p()
    p = lambda a: None if a is None else _lib.ptr(a)   # noqa: E731
    rc = _lib.load().qr_de_tables_create(0, len(ev) if Ne is None else Ne, p(ev), p(ec), len(nv) if Nv is None else Nv, p(nv),
                                         C.byref(h) if out else None)
    return rc, h


BAD_TABLES = [dict(ec=[6, 1]), dict(ec=[6, 256]), dict(ec=[0, 6]), dict(ev=[3, 0]), dict(ev=[256, 3]), dict(ev=[3, -1]),
              dict(nv=[3, 256]), dict(nv=[-1, 3]), dict(Ne=0), dict(Ne=1 << 31), dict(Nv=0), dict(Nv=1 << 31), dict(Ne=-1)]


@pytest.mark.parametrize("spoil", BAD_TABLES, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_tables_create_refuses_on_the_host(spoil):
    """Every degree and size is validated before any device call: QR_EVALUE without a GPU too."""
    from qamr import _lib

    a = dict(ev=[3, 3], ec=[6, 6], nv=[3, 0])
    a.update(spoil)
    rc, h = _create(**a)
    assert rc == _lib.QR_EVALUE and not h.value and _lib.last_error()


def test_tables_create_refuses_null_pointers():
    from qamr import _lib

    for a in (dict(ev=None, Ne=2), dict(ec=None), dict(nv=None, Nv=2), dict(out=False)):
        kw = dict(ev=[3, 3], ec=[6, 6], nv=[3, 0])
        kw.update(a)
        assert _create(**kw)[0] == _lib.QR_EVALUE
    assert _lib.load().qr_de_tables_destroy(None) == 0


def test_device_entries_refuse_before_the_device():
    """The bounds and null pointers of qr_de_population_device and qr_de_evolve_device over host buffers (never
    launched: every call fails a check first) leave the outputs alone."""
    from qamr import _lib

    lib, vp = _lib.load(), C.c_void_p
    L, w, u = np.zeros(2 * 64), np.zeros(2 * 64, np.uint8), np.full(2 * 3, F.PAD)
    ok = dict(B=3, ld=64, rows=2, lappr=L.ctypes.data, word=w.ctypes.data, alpha=1.0, u=u.ctypes.data)
    for spoil in (dict(B=0), dict(B=65), dict(ld=96), dict(ld=0), dict(rows=0), dict(rows=(1 << 31) // 3 + 1), dict(alpha=math.nan),
                  dict(alpha=math.inf), dict(alpha=-math.inf), dict(lappr=None), dict(word=None), dict(u=None)):
        a = dict(ok, **spoil)
        assert lib.qr_de_population_device(a["B"], a["ld"], a["rows"], vp(a["lappr"]), vp(a["word"]), a["alpha"], vp(a["u"]),
                                           None) == _lib.QR_EVALUE, spoil
    assert (u == F.PAD).all()
    # a null tables handle with everything else valid; the other bounds need a handle (the GPU test)
    v2c, c2v, err = np.full(4, F.PAD), np.full(4, F.PAD), np.full(3, F.PAD_ERRORS, np.int64)
    assert lib.qr_de_evolve_device(None, 6, vp(u.ctypes.data), 4, 2, 0, vp(v2c.ctypes.data), vp(c2v.ctypes.data),
                                   vp(err.ctypes.data), None) == _lib.QR_EVALUE
    ev = np.array([3], np.int32)
    for Mu, M, T in ((0, 4, 2), (1 << 31, 4, 2), (6, 0, 2), (6, (1 << 30) + 1, 2), (6, 4, -1), (6, 4, 10001)):
        assert lib.qr_de_evolve_host(0, 1, _lib.ptr(ev), _lib.ptr(ev * 2), 1, _lib.ptr(ev), Mu, _lib.ptr(u), M, T, 0,
                                     _lib.ptr(v2c), _lib.ptr(c2v), _lib.ptr(err)) == _lib.QR_EVALUE, (Mu, M, T)
    assert (v2c == F.PAD).all() and (c2v == F.PAD).all() and (err == F.PAD_ERRORS).all()


def test_python_entries_raise_value_error_before_the_device():
    import torch

    from qamr.density_evolution import DETables, evolve, evolve_device, signed_population

    t3 = ([3, 3], [6, 6], [3, 0])
    for tables in (([3], [6, 6], [3]), ([3.0], [6], [3]), ([], [], [3]), ([3], [1], [3]), ([256], [6], [3]), ([3], [6], [-1]),
                   ([[3]], [[6]], [3])):
        with pytest.raises(ValueError):
            DETables(*tables)
    u = np.zeros(5)
    for args in ((u, t3, 0, 1, 0), (u, t3, (1 << 30) + 1, 1, 0), (u, t3, 4, -1, 0), (u, t3, 4, 10001, 0), (u, t3, 4, 1, -1),
                 (u, t3, 4, 1, 1 << 64), (u, t3, 4.5, 1, 0), (u[:0], t3, 4, 1, 0), (u.astype(np.float32), t3, 4, 1, 0),
                 (u, ([3], [6, 6], [3]), 4, 1, 0), (u, ([3], [1], [3]), 4, 1, 0)):
        with pytest.raises(ValueError):
            evolve(*args)
    with pytest.raises(ValueError):
        evolve_device(torch.zeros(5, dtype=torch.float64), t3, 4, 1, 0)       # not a DETables
    Lt, wt = torch.zeros((8, 64), dtype=torch.float64), torch.zeros((8, 64), dtype=torch.uint8)
    for args, kw in (((Lt, wt, 0), {}), ((Lt, wt, 65), {}), ((Lt[:, :60], wt[:, :60], 1), {}), ((Lt, wt, 1), dict(alpha=math.nan)),
                     ((Lt, wt, 1), dict(alpha=math.inf)), ((Lt.float(), wt, 1), {}), ((np.zeros((8, 64)), wt, 1), {}),
                     ((Lt, wt, 1), {})):   # the last: host tensors
        with pytest.raises(ValueError):
            signed_population(*args, **kw)


# ------------------------------------------------------------------ the built code object
def test_kernels_in_code_object_without_scratch():
    import kernel_resources as K
    from qamr import _lib

    ks = K.kernels(_lib.LIB_PATH)
    dm = K.demangle([k.removesuffix(".kd") for k in ks])
    got = {dm[k.removesuffix(".kd")]: v for k, v in ks.items() if "qr::k_de_" in dm[k.removesuffix(".kd")]}
    want = ["qr::k_de_check(qr::DeArgs)", "qr::k_de_population(int, int, long, double const*, unsigned char const*, double, double*)",
            "void qr::k_de_post<false>(qr::DeArgs)", "void qr::k_de_post<true>(qr::DeArgs)",
            "void qr::k_de_var<false>(qr::DeArgs)", "void qr::k_de_var<true>(qr::DeArgs)"]
    assert sorted(got) == want, sorted(got)
    for name, r in got.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)


# ------------------------------------------------------------------ CLI
def test_cli_parser_and_argument_checks():
    from qamr import sim_density_evolution as cli

    a = cli.build_parser().parse_args(["code.csv"])
    assert (a.edgefile, a.mode, a.demapper, a.alphas, a.iterations, a.population, a.frames, a.seed, a.out) == \
        ("code.csv", "softening", "search", [1.0], 50, 1 << 20, 64, 0, "de.csv") and not a.configuration_base
    a = cli.build_parser().parse_args("code.csv --bps 2 --snr 3 4 --nsnr 5 --alphas 0.7 1.0 --iterations 50 --population 1048576 "
                                      "--frames 64 --seed 0 --demapper simplified --mode direct --out de.csv".split())
    assert (a.bps, a.snr, a.nsnr, a.alphas, a.iterations, a.population, a.frames, a.demapper, a.mode) == \
        (2, [3.0, 4.0], 5, [0.7, 1.0], 50, 1048576, 64, "simplified", "direct")
    cli.check_args(a)
    for bad in ("--nsnr 0", "--frames 0", "--alphas nan", "--iterations -1", "--iterations 10001", "--population 0",
                "--population 1073741825", "--seed -1"):
        with pytest.raises(SystemExit):
            cli.check_args(cli.build_parser().parse_args(["code.csv"] + bad.split()))
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args([])                   # the code is required
    assert cli.HEADER == "EsN0dB,alpha,final,best,first_zero"
    assert cli.format_row((3.5, 0.7, 0.25, 0.125, None)) == "3.5,0.7,0.25,0.125,"
    assert cli.format_row((4.0, 1.0, 0.0, 0.0, 17)) == "4.0,1.0,0.0,0.0,17"


def test_result_helpers():
    from qamr.density_evolution import DEResult

    r = DEResult(np.array([5, 2, 0, 0], np.int64), None, np.zeros(8), 8)
    assert r.first_zero() == 2 and r.error_rate().tolist() == [0.625, 0.25, 0.0, 0.0]
    assert DEResult(np.array([5, 2], np.int64), None, np.zeros(8), 8).first_zero() is None


# ------------------------------------------------------------------ the conditions of the GPU cases
def test_case_a_conditions():
    """(3, 6) at sigma = 0.80, below the threshold 0.8809: the error count falls over the 8 iterations and is not
    yet 0 at t = 2, so an evolution that stops early, repeats an iteration or reads a stale population shows."""
    u, (ev, ec, nv) = F.a_inputs()
    assert u.size == 1000 and (ev == 3).all() and (ec == 6).all() and (nv == 3).all()
    errors, v2c, c2v = F.a_ref(4096)
    print("case A errors at M = 4096:", errors.tolist())
    assert errors.size == 9 and errors[8] < errors[2] < errors[0] and errors[2] > 0
    assert 0.05 < errors[0] / 4096 < 0.15                   # the raw error rate Q(1 / 0.8) = 0.106
    assert v2c[0] is None and not c2v[0].any() and not np.signbit(c2v[0]).any()
    for M in F.A_SIZES:                                      # each size is its own evolution
        e, _, c = F.a_ref(M)
        assert e.size == 9 and all(a.size == M for a in c)
    # M = 1: every message index is 0, so v2c(t)[0] = u + 2 c2v(t-1)[0]
    e, v, c = F.a_ref(1)
    assert all(F.rnd(F.A_SEED, t, 0, 0, 2 + k, 1) == 0 for t in (1, 2) for k in (0, 1))


def test_case_b_conditions():
    u, (ev, ec, nv) = F.b_inputs()
    assert set(ev.tolist()) == set(F.B_VDEG) and set(ec.tolist()) == set(F.B_CDEG) and set(nv.tolist()) == set(F.B_NDEG)
    # the degrees drawn inside the first wave differ: it runs to its largest trip count
    J = np.arange(64, dtype=np.uint64)
    for phase, table in ((0, ev), (1, ec)):
        d = table[F.rnd_vec(F.B_SEED, 1, phase, J, 0, table.size)]
        assert d.min() <= 2 and d.max() == 255 and np.unique(d).size >= 4
    errors, v2c, c2v = F.b_ref()
    assert errors.size == F.B_T + 1 and np.isfinite(c2v[F.B_T]).all()
    u, (ev, ec, nv) = F.b_inputs(True)
    assert set(ec.tolist()) == set(F.B_HIGH_RATE_CDEG)
    assert np.isfinite(F.b_ref(True)[2][F.B_T]).all()


def test_case_c_conditions():
    """The planted specials reach the populations: NaN and inf messages, a -0.0 that a degree-1 variable handed
    on untouched, and finite messages beside them."""
    u, (ev, ec, nv), n = F.c_inputs()
    assert np.isnan(u).sum() >= 2 and np.isinf(u).sum() >= 4 and (u == 0).sum() >= 4 and 0 < (np.abs(u[u != 0]) < 1e-300).sum()
    assert set(ev.tolist()) == {1, 2, 3} and set(ec.tolist()) == {2, 3, 6} and set(nv.tolist()) == {0, 1, 3}
    errors, v2c, c2v = F.c_ref()
    first = v2c[1]
    assert np.signbit(first[first == 0]).any()              # -0.0 survives the first variable phase
    last = c2v[F.C_T]
    assert np.isnan(last).any() and np.isfinite(last).sum() >= 16
    assert np.isinf(v2c[1]).any() and np.isnan(v2c[F.C_T]).any()
    assert errors[0] > 0


def test_signed_population_restatement():
    L = np.array([[1.5, -2.0], [math.nan, -0.0], [math.inf, 5e-324]])
    w = np.array([[0, 1], [1, 1], [1, 0]], np.uint8)
    u = F.signed_population(L, w, 0.5)
    assert u[[0, 1]].tolist() == [0.75, 1.0] and math.isnan(u[2]) and u[3] == 0 and not np.signbit(u[3])
    assert u[4] == -math.inf and u[5] == 0.0               # 0.5 * 5e-324 rounds to +0.0 (ties to even)
