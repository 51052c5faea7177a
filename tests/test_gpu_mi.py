"""The Monte-Carlo mutual-information estimator on the GPU against tests/golden/mi.npz (written by
tests/golden/make_golden_mi.py from the reference's NoiseMapper / PAMAlphabet and the restated scalar
lines of mutual_information.pyx:245-297).  Every comparison is bit for bit (conftest.assert_bit_exact:
infinities compare as bits, NaN matches NaN)."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import assert_bit_exact, golden

from debug_rerun import rerun_on_debug_build
from mapper_fixture import expected_terms, mapper, mc_inputs, run_device

pytestmark = pytest.mark.gpu

CASES = list(range(1, 9))
B, S, LD = 70, 37, 128


@pytest.fixture(scope="module")
def fx():
    g = golden("mi.npz")
    assert int(g["n_cases"]) == 8 and int(g["B"]) == B and int(g["S"]) == S
    return g


def test_device_log2_vs_libm(gpu):
    """qr_log2_host (the device's g_log2_full) against math.log2 (libm's) on 1e5 inputs and the specials."""
    from qamr import _lib

    rng = np.random.default_rng(77)
    x = np.concatenate([
        2.0 ** rng.uniform(-60, 60, 40000), rng.uniform(0.95, 1.05, 30000), rng.uniform(0.5, 2.0, 20000),
        rng.integers(1, 1 << 52, 5000).astype(np.uint64).view(np.float64),          # subnormals
        rng.integers(0, 1 << 63, 5000).astype(np.uint64).view(np.float64),          # any positive pattern
        [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 2.0, 0.5, -1.0, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308,
         1.0 - float.fromhex("0x1.5b51p-5"), 1.0 + float.fromhex("0x1.6ab2p-5"), np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), -5e-324]])
    x = np.ascontiguousarray(x, np.float64)
    assert x.size >= 100000
    out = np.empty_like(x)
    _lib.check(_lib.load().qr_log2_host(x.size, _lib.ptr(x), _lib.ptr(out)), "log2")

    def ref(v):
        if v != v or v < 0:
            return math.nan
        if v == 0:
            return -math.inf
        return math.log2(v)

    assert_bit_exact(out, np.array([ref(float(v)) for v in x]))
    assert out[-17] == -np.inf and out[-16] == -np.inf and out[-15] == np.inf and np.isnan(out[-14]) and np.isnan(out[-13])


@pytest.mark.parametrize("c", CASES)
def test_device_blocks_vs_reference(gpu, fx, c):
    """The device entry at B = 70, ld = 128, S = 37 (two tiles, the second with 6 valid lanes): terms and
    totals equal the fixture's, the padding columns are not written, p_Xhat from the device's NoiseMapper
    equals the fixture's; then the same at B = 1, ld = 64."""
    from qamr.mutual_information import P_xhat, montecarlo_information_device, mutual_information_X_Xhat

    k = f"c{c}_"
    pa, nm = mapper(fx, k)
    pX = P_xhat(nm)
    assert_bit_exact(pX, fx[k + "p_Xhat"])
    assert_bit_exact(nm.fwrd_transition_probability, fx[k + "fwrd"])
    assert_bit_exact([mutual_information_X_Xhat(nm, pX)], [fx[k + "I_X_Xhat"]])
    x, y = mc_inputs(fx, k, LD)
    info, terms = run_device(nm, pX, x, y, B, LD)
    assert_bit_exact(terms[:, :, :B], expected_terms(fx, k))
    assert_bit_exact(info[:, :B], fx[k + "totals"].T)
    assert np.isnan(terms[:, :, B:]).all() and np.isnan(info[:, B:]).all()
    # without the terms (they live in the workspace) the totals are the same
    plain = montecarlo_information_device(nm, pX, x, y, B)
    assert tuple(plain.shape) == (3, B)
    assert_bit_exact(plain.cpu().numpy(), fx[k + "totals"].T)
    # one block, one tile
    x1, y1 = mc_inputs(fx, k, 64, 1)
    info1, terms1 = run_device(nm, pX, x1, y1, 1, 64)
    assert_bit_exact(terms1[:, :, :1], expected_terms(fx, k, 1))
    assert_bit_exact(info1[:, 0], fx[k + "totals"][0])
    assert np.isnan(terms1[:, :, 1:]).all() and np.isnan(info1[:, 1:]).all()


def test_which_masks(gpu, fx):
    """All 8 masks on case 5: a disabled quantity is exactly 0.0 / N and its term plane is not written,
    the enabled ones are unchanged."""
    from qamr.mutual_information import P_xhat

    k = "c5_"
    pa, nm = mapper(fx, k)
    pX = P_xhat(nm)
    x, y = mc_inputs(fx, k, LD)
    exp_t, exp_i = expected_terms(fx, k), fx[k + "totals"].T
    for mask in range(8):
        which = [(mask >> q) & 1 for q in range(3)]
        info, terms = run_device(nm, pX, x, y, B, LD, which)
        for q in range(3):
            if which[q]:
                assert_bit_exact(terms[q, :, :B], exp_t[q])
                assert_bit_exact(info[q, :B], exp_i[q])
            else:
                assert np.isnan(terms[q]).all()
                assert_bit_exact(info[q, :B], np.full(B, 0.0 / S))
                assert not np.signbit(info[q, :B]).any()
        assert np.isnan(info[:, B:]).all()


@pytest.mark.parametrize("c", [2, 4, 7])
def test_host_entry_and_montecarlo_information(gpu, fx, c):
    """qr_mi_montecarlo_host agrees with the device entry, and montecarlo_information under
    np.random.seed(5000 + 100 c + f) returns the fixture's totals of block f (the reference's draws)."""
    from qamr import _lib
    from qamr.mutual_information import P_xhat, montecarlo_information

    k = f"c{c}_"
    pa, nm = mapper(fx, k)
    pX = P_xhat(nm)
    for f in (0, 3, 69):
        np.random.seed(5000 + 100 * c + f)
        terms = np.full((3, S), np.nan)
        got = montecarlo_information(pa, nm, pX, S, _terms=terms)
        assert isinstance(got, tuple) and len(got) == 3 and all(isinstance(v, float) for v in got)
        assert_bit_exact(got, fx[k + "totals"][f])
        assert_bit_exact(terms, fx[k + "terms"][:, f, :])
    # which, through the host entry: disabled quantities are 0.0 / N
    np.random.seed(5000 + 100 * c)
    got = montecarlo_information(pa, nm, pX, S, np.array([0, 1, 0], np.uint8))
    assert_bit_exact(got, [0.0, fx[k + "totals"][0][1], 0.0])
    # the raw entry on stored inputs, N not a multiple of 64 and N > 64
    x = np.ascontiguousarray(fx[k + "x"][:3].astype(np.int64).ravel())
    y = np.ascontiguousarray(fx[k + "y"][:3].ravel())
    out, terms = np.empty(3), np.empty((3, x.size))
    _lib.check(_lib.load().qr_mi_montecarlo_host(nm.handle, x.size, _lib.ptr(x), _lib.ptr(y), None, _lib.ptr(out),
                                                 _lib.ptr(terms)))
    assert_bit_exact(terms, fx[k + "terms"][:, :3, :].reshape(3, -1))
    I = [0.0, 0.0, 0.0]
    for p in range(x.size):
        I[0] += terms[0, p]
        I[1] += terms[1, p]
        I[2] -= terms[2, p]
    assert_bit_exact(out, [v / x.size for v in I])


def test_out_of_range_symbol_is_nan_for_that_sample_only(gpu, fx):
    from qamr.mutual_information import P_xhat

    k = "c6_"
    pa, nm = mapper(fx, k)
    pX = P_xhat(nm)
    x, y = mc_inputs(fx, k, LD)
    x[2, 5] = nm.order
    x[36, 69] = -1
    info, terms = run_device(nm, pX, x, y, B, LD)
    want = expected_terms(fx, k).copy()
    want[:, 2, 5] = np.nan
    want[:, 36, 69] = np.nan
    assert_bit_exact(terms[:, :, :B], want)
    tot = fx[k + "totals"].T.copy()
    tot[:, 5] = np.nan
    tot[:, 69] = np.nan
    assert_bit_exact(info[:, :B], tot)


def test_launch_pair_is_capturable(gpu, fx):
    """After a warm-up call (grid and tables exist) the two launches allocate nothing and do not
    synchronise: they capture into a graph and the replay writes the same bits."""
    import torch
    from qamr.mutual_information import P_xhat, montecarlo_information_device

    k = "c5_"
    pa, nm = mapper(fx, k)
    pX = P_xhat(nm)
    x, y = mc_inputs(fx, k, LD)
    eager = montecarlo_information_device(nm, pX, x, y, B).cpu().numpy()   # warm-up
    torch.cuda.synchronize()
    info = torch.zeros((3, LD), dtype=torch.float64, device="cuda")
    terms = torch.zeros((3, S, LD), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        montecarlo_information_device(nm, pX, x, y, B, terms=terms, out=info)
    info.zero_()
    terms.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert_bit_exact(info.cpu().numpy()[:, :B], eager)
    assert_bit_exact(info.cpu().numpy()[:, :B], fx[k + "totals"].T)
    assert_bit_exact(terms.cpu().numpy()[:, :, :B], expected_terms(fx, k))


def test_device_entry_before_grid_or_tables_is_evalue(gpu):
    import torch
    import qamr
    from qamr import _lib

    nm = qamr.NoiseMapper(qamr.PAMAlphabet(2, 2.0), 0.5)   # __init__ builds neither grid nor MI tables
    x = torch.zeros((4, 64), dtype=torch.int64, device="cuda")
    y = torch.zeros((4, 64), dtype=torch.float64, device="cuda")
    info = torch.zeros((3, 64), dtype=torch.float64, device="cuda")
    terms = torch.zeros((3, 4, 64), dtype=torch.float64, device="cuda")
    L = _lib.load()

    def call(ws=None, ws_bytes=0, d_terms=terms, ld=64, Bq=64, Sq=4):
        return L.qr_mi_montecarlo_device(nm.handle, 7, Bq, ld, Sq, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                         C.c_void_p(info.data_ptr()),
                                         None if d_terms is None else C.c_void_p(d_terms.data_ptr()), ws, ws_bytes, None)

    assert call() == _lib.QR_EVALUE and "grid" in _lib.last_error()
    nm._device_grid()
    assert call() == _lib.QR_EVALUE and "qr_demap_mi_tables" in _lib.last_error()
    hx, hy, ho = np.zeros(4, np.int64), np.zeros(4), np.zeros(3)
    assert L.qr_mi_montecarlo_host(nm.handle, 4, _lib.ptr(hx), _lib.ptr(hy), None, _lib.ptr(ho), None) == _lib.QR_EVALUE
    pX = np.full(4, 0.25)
    _lib.check(L.qr_demap_mi_tables(nm.handle, _lib.ptr(pX), _lib.ptr(np.ascontiguousarray(nm.fwrd_transition_probability))))
    assert call() == _lib.QR_OK
    # the workspace in place of the terms: short, then exact
    need = C.c_size_t(0)
    assert L.qr_mi_workspace_size(64, 4, C.byref(need)) == 0 and need.value == 3 * 4 * 64 * 8
    assert call(C.c_void_p(terms.data_ptr()), need.value - 1, None) == _lib.QR_EVALUE and "workspace" in _lib.last_error()
    assert call(None, need.value, None) == _lib.QR_EVALUE
    assert call(C.c_void_p(terms.data_ptr()), need.value, None) == _lib.QR_OK
    # shapes and masks
    assert call(Sq=0) == _lib.QR_EVALUE and call(Bq=65) == _lib.QR_EVALUE and call(Bq=0) == _lib.QR_EVALUE
    assert L.qr_mi_montecarlo_device(nm.handle, 8, 64, 64, 4, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                     C.c_void_p(info.data_ptr()), C.c_void_p(terms.data_ptr()), None, 0, None) == _lib.QR_EVALUE
    torch.cuda.synchronize()
    # bps > 6: unsupported, like the batched formulation-1 demapper
    nm7 = qamr.NoiseMapper(qamr.PAMAlphabet(7, 2.0), 0.05, n_intervals_per_step=20)
    nm7._device_grid()
    p7 = np.full(128, 1 / 128)
    _lib.check(L.qr_demap_mi_tables(nm7.handle, _lib.ptr(p7), _lib.ptr(np.ascontiguousarray(nm7.fwrd_transition_probability))))
    rc = L.qr_mi_montecarlo_device(nm7.handle, 7, 64, 64, 4, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                   C.c_void_p(info.data_ptr()), C.c_void_p(terms.data_ptr()), None, 0, None)
    assert rc == _lib.QR_EUNSUPPORTED


def test_cli_small_run_is_reproducible(gpu, tmp_path):
    """2 SNR points x 4 blocks x 64 samples: the four columns with finite values, and the identical
    file twice under the same --seed."""
    from qamr.sim_montecarlo_information import main

    outs = []
    for name in ("a.csv", "b.csv"):
        path = str(tmp_path / name)
        rows = main(["--out", path, "--snr", "0", "10", "--nsnr", "2", "--bps", "2", "--niters", "4",
                     "--samples-per-iter", "64", "--seed", "5"])
        assert len(rows) == 2
        outs.append(open(path).read())
    assert outs[0] == outs[1]
    lines = outs[0].strip().split("\n")
    assert lines[0] == ",EsN0dB,I(X;Xhat),I(X;Y),I(N,X;Xhat)" and len(lines) == 3
    for i, ln in enumerate(lines[1:]):
        v = ln.split(",")
        assert int(v[0]) == i and len(v) == 5 and all(math.isfinite(float(t)) for t in v[1:])
    assert float(lines[1].split(",")[1]) == 0.0 and float(lines[2].split(",")[1]) == 10.0
    other = str(tmp_path / "c.csv")
    main(["--out", other, "--snr", "0", "10", "--nsnr", "2", "--bps", "2", "--niters", "4", "--samples-per-iter", "64",
          "--seed", "6"])
    assert open(other).read() != outs[0]


# ----------------------------------------------------------------- debug build
PARITY = ([f"test_device_blocks_vs_reference[{c}]" for c in CASES] + ["test_which_masks"] +
          [f"test_host_entry_and_montecarlo_information[{c}]" for c in (2, 4, 7)] +
          ["test_out_of_range_symbol_is_nan_for_that_sample_only"])


def test_debug_build_mi_index_checks(gpu):
    """This file's parity tests in a child process on libqamr_debug.so: the symbol, decision and grid
    index checks of k_mi_terms (mi.hip QR_DCHECK) never fail -- conftest's autouse fixture fails any
    test after which one did."""
    rerun_on_debug_build([f"tests/test_gpu_mi.py::{t}" for t in PARITY], len(PARITY), timeout=600)
