"""The table-interpolated g_inv and the formulation-1 demapper on the GPU against the reference's
own outputs (tests/golden/interp.npz, written by tests/golden/make_golden_interp.py from
NoiseMapper.y_range / F_Y_values / demap_noise / demap_lappr_simplified(_array) and Decoder.decode;
noisemapper.pyx:27-63, 135-144, 295-307, 391-403, 563-620).  Every comparison is bit for bit
(conftest.assert_bit_exact: infinities compare as bits, NaN matches NaN), with both bodies of the
grid index search (knob interp_fast 1 = coarse table + segment bisection, 0 = the reference's
__binsearch probe for probe) and across coarse-table segment sizes (knob interp_seg)."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_exact, golden

from debug_rerun import rerun_on_debug_build
from decode_fixture import knobs
from mapper_fixture import block_expected, mapper, sha, to_dev

pytestmark = pytest.mark.gpu

N_CASES = 11   # interp.npz "n_cases" (checked in test_interp_cpu.py)
WAVE_CASES = list(range(N_CASES))   # every fixture case has bps <= 6: the batched kernel serves it


@pytest.fixture(scope="module")
def fx():
    g = golden("interp.npz")
    assert int(g["n_cases"]) == N_CASES
    return g


def make_nm(g, c):
    """A new NoiseMapper in every test: knob interp_seg is read when its grid is built."""
    return mapper(g, f"c{c}_")[1]


# ----------------------------------------------------------------------- grid
@pytest.mark.parametrize("c", range(N_CASES))
def test_grid_matches_reference(gpu, fx, c):
    """qr_demap_grid_info / _host: n_points, end values and digests of y_range / F_Y_values are the
    reference's (noisemapper.pyx:135-144), and equal the y_range / F_Y_values properties."""
    nm = make_nm(fx, c)
    k = f"c{c}_"
    n, nondecreasing = nm.grid_info()
    assert n == int(fx[k + "n_points"])
    y, F = nm.grid_tables()
    assert y.size == n and F.size == n
    assert_bit_exact(y[[0, -1]], fx[k + "y_ends"])
    assert_bit_exact(F[[0, -1]], fx[k + "F_ends"])
    assert sha(y) == str(fx[k + "y_sha"])
    assert sha(F) == str(fx[k + "F_sha"])
    assert_bit_exact(y, nm.y_range)
    assert_bit_exact(F, nm.F_Y_values)
    # the generator saw no decrease in any of these tables; with the reference's bits neither does the device
    assert nondecreasing is True and not (np.diff(F) < 0).any()
    # a second creation with the same parameters changes nothing
    assert nm.grid_info() == (n, True)


# ---------------------------------------------------------------------- g_inv
@pytest.mark.parametrize("fast", [1, 0])
@pytest.mark.parametrize("c", range(N_CASES))
def test_g_inv_vs_reference(gpu, fx, c, fast):
    """NoiseMapper.demap_noise / g_inv (noisemapper.pyx:295-307, 391-403) on 300 seeded n_hat, the
    edge values (0, 1, 5e-324, 1 - 2^-53, 2^-53, 1e-300, -0.1, 1.1) and NaN, against every i."""
    nm = make_nm(fx, c)
    ref = fx[f"c{c}_ginv"]
    n = fx["n300"]
    M = nm.order
    assert ref.shape == (M, n.size)
    with knobs(interp_fast=fast):
        got = nm.demap_noise(np.tile(n, M), np.repeat(np.arange(M, dtype=np.int64), n.size))
        assert_bit_exact(got.reshape(M, n.size), ref)
        for i in (0, M - 1):
            for q in (0, 300, 301, 306, 308):   # a draw, 0, 1, -0.1, NaN
                assert_bit_exact([nm.g_inv(n[q], i)], [ref[i, q]])
        assert np.isnan(nm.demap_noise(np.array([0.5, 0.5]), np.array([-1, M], np.int64))).all()
    with pytest.raises(ValueError, match="Sizes do not match"):
        nm.demap_noise(np.zeros(3), np.zeros(2, np.int64))
    with pytest.raises(ValueError, match="Buffer dtype mismatch"):
        nm.demap_noise(np.zeros(3, np.float32), np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="Buffer dtype mismatch"):
        nm.demap_noise(np.zeros(3), np.zeros(3, np.int32))


# ---------------------------------------------------------- host formulation 1
@pytest.mark.parametrize("fast", [1, 0])
@pytest.mark.parametrize("c", range(N_CASES))
def test_host_formulation1_vs_reference(gpu, fx, c, fast):
    """demap_lappr_simplified_array and the scalar form (noisemapper.pyx:563-620) on 2000 seeded
    (n, j) plus the edge values; the high-SNR cases hold +-inf and NaN LAPPRs (underflowed sums)."""
    nm = make_nm(fx, c)
    k = f"c{c}_"
    n, j, ref = fx["n2000"], fx[k + "j2000"].astype(np.int64), fx[k + "la"]
    bps = nm.bit_per_symbol
    with knobs(interp_fast=fast):
        assert_bit_exact(nm.demap_lappr_simplified_array(n, j), ref)
        for s in (0, 7, 2001, 2006):
            assert_bit_exact(nm.demap_lappr_simplified(n[s], j[s]), ref[s * bps:(s + 1) * bps])
    if c == 7:
        assert np.isinf(ref).sum() > 1000   # the case exists to put exp's zeros and log(0) on the path
    with pytest.raises(ValueError, match="Sizes of transformed noise vector and tx symbols do not match"):
        nm.demap_lappr_simplified_array(np.zeros(3), np.zeros(2, np.int64))
    with pytest.raises(ValueError, match="Buffer dtype mismatch"):
        nm.demap_lappr_simplified_array(np.zeros(3, np.float32), np.zeros(3, np.int64))


# --------------------------------------------------------------- device block
@pytest.mark.parametrize("c", WAVE_CASES)
def test_device_block_vs_reference(gpu, fx, c):
    """demap_simplified_device on the [S=6][B=70] block at ld = 128: the decoder's layout, alpha as
    one fp64 multiply, untouched padding columns, NaN for an out-of-range j, a caller's `out`."""
    import torch

    nm = make_nm(fx, c)
    k = f"c{c}_"
    bps, S, B, ld = nm.bit_per_symbol, 6, 70, 128
    exp = block_expected(fx[k + "blk_la"], S, B, bps)
    n_fi = to_dev(fx[k + "blk_n"], ld, torch.float64)
    j_fi = to_dev(fx[k + "blk_j"].astype(np.int64), ld, torch.int64)
    for fast in (1, 0):
        with knobs(interp_fast=fast):
            for alpha in (1.0, 0.7):
                out = torch.full((S * bps, ld), float("nan"), dtype=torch.float64, device="cuda")
                ret = nm.demap_simplified_device(n_fi, j_fi, B, alpha, out=out)
                torch.cuda.synchronize()
                assert ret.data_ptr() == out.data_ptr()
                got = out.cpu().numpy()
                assert_bit_exact(got[:, :B], exp if alpha == 1.0 else exp * 0.7)
                assert np.isnan(got[:, B:]).all()
    # an out-of-range symbol index: NaN for that (symbol, frame) alone
    j_bad = j_fi.clone()
    j_bad[2, 5] = nm.order
    j_bad[4, 69] = -1
    got = nm.demap_simplified_device(n_fi, j_bad, B).cpu().numpy()[:, :B]
    want = exp.copy()
    want[2 * bps:3 * bps, 5] = np.nan
    want[4 * bps:5 * bps, 69] = np.nan
    assert_bit_exact(got, want)
    with pytest.raises(ValueError):
        nm.demap_simplified_device(n_fi, j_fi, B, out=torch.empty((S * bps, 64), dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("c", [5, 9])
def test_segment_size_knob_is_result_invariant(gpu, fx, c):
    """Knob interp_seg (log2 of the grid entries per coarse-table segment; the grid is rebuilt when
    it changes): 2-entry segments, the default's neighbours, segments longer than the whole
    288-point grid of case 9 (one coarse entry) and the clamped ends give the reference's bits."""
    import torch

    nm = make_nm(fx, c)
    k = f"c{c}_"
    bps, S, B, ld, M = nm.bit_per_symbol, 6, 70, 128, nm.order
    n300, ginv = fx["n300"], fx[k + "ginv"]
    exp = block_expected(fx[k + "blk_la"], S, B, bps)
    n_fi = to_dev(fx[k + "blk_n"], ld, torch.float64)
    j_fi = to_dev(fx[k + "blk_j"].astype(np.int64), ld, torch.int64)
    for seg in (1, 3, 6, 12, 0, 25):
        with knobs(dict(interp_seg=4), interp_seg=seg):
            got = nm.demap_noise(np.tile(n300, M), np.repeat(np.arange(M, dtype=np.int64), n300.size))
            assert_bit_exact(got.reshape(M, n300.size), ginv)
            assert_bit_exact(nm.demap_simplified_device(n_fi, j_fi, B).cpu().numpy()[:, :B], exp)
            assert nm.grid_info() == (int(fx[k + "n_points"]), True)


# ------------------------------------------------------------------ properties
@pytest.mark.parametrize("bps", [1, 2, 3, 4, 5, 6])
def test_device_kernel_matches_host_kernel(gpu, bps):
    """The 64-frame-tile kernel and the one-lane-per-symbol kernel agree bit for bit on a seeded
    [S=40][B=200] batch (ld = 256: a full tile, partial tiles, more than one workgroup), both
    index searches."""
    import torch
    import qamr

    pa = qamr.PAMAlphabet(bps, 2.0)
    nv = pa.variance * 10 ** (-(4.0 + 5.0 * bps) / 10) / 2
    cfg = np.zeros(pa.order, np.uint8)
    cfg[1::2] = 1
    nm = qamr.NoiseMapper(pa, nv, cfg)
    rng = np.random.default_rng(900 + bps)
    S, B, ld = 40, 200, 256
    n = rng.uniform(0, 1, (S, B))
    j = rng.integers(0, pa.order, (S, B)).astype(np.int64)
    n_fi, j_fi = to_dev(n, ld, torch.float64), to_dev(j, ld, torch.int64)
    res = []
    for fast in (1, 0):
        with knobs(interp_fast=fast):
            host = block_expected(nm.demap_lappr_simplified_array(n.ravel(), j.ravel()), S, B, bps)
            dev = nm.demap_simplified_device(n_fi, j_fi, B).cpu().numpy()[:, :B]
            assert_bit_exact(dev, host)
            res.append(host)
    assert_bit_exact(res[0], res[1])
    assert np.isfinite(res[0]).any()


def test_device_entry_before_grid_is_evalue(gpu):
    """qr_demap_simplified_batch_device on a demapper whose grid was never created: QR_EVALUE."""
    import torch
    import qamr
    from qamr import _lib

    nm = qamr.NoiseMapper(qamr.PAMAlphabet(2, 2.0), 0.5)   # __init__ builds no grid
    n = torch.zeros((4, 64), dtype=torch.float64, device="cuda")
    j = torch.zeros((4, 64), dtype=torch.int64, device="cuda")
    out = torch.zeros((8, 64), dtype=torch.float64, device="cuda")
    L = _lib.load()
    rc = L.qr_demap_simplified_batch_device(nm.handle, 64, 64, 4, C.c_void_p(n.data_ptr()), C.c_void_p(j.data_ptr()),
                                            1.0, C.c_void_p(out.data_ptr()), None)
    assert rc == _lib.QR_EVALUE
    assert "grid" in _lib.last_error()
    npts, nd = C.c_int32(0), C.c_int32(0)
    assert L.qr_demap_grid_info(nm.handle, C.byref(npts), C.byref(nd)) == _lib.QR_EVALUE
    with pytest.raises(ValueError):   # parameters the reference's formula cannot turn into a grid
        _lib.check(L.qr_demap_grid_create(nm.handle, 0.0, 1000, 2.0))
    # bps > 6: the batched kernel refuses, the host entry point serves it
    nm7 = qamr.NoiseMapper(qamr.PAMAlphabet(7, 2.0), 0.05, n_intervals_per_step=20)
    la = nm7.demap_lappr_simplified_array(np.array([0.25, 0.5]), np.array([3, 100], np.int64))
    assert la.shape == (14,) and not np.isnan(la).any()
    n7 = torch.zeros((1, 64), dtype=torch.float64, device="cuda")
    j7 = torch.zeros((1, 64), dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.QamrError):
        nm7.demap_simplified_device(n7, j7, 64)


# --------------------------------------------------------------------- capture
def test_demap_simplified_is_capturable(gpu, fx):
    """After a warm-up call (the grid exists), the launch makes no allocation and no host
    synchronisation: it captures into a graph and the replay writes the same bits."""
    import torch

    c = 5
    nm = make_nm(fx, c)
    bps, S, B, ld = nm.bit_per_symbol, 6, 70, 128
    n_fi = to_dev(fx[f"c{c}_blk_n"], ld, torch.float64)
    j_fi = to_dev(fx[f"c{c}_blk_j"].astype(np.int64), ld, torch.int64)
    eager = nm.demap_simplified_device(n_fi, j_fi, B, 0.7)   # warm-up: creates the grid
    torch.cuda.synchronize()
    out = torch.zeros((S * bps, ld), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        nm.demap_simplified_device(n_fi, j_fi, B, 0.7, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert_bit_exact(out.cpu().numpy()[:, :B], eager.cpu().numpy()[:, :B])
    assert_bit_exact(out.cpu().numpy()[:, :B], block_expected(fx[f"c{c}_blk_la"], S, B, bps) * 0.7)


# ------------------------------------------------------------------ end to end
def test_end_to_end_frames_vs_reference(gpu, fx):
    """The reference's softening pipeline with demap_lappr_simplified_array and Decoder.decode(..., 50)
    on 12 frames of the N = 1008 code (failures and early stops): LAPPRs, final LAPPRs, success and
    iterations through SofteningPipeline(demapper="simplified") equal the reference's."""
    import torch
    import qamr
    from qamr import codes
    from qamr.pipeline import Batch, SofteningPipeline

    vid, cid = codes.regular_code(1008)
    dec = qamr.Decoder(vid, cid)
    B = 12
    pipe = SofteningPipeline(dec, 2, 4.0, B, max_iterations=50, demapper="simplified")
    assert pipe.noise_var == float(fx["e2e_noise_var"])
    ld = pipe.ld
    x = to_dev(fx["e2e_x"].astype(np.int64).T, ld, torch.int64)
    nhat = to_dev(fx["e2e_nhat"].T, ld, torch.float64)
    synd = to_dev(np.unpackbits(fx["e2e_synd"], axis=1)[:, :504].T, ld, torch.uint8)
    word = to_dev(np.unpackbits(fx["e2e_word"], axis=1)[:, :1008].T, ld, torch.uint8)
    b = Batch(B, ld, x, nhat, word, synd)
    lappr = pipe.demap(b)
    assert_bit_exact(lappr.cpu().numpy()[:, :B].T, fx["e2e_lappr"])
    fin, succ, its = pipe.decode(lappr, b)
    torch.cuda.synchronize()
    assert list(zip(fx["e2e_success"].tolist(), fx["e2e_iters"].tolist()))[:4] == [(0, 50), (0, 50), (0, 50), (1, 11)]
    assert np.array_equal(succ.cpu().numpy()[:B], fx["e2e_success"])
    assert np.array_equal(its.cpu().numpy()[:B], fx["e2e_iters"])
    assert_bit_exact(fin.cpu().numpy()[:, :B].T, fx["e2e_final"])
    # the default pipeline still runs the search demapper
    ref_search = SofteningPipeline(dec, 2, 4.0, B, max_iterations=50)
    assert ref_search.demapper == "search"
    assert_bit_exact(ref_search.demap(b).cpu().numpy()[:, :B], pipe.nm.demap_device(nhat, x, B).cpu().numpy()[:, :B])


@pytest.mark.parametrize("demapper", ["simplified", "search"])
def test_simulator_demapper_keyword(gpu, demapper, monkeypatch):
    """Simulator(..., demapper=...).run_snr decodes the LAPPRs of the kernel the keyword names: the
    hook's LAPPRs equal that kernel's on the inputs the simulator gave its demapper, and the other
    kernel is never called."""
    import torch
    import qamr
    from qamr import codes
    from qamr.sim import Simulator

    calls = {"simplified": [], "search": []}
    orig_s, orig_d = qamr.NoiseMapper.demap_simplified_device, qamr.NoiseMapper.demap_device

    def rec_s(self, n, j, B, alpha=1.0, out=None, stream=None):
        calls["simplified"].append((n.clone(), j.clone(), B))
        return orig_s(self, n, j, B, alpha, out=out, stream=stream)

    def rec_d(self, n, j, B, alpha=1.0, out=None, stream=None):
        calls["search"].append((n.clone(), j.clone(), B))
        return orig_d(self, n, j, B, alpha, out=out, stream=stream)

    monkeypatch.setattr(qamr.NoiseMapper, "demap_simplified_device", rec_s)
    monkeypatch.setattr(qamr.NoiseMapper, "demap_device", rec_d)
    vid, cid = codes.regular_code(1008)
    dec = qamr.Decoder(vid, cid)
    sim = Simulator(dec, 2, "softening", max_iterations=10, batch=64, demapper=demapper)
    seen = []

    def hook(bidx, lappr, synd, word, B):
        torch.cuda.synchronize()
        seen.append(lappr[:, :B].cpu().numpy().copy())

    snr = 4.0
    res = sim.run_snr(snr, 64, 10 ** 9, seed=3, hook=hook)
    assert res[0] == snr and len(seen) == 1
    other = "search" if demapper == "simplified" else "simplified"
    assert len(calls[demapper]) == 1 and not calls[other]
    monkeypatch.undo()
    n, j, B = calls[demapper][0]
    nm = qamr.NoiseMapper(sim.pa, sim.pa.variance * (10 ** (-snr / 10)) / 2, sim.cfg)
    simplified = nm.demap_simplified_device(n, j, B).cpu().numpy()[:, :B]
    search = nm.demap_device(n, j, B).cpu().numpy()[:, :B]
    assert not np.array_equal(simplified, search)
    assert_bit_exact(seen[0], simplified if demapper == "simplified" else search)


def test_unknown_demapper_is_rejected(gpu):
    import qamr
    from qamr import codes
    from qamr.pipeline import SofteningPipeline
    from qamr.sim import Simulator, simulate_softening_snr_dB

    dec = qamr.Decoder(*codes.regular_code(1008))
    with pytest.raises(ValueError, match="demapper"):
        SofteningPipeline(dec, 2, 4.0, 64, demapper="sofisticated")
    with pytest.raises(ValueError, match="demapper"):
        Simulator(dec, 2, demapper="interp")
    with pytest.raises(ValueError, match="demapper"):
        simulate_softening_snr_dB(4.0, dec, 2, np.zeros(4, np.uint8), 5, 8, 100, demapper="fast")


# ----------------------------------------------------------------- debug build
# Grid shapes of the debug run: the smallest and the largest grids, the +-inf cases, the non-uniform
# alphabet, and the two n_intervals_per_step = 100 grids (288 and 1001 points: 5 and 16 coarse
# entries, a short last segment) -- the index checks depend on the shape, not on the values.
DEBUG_CASES = (0, 4, 7, 8, 9, 10)
PARITY = ([f"test_grid_matches_reference[{c}]" for c in DEBUG_CASES] +
          [f"test_g_inv_vs_reference[{c}-{f}]" for c in DEBUG_CASES for f in (1, 0)] +
          [f"test_host_formulation1_vs_reference[{c}-{f}]" for c in DEBUG_CASES for f in (1, 0)] +
          [f"test_device_block_vs_reference[{c}]" for c in DEBUG_CASES] +
          [f"test_device_kernel_matches_host_kernel[{b}]" for b in (1, 6)] +
          [f"test_segment_size_knob_is_result_invariant[{c}]" for c in (5, 9)])


def test_debug_build_interp_index_checks(gpu):
    """This file's parity tests in a child process on libqamr_debug.so: the grid index checks
    (0 <= r, r + 1 < n_points where pair r + 1 is read, the coarse-table index; grid_interp.hpp QR_DCHECK)
    never fail -- conftest's autouse fixture fails any test after which one did."""
    rerun_on_debug_build([f"tests/test_gpu_interp.py::{t}" for t in PARITY], len(PARITY), timeout=600)
