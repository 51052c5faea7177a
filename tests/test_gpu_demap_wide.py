"""GPU parity tests of the search demapper outside uniform 2..16-PAM at 0..40 dB, against the
reference's own outputs (tests/golden/demap_wide.npz, make_golden_demap_wide.py): shaped
probabilities, 32 / 64-PAM (k_demap_wave<5>, <6>; 64-PAM has no quantile table), 128 / 256-PAM
(k_demap<., 7>, <., 8>, launched by nothing else), -12 / -6 dB, and 80 / 85 dB, where
build_demap_host drops the Taylor table and Newton runs on the component sums.  Which regime of
the root search each case reaches is reported and asserted on the host by
tests/test_demap_replay.py::test_fast_search_bit_identical_wide.  Everything is bit for bit
(conftest.assert_bit_exact: infinities and the NaN pattern included)."""
import numpy as np
import pytest

from conftest import assert_bit_exact, golden

import oracle as O
from decode_fixture import knobs
from mapper_fixture import FIXTURE, block_expected, mapper

import make_golden_cases as MC

pytestmark = pytest.mark.gpu

N_CASES = len(MC.DEMAP_WIDE_CASES)
BASE_CASES = [c for c, case in enumerate(MC.DEMAP_WIDE_CASES) if case[4]]
LD, ALPHA, SENTINEL = 128, 0.75, -12345.678

# (demap_hyp, demap_fast) of qr_tune
SETTINGS = {"wave_private": (1, 1),   # k_demap_wave for bps <= 6; bps 7, 8 fall to k_demap<true, .>
            "per_symbol": (0, 1),     # k_demap<true, .>
            "brute_force": (1, 0)}    # k_demap<false, .>: the reference's loops verbatim


_NM = {}


def _nm(c, base):
    """The case's NoiseMapper (built once: its host tables cost more than the kernels here); base: with
    NoiseMapper's default sign configuration instead of the case's."""
    return mapper(golden("demap_wide.npz"), f"c{c}_", None if base else FIXTURE, cache=_NM)[1]


def _padded_block(n, j, M, ld):
    """[S][B] host blocks -> device tensors [S][ld] whose padding columns [B, ld) hold NaN and
    out-of-range symbol indices: the kernels must neither use nor write them."""
    import torch
    S, B = n.shape
    nt = np.full((S, ld), np.nan)
    jt = np.empty((S, ld), np.int64)
    jt[:] = np.resize(np.array([M, -1, 1 << 40, -(1 << 40)], np.int64), ld)
    nt[:, :B], jt[:, :B] = n, j
    dev = torch.device("cuda", 0)
    return torch.from_numpy(nt).to(dev), torch.from_numpy(jt).to(dev)


def _device_demap(nm, n, j, alpha, ld=LD):
    """demap_device on the ragged block into a sentinel-filled output; returns the columns
    [0, B) after asserting that the sentinel survives in [B, ld)."""
    import torch
    S, B = n.shape
    bps = nm.bit_per_symbol
    nt, jt = _padded_block(n, j, 1 << bps, ld)
    out = torch.full((S * bps, ld), SENTINEL, dtype=torch.float64, device=nt.device)
    nm.demap_device(nt, jt, B, alpha=alpha, out=out)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert_bit_exact(o[:, B:], np.full((S * bps, ld - B), SENTINEL))
    return o[:, :B]


@pytest.mark.parametrize("c", range(N_CASES))
def test_tables_and_host_entry_vs_reference(gpu, c):
    """F_Y_thresholds / delta_F_Y, and demap_lappr_array (k_demap at ld = 1)."""
    g = golden("demap_wide.npz")
    k = f"c{c}_"
    nm = _nm(c, False)
    assert_bit_exact(nm.F_Y_thresholds, g[k + "Fthr"])
    assert_bit_exact(nm.delta_F_Y, g[k + "dF"])
    n, j = g[k + "n"].ravel(), g[k + "j"].ravel().astype(np.int64)
    assert_bit_exact(nm.demap_lappr_array(n, j), g[k + "la"])
    if c in BASE_CASES:
        assert_bit_exact(_nm(c, True).demap_lappr_array(n, j), g[k + "base_la"])


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("c", range(N_CASES))
def test_device_entry_vs_reference(gpu, c, setting):
    """demap_device on a ragged two-tile batch (B = 70 or 8 of ld = 128), alpha = 0.75, through
    each of the three kernels; the padding columns are neither read (NaN, bad indices) nor
    written (qr_demap_batch_device's contract)."""
    g = golden("demap_wide.npz")
    k = f"c{c}_"
    nm = _nm(c, False)
    bps = nm.bit_per_symbol
    n, j = g[k + "n"], g[k + "j"].astype(np.int64)
    S, B = n.shape
    hyp, fast = SETTINGS[setting]
    with knobs(demap_hyp=hyp, demap_fast=fast):
        got = _device_demap(nm, n, j, ALPHA)
    assert_bit_exact(got, block_expected(g[k + "la"] * ALPHA, S, B, bps))


@pytest.mark.parametrize("c", range(N_CASES))
def test_root_search_vs_reference(gpu, c):
    """demap_noise_search at the default accuracy: the certified fast search and the loops."""
    g = golden("demap_wide.npz")
    k = f"c{c}_"
    di = g[k + "dns_i"].astype(np.int64)
    n = g[k + "n"].ravel()[:di.size].copy()
    for base in (False, True) if c in BASE_CASES else (False,):
        nm = _nm(c, base)
        ref = g[k + ("base_dns" if base else "dns")]
        for fast in (1, 0):
            with knobs(demap_fast=fast):
                got = nm.demap_noise_search(n, di)
            assert_bit_exact(got, ref)


@pytest.mark.parametrize("c", range(N_CASES))
def test_bob_side_at_thresholds_vs_reference(gpu, c):
    """k_bob / k_map_noise on every decision threshold and its nextafter neighbours, +-0.0 (a
    threshold for every M >= 2), every constellation point, the outer thresholds +-100 a_max,
    +-1e300 and +-inf."""
    import qamr
    g = golden("demap_wide.npz")
    k = f"c{c}_"
    nm = _nm(c, False)
    y, xh = g[k + "y_edge"], g[k + "xhat_edge"].astype(np.int64)
    assert np.array_equal(nm.hard_decide_index(y), xh)
    assert_bit_exact(nm.map_noise(y, xh), g[k + "nhat_edge"])
    xh2, nh2, word = nm._bob_host(y)
    assert np.array_equal(xh2, xh)
    assert_bit_exact(nh2, g[k + "nhat_edge"])
    pa = qamr.PAMAlphabet(nm.bit_per_symbol, 2.0)
    assert np.array_equal(word, pa.demap_symbols_to_bits(xh))
    if c in BASE_CASES:
        assert_bit_exact(_nm(c, True).map_noise(y, xh), g[k + "base_nhat_edge"])


@pytest.mark.parametrize("bps,snr", [(2, 4.0), (3, 9.5), (4, 13.0), (5, 20.0)])
def test_random_shaped_alphabet_vs_oracle(gpu, bps, snr):
    """A seeded random probability vector (in-order sum exactly 1.0, the rule of the fixture)
    and sign configuration: the wave-private demapper against the oracle, which
    tests/test_demap_wide_cpu.py pins on the reference for shaped and 32-PAM alphabets."""
    import qamr
    M = 1 << bps
    rng = np.random.default_rng(900 + bps)
    p = MC.exact_unit_sum(rng.dirichlet(np.full(M, 4.0)))
    assert MC.inorder_sum(p) == 1.0 and (p > 0).all()
    pa = qamr.PAMAlphabet(bps, 2.0, p)
    nv = pa.variance * 10 ** (-snr / 10) / 2
    cfg = rng.integers(0, 2, M).astype(np.uint8)
    nm = qamr.NoiseMapper(pa, nv, cfg)
    onm = O.OracleNoiseMapper(bps, 2.0, nv, cfg, p)
    assert_bit_exact(nm.F_Y_thresholds, onm.F_Y_thresholds)
    assert_bit_exact(nm.delta_F_Y, onm.delta_F_Y)
    S, B = 64, 70
    n = rng.random((S, B))
    n[0, :6] = [1e-300, 1 - 2.0 ** -53, 2.0 ** -53, 0.5, 0.0, 1.0]
    j = rng.integers(0, M, (S, B))
    got = _device_demap(nm, n, j, ALPHA)
    for f in (0, 63, 64, 69):
        ref = onm.demap_lappr_array(n[:, f].copy(), j[:, f].copy()) * ALPHA
        assert_bit_exact(got[:, f], ref)   # row s * bps + k
