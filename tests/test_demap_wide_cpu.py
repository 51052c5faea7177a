"""CPU tests: the oracle (C restatement) pinned on tests/golden/demap_wide.npz, the reference's
own outputs for the search demapper outside uniform 2..16-PAM at 0..40 dB: shaped
probabilities, 32..256-PAM, -12 / -6 dB and 80 / 85 dB (make_golden_demap_wide.py).  Tables,
LAPPRs, the root search and the Bob side at the decision thresholds, bit for bit: this is what
entitles tests/test_gpu_demap_wide.py to use the oracle for random shaped alphabets, and
tests/test_gpu_demap.py to use it for 32 / 64-PAM."""
import numpy as np
import pytest

from conftest import assert_bit_exact, golden

import oracle as O

import make_golden_cases as MC

N_CASES = len(MC.DEMAP_WIDE_CASES)
BASE_CASES = [c for c, case in enumerate(MC.DEMAP_WIDE_CASES) if case[4]]


def _onm(g, c, base=False):
    k = f"c{c}_"
    return O.OracleNoiseMapper(int(g[k + "bps"]), 2.0, float(g[k + "noise_var"]), None if base else g[k + "cfg"],
                               g[k + "probs"])


def test_fixture_matches_case_table():
    """The fixture holds the cases of make_golden_cases.DEMAP_WIDE_CASES, built by its rules:
    noise_var from the SNR, in-order probability sums of exactly 1.0, n in [0, 1]."""
    from qamr import PAMAlphabet

    g = golden("demap_wide.npz")
    assert int(g["n_cases"]) == N_CASES
    for c, (bps, snr, shape, symbols, has_base) in enumerate(MC.DEMAP_WIDE_CASES):
        k = f"c{c}_"
        M = 1 << bps
        p = g[k + "probs"]
        want = MC.demap_wide_probs(bps, shape)
        assert int(g[k + "bps"]) == bps and g[k + "n"].size == symbols and g[k + "la"].size == symbols * bps
        assert np.array_equal(p, np.full(M, 1.0 / M) if want is None else want)
        assert MC.inorder_sum(p) == 1.0
        assert float(g[k + "noise_var"]) == PAMAlphabet(bps, 2.0, p).variance * 10 ** (-snr / 10) / 2
        assert np.array_equal(g[k + "cfg"], MC.alternating(M))
        n = g[k + "n"]
        assert ((n >= 0) & (n <= 1)).all()
        assert list(n.ravel()[:4]) == [1e-300, 1 - 2.0 ** -53, 2.0 ** -53, 0.5]
        assert (k + "base_la" in g.files) == has_base


@pytest.mark.parametrize("c", range(N_CASES))
def test_oracle_tables_and_lappr_vs_reference(c):
    g = golden("demap_wide.npz")
    k = f"c{c}_"
    onm = _onm(g, c)
    assert_bit_exact(onm.F_Y_thresholds, g[k + "Fthr"])
    assert_bit_exact(onm.delta_F_Y, g[k + "dF"])
    n, j = g[k + "n"].ravel(), g[k + "j"].ravel().astype(np.int64)
    assert_bit_exact(onm.demap_lappr_array(n, j), g[k + "la"])
    if c in BASE_CASES:
        assert_bit_exact(_onm(g, c, base=True).demap_lappr_array(n, j), g[k + "base_la"])


@pytest.mark.parametrize("c", range(N_CASES))
def test_oracle_root_search_vs_reference(c):
    g = golden("demap_wide.npz")
    k = f"c{c}_"
    di = g[k + "dns_i"].astype(np.int64)
    n = g[k + "n"].ravel()[:di.size]
    for base in (False, True) if c in BASE_CASES else (False,):
        onm = _onm(g, c, base)
        assert_bit_exact([onm.g_inv_search(a, i) for a, i in zip(n, di)], g[k + ("base_dns" if base else "dns")])


@pytest.mark.parametrize("c", range(N_CASES))
def test_oracle_bob_side_at_thresholds_vs_reference(c):
    """hard_decide_index / map_noise on every threshold and its nextafter neighbours, +-0.0,
    every constellation point, the outer thresholds +-100 a_max, +-1e300 and +-inf."""
    g = golden("demap_wide.npz")
    k = f"c{c}_"
    y, xh = g[k + "y_edge"], g[k + "xhat_edge"].astype(np.int64)
    onm = _onm(g, c)
    assert np.array_equal(onm.hard_decide_index(y), xh)
    assert_bit_exact(onm.map_noise(y, xh), g[k + "nhat_edge"])
    if c in BASE_CASES:
        assert_bit_exact(_onm(g, c, base=True).map_noise(y, xh), g[k + "base_nhat_edge"])
