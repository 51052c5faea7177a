"""Case tables shared by tests/golden/make_golden.py (which ran them through the reference)
and the tests that read the fixtures back (pure data; importable without the reference)."""
import numpy as np

NOISE_SEARCH_CASES = (  # (bps, snr dB, probabilities or None) of noise_search.npz
    (1, 2.0, None), (2, 3.0, None), (2, 9.5, None), (2, 4.0, (0.1, 0.4, 0.3, 0.2)), (3, 8.0, None),
    (4, 13.0, None), (4, 25.0, None))
NOISE_SEARCH_ACC = (1e-6, 1e-9, 1e-12)


# demap_wide.npz (make_golden_demap_wide.py): (bps, snr dB, probabilities, symbols, also all-zero configuration?)
# probabilities: None = uniform, a float nu = shaped p_m ~ exp(-nu a_m^2), a tuple = as given.
DEMAP_WIDE_CASES = (
    (2, 4.0, (0.1, 0.4, 0.3, 0.2), 420, True),
    (3, 9.5, 0.05, 420, False),
    (4, 13.0, 0.01, 420, True),
    (5, 20.0, 0.003, 420, False),
    (5, 20.0, None, 420, False),
    (6, 30.0, None, 140, False),
    (7, 30.0, None, 70, False),
    (8, 36.0, None, 8, False),
    (2, -12.0, None, 420, False),
    (4, -6.0, None, 420, False),
    (2, 80.0, None, 420, False),
    (4, 80.0, None, 420, False),
    (5, 80.0, 0.003, 70, False),
    (3, 85.0, 0.05, 420, False),
)


def inorder_sum(p):
    """The double sum of p in index order, as alphabet.pyx:52-55 and F_Y(+inf) accumulate it."""
    s = 0.0
    for v in p:
        s += float(v)
    return s


def exact_unit_sum(p):
    """p / sum(p), then the residual of the in-order double sum taken off the largest entry until
    that sum is exactly 1.0.  F_Y(+inf) is that sum (noisemapper.pyx:278-286): with a sum below
    1.0 the reference's bracket loop never ends for a target of 1.0 in the last region.
    One or two corrections suffice for the fixture's cases; where the roundings of the partial
    sums make the corrections cycle (seen on random vectors), the next largest entry takes over."""
    p = np.array(p, np.float64)
    p /= p.sum()
    for m in np.argsort(-p, kind="stable"):
        for _ in range(4):
            r = inorder_sum(p) - 1.0
            if r == 0.0:
                return p
            p[m] -= r
    raise ValueError("the probabilities' in-order sum did not reach 1.0")


def demap_wide_probs(bps, shape):
    """Probability vector of a DEMAP_WIDE_CASES entry (None for the uniform alphabet)."""
    if shape is None:
        return None
    M = 1 << bps
    if isinstance(shape, tuple):
        return exact_unit_sum(shape)
    a = (np.arange(M) - (M - 1) / 2) * 2.0   # alphabet.pyx:62, step 2
    return exact_unit_sum(np.exp(-shape * a * a))


def alternating(M):
    cfg = np.zeros(M, np.uint8)
    cfg[1::2] = 1  # sim_reconciliation.py:84-86
    return cfg
