"""Rate adaptation, host side (qamr/rate_adapt.py; DESIGN.md "Rate adaptation"): the slot map and the filler
order, expand_host (the normative definition of the expand kernel), rate(), every refusal, untainted_order on
the 1008 code, and the argument checks of the two C entries, which refuse before any device call."""
import numpy as np
import pytest

from conftest import assert_bit_exact

L0 = 1e300


def example():
    """V = 10: shortened (7, 2), punctured (5, 0, 9) -> fillers 7, 2, 5, 0, 9; payload rows 1, 3, 4, 6, 8."""
    from qamr.rate_adapt import RateAdaption

    return RateAdaption(10, punctured=[5, 0, 9], shortened=[7, 2])


def test_slot_map_and_filler_order():
    a = example()
    assert (a.V, a.p, a.s, a.n) == (10, 3, 2, 5)
    assert a.fillers.tolist() == [7, 2, 5, 0, 9]
    assert a.payload_rows.tolist() == [1, 3, 4, 6, 8] and a.payload_rows.dtype == np.int64
    assert a.slot.dtype == np.int32
    #                           v: 0   1   2  3  4   5  6   7  8   9
    assert a.slot.tolist() == [-4, 0, -2, 1, 2, -3, 3, -1, 4, -5]


def test_from_order_discloses_the_last_pick_first():
    from qamr.rate_adapt import RateAdaption

    order = np.array([4, 8, 1, 6, 0, 9, 3, 2, 7, 5])
    a = RateAdaption.from_order(order, 3, 2)
    assert a.punctured.tolist() == [1, 8, 4] and a.shortened.tolist() == [7, 5]
    assert a.fillers.tolist() == [7, 5, 1, 8, 4]
    assert a.payload_rows.tolist() == [0, 2, 3, 6, 9]
    b = RateAdaption.from_order(order, 0, 0)
    assert b.n == 10 and b.slot.tolist() == list(range(10)) and b.fillers.size == 0


def payload(B, n):
    rng = np.random.default_rng(3)
    lp = rng.normal(0, 4, (B, n))
    lp[0, 0], lp[1, 1], lp[2, 2], lp[3, 3], lp[4, 4] = np.nan, np.inf, -np.inf, -0.0, 1e300
    lp[5, 0] = -1e300
    wp = rng.integers(0, 2, (B, n), dtype=np.uint8)
    return lp, wp


@pytest.mark.parametrize("revealed", [None, 0, 1, 3, 8, -3])
def test_expand_host_on_the_example(revealed):
    from qamr.rate_adapt import expand_host

    a = example()
    B = 6
    lp, wp = payload(B, a.n)
    fill = np.array([[0, 1, 0, 1, 1], [1, 0, 1, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [7, 0, 255, 0, 2],
                     [0, 1, 1, 0, 1]], np.uint8)
    rev = None if revealed is None else np.full(B, revealed, np.int64)
    lappr, word = expand_host(a, lp, wp, fill, rev)
    assert lappr.shape == (B, 10) and word.shape == (B, 10) and word.dtype == np.uint8
    # payload: bit for bit (NaN, +-inf, -0.0, +-1e300 included)
    assert_bit_exact(lappr[:, a.payload_rows], lp)
    assert np.isnan(lappr[0, 1]) and np.signbit(lappr[3, 6]) and lappr[3, 6] == 0.0
    assert np.array_equal(word[:, a.payload_rows], wp)
    # fillers, written out: filler j at variable fillers[j]; known iff j < s + max(revealed, 0)
    r = 0 if revealed is None else max(revealed, 0)
    for b in range(B):
        for j, v in enumerate([7, 2, 5, 0, 9]):
            bit = 1 if fill[b, j] else 0
            assert word[b, v] == bit
            want = (-L0 if bit else L0) if j < 2 + r else 0.0
            assert lappr[b, v] == want and not (want == 0.0 and np.signbit(lappr[b, v]))


def test_expand_host_per_frame_counts_and_other_L():
    from qamr.rate_adapt import expand_host

    a = example()
    lp, wp = payload(6, a.n)
    fill = np.ones((6, 5), np.uint8)
    lappr, _ = expand_host(a, lp, wp, fill, np.array([0, 1, 3, 8, -3, 2]), L=25.0)
    known = np.array([2, 3, 5, 5, 2, 4])
    for b in range(6):
        assert lappr[b, [7, 2, 5, 0, 9]].tolist() == [-25.0] * known[b] + [0.0] * (5 - known[b])
    for bad in (np.inf, np.nan, 0.0, -1.0):
        with pytest.raises(ValueError):
            expand_host(a, lp, wp, fill, None, L=bad)
    with pytest.raises(ValueError):
        expand_host(a, lp[:, :4], wp, fill)


def test_rate_against_the_formula():
    from qamr.rate_adapt import RateAdaption

    V, C, K = 1008, 504, 504
    for p, s in ((0, 0), (100, 0), (0, 200), (100, 100)):
        a = RateAdaption.from_order(np.arange(V), p, s)
        assert a.rate(K) == (K - s) / (V - p - s)
        assert a.rate(K, 12.5) == (K - s - 12.5) / (V - p - s)
        leak = (C - p + s) / a.n                       # disclosed per payload bit: the syndrome and the s shortened bits
        assert abs((1 - a.rate(K)) - (leak - s / a.n)) < 1e-15
    assert RateAdaption.from_order(np.arange(V), 0, 0).rate(K) == 0.5


def test_value_errors():
    from qamr.rate_adapt import RateAdaption

    for pun, sho in (([1, 2], [2, 3]), ([1, 1], []), ([], [4, 4]), ([10], []), ([], [-1])):
        with pytest.raises(ValueError):
            RateAdaption(10, pun, sho)
    with pytest.raises(ValueError):                     # no payload left
        RateAdaption(4, [0, 1], [2, 3])
    a = RateAdaption(10, [0, 1, 2, 3], [4, 5, 6, 7, 8])   # n = 1
    with pytest.raises(ValueError):                     # p + s = 9 > V - bps = 8
        a.check_bps(2)
    assert a.check_bps(1) == 1
    b = RateAdaption(10, [0], [1, 2])                   # n = 7
    with pytest.raises(ValueError):                     # a payload that is not whole symbols
        b.check_bps(2)
    assert RateAdaption(10, [0], [1]).check_bps(2) == 4
    with pytest.raises(ValueError):
        RateAdaption.from_order(np.arange(10), 6, 5)
    with pytest.raises(ValueError):
        RateAdaption.from_order(np.arange(10), -1, 0)


def test_untainted_order_on_the_1008_code():
    from qamr import codes
    from qamr.rate_adapt import untainted_order

    vid, cid = codes.regular_code(1008, 3, 6, seed=0)
    order, u = untainted_order(vid, cid, 0)
    order2, u2 = untainted_order(vid, cid, 0)
    assert u == u2 == 132 and np.array_equal(order, order2)          # deterministic
    assert order.dtype == np.int64 and np.array_equal(np.sort(order), np.arange(1008))
    other, _ = untainted_order(vid, cid, 1)
    assert not np.array_equal(order, other)
    first = np.zeros(1008, bool)
    first[order[:u]] = True
    on = first[vid]
    per_check = np.bincount(cid[on], minlength=504)
    assert per_check.max() == 1                                      # no check has two neighbours among the first u
    for v in order[:u]:                                              # none of them has a repeated check
        c = cid[vid == v]
        assert np.unique(c).size == c.size == 3
    # the walk: the rest keeps the order of the permutation
    walk = np.random.default_rng(0).permutation(1008)
    assert np.array_equal(order[u:], walk[~first[walk]]) and np.array_equal(order[:u], walk[first[walk]])
    # maximal: every later variable has a marked or a repeated check
    marked = per_check > 0
    for v in order[u:]:
        c = cid[vid == v]
        assert marked[c].any() or np.unique(c).size < c.size


def test_c_entries_refuse_bad_arguments_before_the_device():
    import qamr
    from qamr import _lib

    L = qamr.load()
    for s in ("qr_rate_adapt_expand_device", "qr_count_errors_rows_device"):
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    a = np.zeros(64 * 16, np.float64)
    p = _lib.ptr(a)       # never dereferenced: every call below is refused before a launch
    assert a.ctypes.data % 16 == 0

    def expand(V=10, n=5, pp=3, s=2, B=16, ld=64, ptrs=None, Lv=1e300, rev=None):
        q = [p] * 6 if ptrs is None else ptrs   # slot, lappr_pay, word_pay, fill, lappr, word
        rc = L.qr_rate_adapt_expand_device(V, n, pp, s, q[0], B, ld, q[1], q[2], q[3], rev, Lv, q[4], q[5], None)
        with pytest.raises(ValueError):
            _lib.check(rc)

    for k in range(6):
        q = [p] * 6
        q[k] = None
        expand(ptrs=q)
    expand(B=0)
    expand(B=65)
    expand(ld=96, B=16)
    expand(n=4)               # n + p + s != V
    expand(V=5, n=0, pp=3, s=2)
    expand(V=10, n=13, pp=-3, s=0)
    expand(V=10, n=13, pp=0, s=-3)
    for bad in (np.inf, -np.inf, np.nan, 0.0, -1.0):
        expand(Lv=bad)
    odd = _lib.C.c_void_p(a.ctypes.data + 8)   # 8-byte but not 16-byte aligned
    expand(ptrs=[p, odd, p, p, p, p])

    def count(B=16, ld=64, n_rows=8, ptrs=None):
        q = [p] * 7 if ptrs is None else ptrs
        with pytest.raises(ValueError):
            _lib.check(L.qr_count_errors_rows_device(B, ld, n_rows, *q, None))

    for k in range(7):
        q = [p] * 7
        q[k] = None
        count(ptrs=q)
    for B, ld, n_rows in ((65, 64, 8), (0, 64, 8), (16, 96, 8), (16, 64, -1)):
        count(B, ld, n_rows)


def test_simulator_refuses_numpy_stream_before_the_device():
    """adapt with stream="numpy": the reference's stream has no draws for the filler bits."""
    from qamr import sim
    from qamr.rate_adapt import RateAdaption

    a = RateAdaption.from_order(np.arange(1008), 10, 10)
    with pytest.raises(ValueError, match="adapt"):
        sim.Simulator(None, 2, stream="numpy", adapt=a)
