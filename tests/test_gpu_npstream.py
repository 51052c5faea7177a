"""numpy's legacy global stream on the GPU (qamr.NumpyStream, csrc/npstream.hip) against numpy itself
on the host: words, random_sample, choice, standard_normal and whole batches of frames are the values
numpy hands out, bit for bit, and the state afterwards is np.random.get_state()."""
import numpy as np
import pytest

from conftest import assert_bit_exact

pytestmark = pytest.mark.gpu

A4 = np.array([-3.0, -1.0, 1.0, 3.0])
P_UNIFORM = np.full(4, 0.25)
P_SHAPED = np.array([0.15, 0.35, 0.35, 0.15])
SIGMA = 0.8125


def seed_numpy(seed):
    np.random.seed([1, 2, 3] if seed == "array" else seed)


def assert_state_is_numpys(ns):
    got, ref = ns.get_state(), np.random.get_state()
    assert got[0] == ref[0] == "MT19937"
    assert got[2] == ref[2], ("pos", got[2], ref[2])
    assert np.array_equal(got[1], ref[1]), "key"
    assert got[3] == ref[3], ("has_gauss", got[3], ref[3])
    assert np.float64(got[4]).view(np.int64) == np.float64(ref[4]).view(np.int64), ("cached normal", got[4], ref[4])


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("seed", [0, 1, 2 ** 32 - 1, "array"])
def test_words_and_state(gpu, seed):
    """n words from a stream advanced by 0 (pos = 624 after seeding), 1 and 623 words: block starts,
    block ends, one block, several blocks; the state afterwards is numpy's (key, pos, cache)."""
    from qamr import NumpyStream

    for adv in (0, 1, 623):
        for n in (1, 227, 397, 623, 624, 625, 1248, 3 * 624 + 1):
            seed_numpy(seed)
            np.random.bytes(4 * adv)
            ns = NumpyStream()
            got = host(ns.words(n))
            ref = np.frombuffer(np.random.bytes(4 * n), "<u4")
            assert np.array_equal(got, ref), (seed, adv, n)
            assert_state_is_numpys(ns)
            # and the stream goes on from there
            assert np.array_equal(host(ns.words(5)), np.frombuffer(np.random.bytes(20), "<u4")), (seed, adv, n)
            assert_state_is_numpys(ns)


@pytest.mark.parametrize("n", [1, 2, 1001])
def test_random_sample(gpu, n):
    from qamr import NumpyStream

    np.random.seed(11)
    np.random.bytes(4 * 7)   # an odd word position inside the block
    ns = NumpyStream()
    got = host(ns.random_sample(n))
    assert_bit_exact(got, np.random.random_sample(n))
    assert_state_is_numpys(ns)


@pytest.mark.parametrize("p", [np.full(2, 0.5), P_UNIFORM, np.full(16, 1 / 16), P_SHAPED], ids=["m2", "m4", "m16", "shaped"])
def test_choice(gpu, p):
    from qamr import NumpyStream

    np.random.seed(12)
    np.random.randn(1)   # a cached normal: choice must leave it alone
    ns = NumpyStream()
    got = host(ns.choice(p, 1001))
    assert np.array_equal(got, np.random.choice(p.size, size=1001, p=p))
    assert_state_is_numpys(ns)
    assert ns.get_state()[3] == 1


@pytest.mark.parametrize("n, cached", [(1, 0), (2, 0), (3, 0), (1001, 1), (1, 1), (100003, 0), (600001, 0)])
def test_standard_normal(gpu, n, cached):
    """1, 2, 3 normals; 1001 and a single one from a stream that enters with a cached normal; 100 003
    (a scan workgroup spans 1024 candidates per class: about 62 of them per class) and 600 001 (more
    than 256 tile sums per class: the scan of the sums takes several rounds)."""
    from qamr import NumpyStream

    np.random.seed(13)
    if cached:
        np.random.randn(1)
        assert np.random.get_state()[3] == 1
    ns = NumpyStream()
    got = host(ns.standard_normal(n))
    assert_bit_exact(got, np.random.randn(n))
    assert_state_is_numpys(ns)
    assert_bit_exact(host(ns.standard_normal(2)), np.random.randn(2))
    assert_state_is_numpys(ns)


def host_frames(p, S, B):
    """The reference's loop (sims/reconciliation.pyx:129-132) on numpy's global stream: x [B, S],
    y [B, S], cumulative words per frame and the state after every frame."""
    x = np.empty((B, S), np.int64)
    y = np.empty((B, S))
    states = []
    for f in range(B):
        x[f] = np.random.choice(p.size, size=S, p=p)
        y[f] = A4[x[f]] + SIGMA * np.random.randn(S)
        states.append(np.random.get_state())
    return x, y, states


def words_between(s0, s1, upper):
    """Words consumed between two states of one stream (fewer than `upper`)."""
    n = (s1[2] - s0[2]) % 624   # the positions fix the count modulo a block
    while n <= upper:
        np.random.set_state(s0)
        if n:
            np.random.bytes(4 * n)
        st = np.random.get_state()
        if st[2] == s1[2] and np.array_equal(st[1], s1[1]):
            return n
        n += 624
    raise AssertionError("states are not on one stream")


def check_frames(S, B, ld, p, seed, slack_pct):
    from qamr import NumpyStream, _lib

    saved = _lib.tune_get("np_slack_pct")
    try:
        if slack_pct is not None:
            _lib.tune_set("np_slack_pct", slack_pct)
        np.random.seed(seed)
        np.random.bytes(4 * 3)
        s0 = np.random.get_state()
        ns = NumpyStream()
        x, y, fw = ns.frames(p, A4, SIGMA, S, B, ld=ld)
    finally:
        _lib.tune_set("np_slack_pct", saved)
    assert tuple(x.shape) == tuple(y.shape) == (S, ld)
    x, y, fw = host(x), host(y), host(fw)
    xr, yr, states = host_frames(p, S, B)
    assert np.array_equal(x[:, :B].T, xr)
    assert_bit_exact(y[:, :B].T, yr)
    assert not x[:, B:].any() and not y[:, B:].view(np.int64).any(), "padding columns are not zero"
    assert_state_is_numpys(ns)
    end = np.random.get_state()
    # words per frame: the host's consumed count, found from its states
    prev, total, upper = s0, 0, 8 * S + 4096
    cum = []
    for f in range(B):
        total += words_between(prev, states[f], upper)
        prev = states[f]
        cum.append(total)
    assert np.array_equal(fw, np.array(cum, np.int64))
    for w in sorted({0, B // 2, B - 1}):
        ns.seek_frame(w)
        np.random.set_state(states[w])
        assert_state_is_numpys(ns)
    np.random.set_state(end)
    return ns


SHAPES = [(1, 5, 64), (2, 64, 64), (7, 200, 256), (504, 1, 64), (504, 130, 192)]


@pytest.mark.parametrize("slack_pct", [0, None], ids=["mean_only", "default_slack"])
@pytest.mark.parametrize("p", [P_UNIFORM, P_SHAPED], ids=["uniform", "shaped"])
@pytest.mark.parametrize("S, B, ld", SHAPES)
def test_frames(gpu, S, B, ld, p, slack_pct):
    """Batches of frames against the host loop frame by frame: symbols, samples, zero padding,
    words per frame, the state after the batch and after seek_frame(0 / middle / last).  S = 1 and
    S = 7 carry a cached normal across frames; np_slack_pct = 0 sizes the first range at the mean."""
    check_frames(S, B, ld, p, 21, slack_pct)


def test_frames_top_up(gpu):
    """np_slack_pct = 0: seeds whose 130 frames of 504 symbols need more than the mean range are
    located twice (the chain runs again after the range was extended) and come out the same."""
    import qamr

    topped = 0
    qamr.profile_enable(True)
    try:
        for seed in (31, 32, 33, 34, 35, 36):
            qamr.profile_reset()
            check_frames(504, 130, 192, P_SHAPED, seed, 0)
            n_chain = qamr.profile_query("np_chain")[1]
            assert 1 <= n_chain <= 9
            topped += n_chain >= 2
    finally:
        qamr.profile_enable(False)
        qamr.profile_reset()
    # the consumption is within a fraction of a standard deviation of its mean about every other
    # time: six seeds that all fit the mean range have probability 2^-6
    assert topped >= 1


def test_profile_names(gpu):
    import qamr

    qamr.profile_enable(True)
    try:
        qamr.profile_reset()
        check_frames(7, 200, 256, P_SHAPED, 41, None)
        for name in ("np_words", "np_scan", "np_chain", "np_fill"):
            ms, n = qamr.profile_query(name)
            assert n >= 1 and ms > 0.0, (name, ms, n)
    finally:
        qamr.profile_enable(False)
        qamr.profile_reset()


def test_frames_argument_errors(gpu):
    import torch

    from qamr import NumpyStream

    np.random.seed(1)
    ns = NumpyStream()
    before = ns.get_state()
    with pytest.raises(ValueError):
        ns.frames(P_SHAPED, A4, SIGMA, 7, 5, ld=65)       # ld % 64
    with pytest.raises(ValueError):
        ns.frames(P_SHAPED, A4, SIGMA, 7, 65, ld=64)      # ld < B
    with pytest.raises(ValueError):
        ns.frames(P_SHAPED, A4, SIGMA, 0, 5)              # S <= 0
    with pytest.raises(ValueError):
        ns.frames(P_SHAPED, A4, SIGMA, 7, 0, ld=64)       # B <= 0
    with pytest.raises(ValueError):
        ns.frames(np.ones(1), np.zeros(1), SIGMA, 7, 5)   # M outside 2..256
    with pytest.raises(ValueError):
        ns.seek_frame(0)                                  # no frames call yet
    assert np.array_equal(ns.get_state()[1], before[1]) and ns.get_state()[2] == before[2]
    torch.cuda.synchronize()
