"""CPU tests of tests/decode_fixture.py, the support module of the decoder's GPU tests: the knob
context manager (qr_tune_set / qr_tune_get need no device), the frame draw and the repack
prediction."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import decode_fixture as DF
import oracle as O


def _get(*names):
    from qamr import _lib

    return tuple(_lib.tune_get(k) for k in names)


def test_knobs_restore_after_the_body_raises():
    before = _get("split", "resident", "few_max")
    with pytest.raises(RuntimeError, match="body"):
        with DF.knobs(dict(split=3, resident=1), resident=0, few_max=5):
            assert _get("split", "resident", "few_max") == (3, 0, 5)
            raise RuntimeError("body")
    assert _get("split", "resident", "few_max") == before


def test_nested_knobs_restore_in_order():
    before = _get("split", "resident")
    with DF.knobs(split=1):
        assert _get("split", "resident") == (1, before[1])
        with DF.knobs(split=3, resident=0):
            assert _get("split", "resident") == (3, 0)
            with DF.knobs(dict(resident=0), split=1):   # a knob of defaults that values does not name: set too
                assert _get("split", "resident") == (1, 0)
            assert _get("split", "resident") == (3, 0)
        assert _get("split", "resident") == (1, before[1])
    assert _get("split", "resident") == before


def test_knobs_refuse_a_changed_default():
    before = _get("split", "resident")
    assert before[0] == 3
    with DF.knobs(split=1):
        with pytest.raises(AssertionError, match="default split=3 changed: update this test"):
            with DF.knobs(dict(resident=before[1], split=3), resident=1 - before[1]):
                pytest.fail("the body must not run")
        assert _get("split", "resident") == (1, before[1])   # and nothing was set
    assert _get("split", "resident") == before


def test_draw_frames_is_deterministic_and_in_the_one_call_order():
    """Hamming(7,4): two draws from the same seed are equal, and equal the draw written out in the
    order words, sigmas, noise."""
    from qamr import codes

    orc = O.OracleCode(*codes.load_edge_csv(os.path.join(GOLDEN, "hamming_7-4.csv")))
    n, sigma = 6, (0.5, 0.8)
    llr, synd, word, sig = DF.draw_frames(orc, np.random.default_rng(42), n, sigma)
    again = DF.draw_frames(orc, np.random.default_rng(42), n, sigma)
    for a, b in zip((llr, synd, word, sig), again):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    rng = np.random.default_rng(42)
    w = rng.integers(0, 2, (n, orc.vnum)).astype(np.uint8)
    s = rng.uniform(*sigma, n)[:, None]
    z = rng.standard_normal((n, orc.vnum))
    assert np.array_equal(word, w) and np.array_equal(sig, s)
    assert np.array_equal(llr, 2 / s ** 2 * ((1 - 2.0 * w) + s * z))
    assert synd.shape == (n, orc.cnum) and all(np.array_equal(synd[f], orc.eval_syndrome(w[f])) for f in range(n))
    assert (sigma[0] <= sig).all() and (sig < sigma[1]).all()


def test_predict_repack_by_hand():
    """B = 512, two ranges of 256.  Range 0: 128 frames succeed at iteration 3, so its running
    count is 256 after iterations 0..2 and 128 from 3 on; the decision point before variable sweep
    4 is the first to read 128 <= 80 % of 256 and repacks to 128 columns; 128 is not <= 80 % of
    128, so that is the only repack.  Range 1: 26 frames succeed at iteration 2, 230 keep running,
    230 > 204.8: never.  With max_iterations = 4 the last decision point (before sweep 3) still
    reads 256: nothing repacks."""
    mi = 8
    succ = np.zeros(512, np.uint8)
    its = np.full(512, mi, np.int32)
    succ[:128], its[:128] = 1, 3
    succ[256:282], its[256:282] = 1, 2
    assert [DF.running(succ, its, 512, t) for t in range(5)] == [(256, 256), (256, 256), (256, 230), (128, 230),
                                                                 (128, 230)]
    assert DF.predict_repack(succ, its, 512, mi) == ((1, 0), (128, 256))
    assert DF.predict_repack(succ, its, 512, 5) == ((1, 0), (128, 256))
    assert DF.predict_repack(succ, its, 512, 4) == DF.NEVER
    # a ragged batch: range 1 holds 194 frames, 168 running from iteration 2 on: 168 <= 204.8 -> 192 columns
    assert DF.running(succ, its, 450, 2) == (256, 168)
    assert DF.predict_repack(succ, its, 450, mi) == ((1, 1), (128, 192))
