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


# ------------------------------------------------------------------ check degrees above 16
HIGH_KEYS = DF.HIGH_DEGREES + ("mix",)


def test_high_degree_codes_shapes_and_histograms():
    """The regular (3, D) codes of HIGH_DEGREES: V as listed, every variable of degree 3, every
    check of degree D.  The mixed code: V = 702, the classes' sizes (one of 65 checks, one of a
    single check; degree 7 is packed, 12 templated and unpacked, 17 / 30 / 64 runtime), parallel
    edges, every sixth variable isolated, variable 0 a hub of degree 70."""
    assert DF.HIGH_DEGREES == (17, 18, 22, 27, 30, 33, 65, 100, 255)
    assert [DF.v_of(D) for D in DF.HIGH_DEGREES] == [782, 768, 770, 774, 770, 770, 780, 800, 850]
    assert all(DF.sigma_of(D) == (0.25, 0.5) for D in DF.HIGH_DEGREES) and DF.sigma_of(16) == (0.35, 0.6)
    for D in DF.HIGH_DEGREES:
        case = DF.case_of(D, "clean")
        V = DF.v_of(D)
        assert case["llr"].shape == (DF.LD, V) and case["synd"].shape == (DF.LD, 3 * V // D)
        assert np.array_equal(np.bincount(case["vid"]), np.full(V, 3))
        assert np.array_equal(np.bincount(case["cid"]), np.full(3 * V // D, D))
        assert DF.high_classes(D) == [(D, 3 * V // D)]
    vid, cid = DF.himix_code()
    V = DF.HIMIX_V
    assert V == 702 and int(vid.max()) + 1 == V
    cdeg = np.bincount(cid)
    assert {int(d): int((cdeg == d).sum()) for d in np.unique(cdeg)} == dict(DF.HIMIX_CLASSES) == {
        7: 40, 12: 20, 17: 65, 30: 13, 64: 1}
    assert DF.high_classes("mix") == DF.HIMIX_CLASSES
    pairs = np.stack([vid, cid], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs), "the code needs parallel edges"
    vdeg = np.bincount(vid, minlength=V)
    iso = np.arange(V) % 6 == 2
    assert vdeg[0] == DF.HIMIX_HUB_DEGREE == 70 and (vdeg[iso] == 0).all() and iso.sum() == 117
    assert set(vdeg[~iso][1:].tolist()) == {3, 4}
    for variant in ("clean", "special"):
        case = DF.himix_case(variant)
        assert case["llr"].shape == (DF.LD, V) and case["synd"].shape == (DF.LD, 139)
        assert case is DF.high_case("mix", variant) and DF.case_of(30, variant) is DF.high_case(30, variant)


def test_special_variant_differs_from_clean_only_in_the_planted_frames():
    for key in (30, "mix"):
        clean, special = DF.high_case(key, "clean"), DF.high_case(key, "special")
        rest = np.setdiff1d(np.arange(DF.LD), DF.PLANTED)
        assert np.array_equal(clean["llr"][rest], special["llr"][rest]) and np.array_equal(clean["synd"], special["synd"])
        for f in (8, 300):
            got = special["llr"][f, :5]
            assert np.array_equal(got.view(np.int64)[:4], np.array(DF.SPECIAL5[:4]).view(np.int64)) and np.isnan(got[4])
            assert np.array_equal(special["llr"][f, 5:], clean["llr"][f, 5:])
        cw = list(DF.PLANTED[:8])
        assert cw == [0, 1, 2, 3, 256, 257, 258, 259]
        assert all(special["orc"].check_lappr(special["llr"][f], special["synd"][f]) for f in cw)


@pytest.mark.parametrize("variant", ["clean", "special"])
@pytest.mark.parametrize("key", HIGH_KEYS)
def test_high_degree_conditions(key, variant):
    """assert_high_conditions, from the oracle alone: 0 < successes < 512, >= 5 distinct stop
    iterations >= 1, the planted codewords stop at (1, 0), at most 384 frames still running after
    iteration 29 (so a 128-column tile goes idle while the active-frame lists are live)."""
    n, stops, left = DF.assert_high_conditions(DF.high_case(key, variant), variant)
    print(key, variant, "successes", n, "distinct stop iterations", stops, "running after 29", left)
    if key == "mix":   # the figures recorded beside HIMIX_SIGMA
        assert (n, stops, left) == {"special": (481, 22, 32), "clean": (482, 22, 31)}[variant]


def test_check_block_restates_make_geom():
    """By hand: 512 columns, 128-column tiles, 2 checks side by side; min_blocks = 2048 leaves a
    class of 77 checks one check per thread, min_blocks = 0 the knob's 16."""
    assert DF.check_block(512, 77) == (128, 2)                       # 77 * 4 / (2048 * 2) = 0 -> per 1
    assert DF.check_block(512, 77, min_blocks=0) == (128, 32)
    assert DF.check_block(512, 77, check_ft=64, check_per=3, min_blocks=0) == (64, 12)
    assert DF.check_block(512, 77, check_ft=256) == (256, 1)
    assert DF.check_block(64, 77, min_blocks=0) == (64, 64)          # ld = 64: the tile divides the columns
    assert DF.check_block(128, 77, check_ft=256, min_blocks=0) == (128, 32)
    assert DF.check_block(4096, 32400, min_blocks=2048) == (128, 32)  # a large class keeps its per


def test_high_degree_classes_end_in_a_ragged_block():
    """With min_blocks = 0 a workgroup holds 32 checks (per 16 x 2 side by side) at the default
    tile and 12 (per 3 x 4) at check_ft = 64, check_per = 3: every runtime-degree class must leave
    its last workgroup ragged, so the ``ci >= n_checks`` break of k_check_generic runs.  The
    regular (3, 18) code has 3 * 768 / 18 = 128 = 4 * 32 checks (v_of is shared with the degree
    matrix), and 36 and 24 are multiples of 12: those classes are ragged in the other of the two
    runs, and which class is ragged where is pinned here."""
    per16 = DF.check_block(DF.LD, 1, min_blocks=0)[1]
    ft64 = DF.check_block(DF.LD, 1, check_ft=64, check_per=3, min_blocks=0)[1]
    assert (per16, ft64) == (32, 12)
    full16, full64 = [], []
    for key in HIGH_KEYS:
        for d, n in DF.high_classes(key):
            if d > 16:
                full16 += [(key, d, n)] if n % per16 == 0 else []
                full64 += [(key, d, n)] if n % ft64 == 0 else []
    assert full16 == [(18, 18, 128)] and full64 == [(65, 65, 36), (100, 100, 24)]
    assert not set(full16) & set(full64)   # every class is ragged in at least one of the two runs
