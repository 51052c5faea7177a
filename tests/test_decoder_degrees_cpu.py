"""The oracle's decoder (oracle/qamr_oracle.c) against the compiled reference's own records at every
check degree the decoder's GPU tests cover: tests/golden/decoder_degrees.npz
(tests/golden/make_golden_degrees.py) holds what the reference's Decoder.decode returned for the
frames of ``decode_fixture.golden_cases()`` -- the degree matrix's regular (3, D) codes for
D = 2..16, those of HIGH_DEGREES (17 .. 255), the repack file's seven small codes, the few-frame
mixed code and the high-degree mixed code, clean and special variants -- as success flags,
iteration counts and per-frame digests of the final LAPPRs at max_iterations 1, 2, 3 and 30.

Every GPU test that compares with ``oracle_of`` of one of these cases is thereby pinned to the
reference itself; tests/test_gpu_high_degrees.py also compares the device's outputs with these
records directly.  No GPU is needed here.
"""
import numpy as np
import pytest

from conftest import assert_bit_exact, golden

import decode_fixture as DF

NAMES = list(DF.golden_cases())


@pytest.fixture(scope="module")
def gold():
    return DF.GoldenDegrees(golden("decoder_degrees.npz"))


def test_fixture_lists_exactly_the_cases(gold):
    """Every case of golden_cases(), in its order: check degrees 2..16 and HIGH_DEGREES in both
    variants, seven small codes, two mixed codes; 512 frames each but the few-frame case."""
    assert gold.names == NAMES
    for D in tuple(range(2, 17)) + DF.HIGH_DEGREES:
        assert f"deg{D}-clean" in gold.at and f"deg{D}-special" in gold.at
    assert len(NAMES) == 2 * (15 + len(DF.HIGH_DEGREES)) + len(DF.CODES) + 1 + 2
    assert all(gold.n_frames(s) == (5 if s == "few-mixed" else DF.LD) for s in NAMES)
    assert set(DF.PLANTED) <= set(DF.golden_frames(DF.LD, 1).tolist()) and DF.golden_frames(DF.LD, 1).size == 69
    assert DF.golden_frames(DF.LD, DF.MI).size == DF.LD and DF.golden_full_frames(DF.LD).tolist() == [8, 300, 12]


def test_digest_definition():
    """8 bytes of BLAKE2b per frame over the little-endian int64 view; every NaN counts as
    0x7ff8000000000000, signed zeros and infinities as themselves."""
    import hashlib

    row = np.array([1.5, -0.0, np.inf, np.nan])
    bits = np.array([0x3FF8000000000000, -0x8000000000000000, 0x7FF0000000000000, DF.CANON_NAN], "<i8")
    want = np.frombuffer(hashlib.blake2b(bits.tobytes(), digest_size=8).digest(), np.uint8)
    other_nan = row.copy()
    other_nan.view(np.int64)[3] = 0x7FF0000000000001   # a signalling NaN with another payload
    assert np.isnan(other_nan[3])
    d = DF.frame_digests(np.stack([row, other_nan, np.array([1.5, 0.0, np.inf, np.nan])]))
    assert d.shape == (3, 8) and d.dtype == np.uint8
    assert np.array_equal(d[0], want) and np.array_equal(d[1], want) and not np.array_equal(d[2], want)
    llr, synd = row[None], np.array([[1, 0]], np.uint8)
    assert np.array_equal(DF.input_digest(llr, synd), DF.input_digest(other_nan[None], synd))
    assert not np.array_equal(DF.input_digest(llr, synd), DF.input_digest(llr, 1 - synd))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference_records(gold, name):
    """The inputs are those recorded (digest first); then at max_iterations 1, 2, 3 and 30 the
    oracle's success, iterations and final LAPPRs (by digest) equal the reference's for every
    recorded frame, and the frames stored in full are equal bit for bit."""
    case = DF.golden_cases()[name]()
    DF.assert_golden_inputs(gold, name, case)
    for mi in DF.GOLDEN_MIS:
        DF.assert_golden_records(gold, name, mi, *DF.oracle_of(case, mi))
    frames, full = gold.full(name)
    assert full.shape == (frames.size, case["llr"].shape[1])
    assert_bit_exact(DF.oracle_of(case, DF.MI)[2][frames], full)
    if name.endswith("-special"):   # the recorded special frames carry what was planted: NaN reaches the output
        assert frames.tolist() == [8, 300, 12]
        assert np.isnan(full[:2]).any(axis=1).all() and np.isfinite(full[2]).all()
