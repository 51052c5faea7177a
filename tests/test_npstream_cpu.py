"""CPU tests of numpy's stream on the GPU: its host pieces (untempering, the state a word offset stands
for, the sizing rule) in a stand-alone program under sanitizers against numpy's own words and states,
the keyword checks of the simulations, and the new entries of the C-ABI."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import native_check

ENTRIES = ("qr_npstream_create", "qr_npstream_destroy", "qr_npstream_state", "qr_npstream_words_device",
           "qr_npstream_random_sample_device", "qr_npstream_standard_normal_device", "qr_npstream_choice_device",
           "qr_npstream_frames_workspace_size", "qr_npstream_frames_device", "qr_npstream_seek_frame")


def write_case(path, seed, adv, n, offsets):
    """The case file of tests/native/npstream_check.cpp from numpy itself."""
    np.random.seed(seed)
    if adv:
        np.random.bytes(4 * adv)
    s0 = np.random.get_state()
    words = np.frombuffer(np.random.bytes(4 * n), "<u4")
    with open(path, "wb") as fh:
        fh.write(np.ascontiguousarray(s0[1], "<u4").tobytes())
        fh.write(np.array([s0[2], n], "<i4").tobytes())
        fh.write(words.tobytes())
        fh.write(np.array([len(offsets)], "<i4").tobytes())
        for c in offsets:
            np.random.set_state(s0)
            if c:
                np.random.bytes(4 * c)
            st = np.random.get_state()
            fh.write(np.array([c, st[2]], "<i4").tobytes())
            fh.write(np.ascontiguousarray(st[1], "<u4").tobytes())


def test_host_pieces_under_asan_ubsan(tmp_path):
    """npstream_host.hpp in tests/native/npstream_check.cpp under AddressSanitizer +
    UndefinedBehaviorSanitizer: untempering inverts tempering; the blocks generated from
    np.random.get_state()'s key are np.random.bytes' words; the key and pos rebuilt from the tempered
    words at an offset are np.random.get_state() after that many words (offsets inside a block, on a
    block's end, several blocks on; a stream that starts at pos = 624, 1 and 623); the sizing rule."""
    exe = native_check.build(tmp_path, "npstream_check.cpp", opt="-O1", sanitize=True, extra=["-fno-fast-math"])
    for i, (seed, adv) in enumerate([(0, 0), (1, 1), (2 ** 32 - 1, 623), (7, 300)]):
        path = str(tmp_path / f"case{i}.bin")
        n = 3 * 624 + 1
        first_end = (624 - adv) % 624   # words to the end of the starting block (adv = 0: it stands there)
        offsets = sorted({0, 1, first_end, first_end + 1, first_end + 624, 1248, n})
        write_case(path, seed, adv, n, [c for c in offsets if 0 <= c <= n])
        assert "npstream_check ok" in native_check.run(exe, path)


def test_stream_keyword_errors(monkeypatch):
    """An unknown stream and numpy's stream on two ranks are ValueErrors before any device is touched
    (the frames of one stream are sequential: there are no ranks in this mode)."""
    from qamr.sim import Simulator, check_stream, simulate_direct_snr_dB

    with pytest.raises(ValueError, match="stream"):
        Simulator(None, 2, stream="pcg64")
    with pytest.raises(ValueError, match="stream"):
        simulate_direct_snr_dB(2.0, None, 2, 5, 8, 100, stream="Numpy")
    assert check_stream("torch") == "torch" and check_stream("numpy") == "numpy"
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    with pytest.raises(ValueError, match="one rank"):
        Simulator(None, 2, stream="numpy")
    assert check_stream("torch") == "torch"   # torch's streams are per rank


def test_cli_has_the_stream_switch():
    from qamr.sim_reconciliation import build_parser

    p = build_parser()
    assert p.parse_args(["edges.csv"]).stream == "torch"
    assert p.parse_args(["edges.csv", "--stream", "numpy"]).stream == "numpy"
    with pytest.raises(SystemExit):
        p.parse_args(["edges.csv", "--stream", "pcg64"])


def test_entries_in_header_and_ctypes_table():
    from qamr import _lib

    txt = open(os.path.join(ROOT, "include", "qamr.h")).read()
    declared = set(re.findall(r"QR_API\s+int\s*(qr_npstream_\w+)\s*\(", txt))
    assert declared == set(ENTRIES)
    L = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert re.search(r"#define QR_EINTERNAL 5\b", txt) and _lib.QR_EINTERNAL == 5
    with pytest.raises(_lib.QamrError):
        _lib.check(_lib.QR_EINTERNAL)


def test_np_slack_pct_knob():
    from qamr import _lib

    saved = _lib.tune_get("np_slack_pct")
    assert saved == 100
    try:
        for v in (0, 50, 400):
            _lib.tune_set("np_slack_pct", v)
            assert _lib.tune_get("np_slack_pct") == v
        with pytest.raises(ValueError):
            _lib.tune_set("np_slack_pct", -1)
        assert _lib.tune_get("np_slack_pct") == 400
    finally:
        _lib.tune_set("np_slack_pct", saved)


def test_numpy_stream_needs_a_device():
    """No CPU fallback: without a HIP device a NumpyStream cannot be made."""
    from conftest import has_gpu

    from qamr import NumpyStream, QamrError

    if has_gpu():
        return
    with pytest.raises(QamrError):
        NumpyStream()
