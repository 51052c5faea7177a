"""CPU tests of the few-frame decode: the message-slot layout builder under sanitizers, the
``few_max`` knob, and the few-frame kernels in the built gfx950 code object."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import few_fixture as F
import native_check

LIB = os.path.join(ROOT, "qam-reconciliation_amd", "qamr", "libqamr.so")


def test_few_layout_under_asan_ubsan(tmp_path):
    """host_build.hpp build_few_layout in a stand-alone program (tests/native/few_layout_check.cpp)
    under AddressSanitizer + UndefinedBehaviorSanitizer: the slots form a bijection with the edges
    and every variable's list is in ascending edge id, on Hamming(7,4), on the mixed code (seven
    classes, one of a single check; parallel edges, isolated variables) and on
    regular_code(770, 3, 7)."""
    from qamr import codes

    exe = native_check.build(tmp_path, "few_layout_check.cpp", opt="-O1", sanitize=True, extra=["-fno-fast-math"])
    cases = {"hamming": codes.load_edge_csv(os.path.join(GOLDEN, "hamming_7-4.csv")), "mixed": F.mixed_code(),
             "reg770": codes.regular_code(770, 3, 7)}
    vid, cid = cases["mixed"]
    assert np.bincount(np.bincount(cid))[11] == 1  # the one-check class
    files = []
    for name, (v, c) in cases.items():
        files.append(str(tmp_path / f"{name}.edges"))
        F.write_edges(files[-1], v, c)
    assert "few_layout_check ok: 3 codes" in native_check.run(exe, *files)


def test_few_max_knob():
    """0, 1 and 64 round-trip; -1 and 65 are refused and change nothing."""
    from qamr import _lib

    saved = _lib.tune_get("few_max")
    try:
        for v in (0, 1, 64):
            _lib.tune_set("few_max", v)
            assert _lib.tune_get("few_max") == v
        for v in (-1, 65):
            with pytest.raises(ValueError):
                _lib.tune_set("few_max", v)
            assert _lib.tune_get("few_max") == 64
    finally:
        _lib.tune_set("few_max", saved)
    assert _lib.tune_get("few_max") == saved


@pytest.fixture(scope="module")
def res():
    assert os.path.exists(LIB), "libqamr.so not built"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as K

    ks = K.kernels(LIB)
    dm = K.demangle([k.removesuffix(".kd") for k in ks])
    return {dm[k.removesuffix(".kd")]: v for k, v in ks.items()}


def test_few_kernels_in_code_object(res):
    """The gfx950 code object holds k_few_check for every degree 2..16 in the normal mode (1), and
    no few-frame kernel spills to scratch."""
    few = {k: v for k, v in res.items() if "qr::k_few_" in k}
    for D in range(2, 17):
        assert f"void qr::k_few_check<{D}, 1>(qr::FewCheckArgs)" in few, sorted(few)
    assert any(k.startswith("void qr::k_few_var<false>") for k in few), sorted(few)
    assert any(k.startswith("void qr::k_few_var<true>") for k in few), sorted(few)
    assert len(few) == 15 * 3 + 2, sorted(few)
    for name, r in few.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
