"""CPU tests of the layered decode schedule: the layer builder under sanitizers, the Python
first-fit against the recorded layer sizes, the layered kernels in the built gfx950 code object,
and the conditions of the main case from the restatement alone (tests/layered_fixture.py)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import few_fixture as F
import layered_fixture as LF
import native_check

LIB = os.path.join(ROOT, "qam-reconciliation_amd", "qamr", "libqamr.so")


def test_build_layers_under_asan_ubsan(tmp_path):
    """host_build.hpp build_layers in a stand-alone program (tests/native/layers_check.cpp) under
    AddressSanitizer + UndefinedBehaviorSanitizer, on Hamming(7,4), the mixed code (a hub of degree
    70, parallel edges, isolated variables) and regular_code(1008, 3, 6, 0): no two checks of a
    layer share a variable, every check sits in the smallest free layer, the lists are ascending
    and cover every check once, the repeat flags are right; its layer sizes equal the Python
    first-fit's."""
    from qamr import codes

    exe = native_check.build(tmp_path, "layers_check.cpp", opt="-O1", sanitize=True, extra=["-fno-fast-math"])
    cases = {"hamming": codes.load_edge_csv(os.path.join(GOLDEN, "hamming_7-4.csv")), "mixed": F.mixed_code(),
             "reg1008": codes.regular_code(1008, 3, 6, 0)}
    files = []
    for name, (v, c) in cases.items():
        files.append(str(tmp_path / f"{name}.edges"))
        F.write_edges(files[-1], v, c)
    out = native_check.run(exe, *files)
    assert "layers_check ok: 3 codes" in out
    for path, (v, c) in zip(files, cases.values()):
        layer_of, n = LF.first_fit(v, c)
        sizes = ",".join(str(s) for s in LF.layer_sizes(layer_of, n))
        assert f"{path}: layers={n} sizes={sizes}\n" in out, path
    G = LF.graph_of(*cases["mixed"])
    assert G["repeat"].any() and G["n_layers"] >= 24   # parallel edges; the hub makes dozens of tiny layers
    assert int(LF.graph_of(*cases["reg1008"])["repeat"].sum()) == 3


def test_first_fit_layer_sizes():
    """The Python first-fit gives the recorded layers of the two project codes."""
    from qamr import codes

    layer_of, n = LF.first_fit(*codes.regular_code(1008, 3, 6, 0))
    assert n == 9 and LF.layer_sizes(layer_of, n) == LF.REG1008_LAYER_SIZES
    vid, cid = codes.dvbs2_like_half()
    layer_of, n = LF.first_fit(vid, cid)
    assert n == 17 and LF.layer_sizes(layer_of, n) == LF.DVBS2_LAYER_SIZES
    assert int(LF.graph_of(vid, cid)["repeat"].sum()) == 7


@pytest.fixture(scope="module")
def res():
    assert os.path.exists(LIB), "libqamr.so not built"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as K

    ks = K.kernels(LIB)
    dm = K.demangle([k.removesuffix(".kd") for k in ks])
    return {dm[k.removesuffix(".kd")]: v for k, v in ks.items()}


def test_layered_kernels_in_code_object(res):
    """The gfx950 code object holds k_layer_check for every degree 2..16, for the first iteration
    (true) and the later ones (false), and no layered kernel uses scratch or spills."""
    lay = {k: v for k, v in res.items() if "qr::k_layer_" in k}
    for D in range(2, 17):
        for first in ("true", "false"):
            assert f"void qr::k_layer_check<{D}, {first}>(qr::LayerArgs)" in lay, sorted(lay)
    assert len(lay) == 15 * 2, sorted(lay)
    for name, r in lay.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)


def test_main_case_conditions():
    """At 30 iterations the restatement decodes 42 of the 64 frames and fails 22, the successful
    ones stop at 11 distinct iterations, and the oracle's flooding decode succeeds on the same 42."""
    LF.assert_main_conditions(LF.main_case())


def test_symbols_and_signatures():
    """The four entries are exported and bound."""
    from qamr import _lib

    L = _lib.load()
    for name in ("qr_code_layers", "qr_decode_layered_workspace_size", "qr_decode_layered_device",
                 "qr_decode_layered_host"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["qr_decode_layered_device"] == _lib.SIGNATURES["qr_decode_batch_device"]
    assert _lib.SIGNATURES["qr_decode_layered_host"] == _lib.SIGNATURES["qr_decode_host"]


def test_schedule_keyword_is_checked():
    """``schedule`` is validated as ``demapper`` is: before anything touches the GPU."""
    from qamr import pipeline

    assert pipeline.check_schedule("flooding") == "flooding" and pipeline.check_schedule("layered") == "layered"
    for bad in ("bogus", "", None, "Layered"):
        with pytest.raises(ValueError):
            pipeline.check_schedule(bad)
