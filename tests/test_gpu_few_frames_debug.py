"""The few-frame sweeps on the device-asserting debug build (libqamr_debug.so, QR_DEBUG_ASSERT:
tests/test_gpu_debug_build.py).  Their QR_DCHECKs cover every gathered posterior index, every
message slot (check and variable sweeps) and the lane -> (class, check) mapping (decode_few.hip,
DebugSite 17..19).  A child process on that library runs the mixed-class, routing, sizing and
graph-capture tests of tests/test_gpu_few_frames.py and degrees 2, 8 and 15 of its degree matrix;
conftest's autouse fixture fails any test after which a device check failed."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEBUG_LIB = os.path.join(ROOT, "qam-reconciliation_amd", "qamr", "libqamr_debug.so")

FILE = "tests/test_gpu_few_frames.py"
CASES = [
    f"{FILE}::test_few_mixed_classes_vs_oracle",   # B = 1, 3
    f"{FILE}::test_few_routing",
    f"{FILE}::test_few_max_survives_sizing",
    f"{FILE}::test_few_decode_graph_capture",
    f"{FILE}::test_few_degree_matrix_vs_oracle[2-clean]",
    f"{FILE}::test_few_degree_matrix_vs_oracle[2-special]",
    f"{FILE}::test_few_degree_matrix_vs_oracle[8-clean]",
    f"{FILE}::test_few_degree_matrix_vs_oracle[8-special]",
    f"{FILE}::test_few_degree_matrix_vs_oracle[15-clean]",
    f"{FILE}::test_few_degree_matrix_vs_oracle[15-special]",
]


def test_few_frames_debug_build_device_checks(gpu):
    assert os.path.exists(DEBUG_LIB), "libqamr_debug.so missing: run __graft_entry__.build() (make -C csrc)"
    env = dict(os.environ, QAMR_LIB=DEBUG_LIB, QAMR_DEBUG_ASSERTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", *CASES], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "11 passed" in r.stdout, tail  # the 10 entries above (the mixed-class test has 2 parameters)
