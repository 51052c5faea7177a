"""numpy's stream on the device-asserting debug build (libqamr_debug.so, QR_DEBUG_ASSERT:
tests/test_gpu_debug_build.py).  Its QR_DCHECKs cover every word, prefix-count and output index,
the chain's select and the rank -> slot mapping of the normals (npstream.hip, NpDebugSite 20..24).
A child process on that library runs the normals and frames tests of tests/test_gpu_npstream.py
(the top-up included); conftest's autouse fixture fails any test after which a device check failed."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEBUG_LIB = os.path.join(ROOT, "qam-reconciliation_amd", "qamr", "libqamr_debug.so")

FILE = "tests/test_gpu_npstream.py"
CASES = [f"{FILE}::test_standard_normal", f"{FILE}::test_frames", f"{FILE}::test_frames_top_up"]


def test_npstream_debug_build_device_checks(gpu):
    assert os.path.exists(DEBUG_LIB), "libqamr_debug.so missing: run __graft_entry__.build() (make -C csrc)"
    env = dict(os.environ, QAMR_LIB=DEBUG_LIB, QAMR_DEBUG_ASSERTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", *CASES], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "28 passed" in r.stdout, tail  # 7 normals cases, 5 shapes x 2 probability vectors x 2 slacks, the top-up
