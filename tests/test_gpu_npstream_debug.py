"""numpy's stream on the device-asserting debug build (libqamr_debug.so, QR_DEBUG_ASSERT:
tests/test_gpu_debug_build.py).  Its QR_DCHECKs cover every word, prefix-count and output index,
the chain's select and the rank -> slot mapping of the normals (npstream.hip, NpDebugSite 20..24).
A child process on that library runs the normals and frames tests of tests/test_gpu_npstream.py
(the top-up included); conftest's autouse fixture fails any test after which a device check failed."""
import pytest

from debug_rerun import rerun_on_debug_build

pytestmark = pytest.mark.gpu

FILE = "tests/test_gpu_npstream.py"
CASES = [f"{FILE}::test_standard_normal", f"{FILE}::test_frames", f"{FILE}::test_frames_top_up"]


def test_npstream_debug_build_device_checks(gpu):
    # 7 normals cases, 5 shapes x 2 probability vectors x 2 slacks, the top-up
    rerun_on_debug_build(CASES, 28, timeout=300)
