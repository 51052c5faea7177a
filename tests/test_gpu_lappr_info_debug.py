"""The LAPPR information rate on the device-asserting debug build (libqamr_debug.so, QR_DEBUG_ASSERT:
tests/test_gpu_debug_build.py).  Its QR_DCHECKs cover the row index of every LAPPR read and the workspace
slot of every chunk sum (lappr_info.hip, InfoDebugSite 25..26).  A child process on that library runs the
bit-exact cases and the stream / graph-replay test of tests/test_gpu_lappr_info.py; conftest's autouse fixture
fails any test after which a device check failed."""
import pytest

from debug_rerun import rerun_on_debug_build

pytestmark = pytest.mark.gpu

FILE = "tests/test_gpu_lappr_info.py"
CASES = [f"{FILE}::test_bit_exact_against_the_evaluator", f"{FILE}::test_stream_and_graph_replay"]


def test_lappr_info_debug_build_device_checks(gpu):
    # the 14 shapes (two of them past one pass of k_lappr_info_total), the replay
    rerun_on_debug_build(CASES, 15, timeout=300)
