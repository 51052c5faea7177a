"""The layered check sweep on the device-asserting debug build (libqamr_debug.so, QR_DEBUG_ASSERT:
tests/test_gpu_debug_build.py).  Its QR_DCHECKs cover every check id with its degree, every
gathered variable, every message row and the lane's frame column (decode_layered.hip, DebugSite
27..30).  A child process on that library runs the main case and the mixed-class codes of
tests/test_gpu_layered.py; conftest's autouse fixture fails any test after which a device check
failed."""
import pytest

from debug_rerun import rerun_on_debug_build

pytestmark = pytest.mark.gpu

FILE = "tests/test_gpu_layered.py"
CASES = [
    f"{FILE}::test_main_case_vs_definition",       # 4 iteration caps x 3 shapes
    f"{FILE}::test_mixed_classes_vs_definition",
    f"{FILE}::test_mix12_16_5_vs_definition",
]


def test_layered_debug_build_device_checks(gpu):
    rerun_on_debug_build(CASES, 14, timeout=300)
