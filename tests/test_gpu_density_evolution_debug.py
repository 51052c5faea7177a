"""The sampled density evolution on the device-asserting debug build (libqamr_debug.so, QR_DEBUG_ASSERT:
tests/test_gpu_debug_build.py).  Its QR_DCHECKs cover every degree-table, channel and message index of the three
phases and the source element of the population kernel (density_evolution.hip, DeDebugSite 31..34).  A child
process on that library runs cases A to C of tests/test_gpu_density_evolution.py and, for the population kernel,
case D; conftest's autouse fixture fails any test after which a device check failed."""
import pytest

from debug_rerun import rerun_on_debug_build

pytestmark = pytest.mark.gpu

FILE = "tests/test_gpu_density_evolution.py"
CASES = [f"{FILE}::test_a_regular_ensemble", f"{FILE}::test_b_divergent_degrees", f"{FILE}::test_c_special_values",
         f"{FILE}::test_d_signed_population"]


def test_density_evolution_debug_build_device_checks(gpu):
    # the 16 (M, T) of case A, the two degree mixes of B, the special values of C, the 6 (B, alpha) of D
    rerun_on_debug_build(CASES, 25, timeout=300)
