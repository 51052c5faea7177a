"""The few-frame sweeps on the device-asserting debug build (libqamr_debug.so, QR_DEBUG_ASSERT:
tests/test_gpu_debug_build.py).  Their QR_DCHECKs cover every gathered posterior index, every
message slot (check and variable sweeps) and the lane -> (class, check) mapping (decode_few.hip,
DebugSite 17..19).  A child process on that library runs the mixed-class, routing, sizing and
graph-capture tests of tests/test_gpu_few_frames.py and degrees 2, 8 and 15 of its degree matrix;
conftest's autouse fixture fails any test after which a device check failed."""
import pytest

from debug_rerun import rerun_on_debug_build

pytestmark = pytest.mark.gpu

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
    rerun_on_debug_build(CASES, 11, timeout=300)  # the 10 entries above (the mixed-class test has 2 parameters)
