"""Rate adaptation on the device-asserting debug build (libqamr_debug.so, QR_DEBUG_ASSERT:
tests/test_gpu_debug_build.py).  Its QR_DCHECKs cover every output row, payload row and filler index the expand
kernel forms and every listed row of the count (rate_adapt.hip, RaDebugSite 35..38).  A child process on that
library runs the expand, count, replay and blind cases of tests/test_gpu_rate_adapt.py; conftest's autouse
fixture fails any test after which a device check failed."""
import pytest

from debug_rerun import rerun_on_debug_build

pytestmark = pytest.mark.gpu

FILE = "tests/test_gpu_rate_adapt.py"
CASES = [f"{FILE}::test_expand_bit_exact_against_expand_host", f"{FILE}::test_count_rows_against_the_oracle",
         f"{FILE}::test_count_rows_with_the_first_K_rows_equals_count_errors", f"{FILE}::test_stream_and_graph_replay",
         f"{FILE}::test_blind_rounds_against_a_host_replay"]


def test_rate_adapt_debug_build_device_checks(gpu):
    # the 25 expand shapes, the two counts, the replay, the blind rounds
    rerun_on_debug_build(CASES, 29, timeout=300)
