"""The child run on the device-asserting debug build (libqamr_debug.so, QR_DEBUG_ASSERT), shared by the GPU
tests that repeat parity tests under its QR_DCHECK index checks.  With QAMR_DEBUG_ASSERTS=1 conftest's autouse
fixture fails any test of the child after which a device check failed."""
import os
import subprocess
import sys

from conftest import ROOT

DEBUG_LIB = os.path.join(ROOT, "qam-reconciliation_amd", "qamr", "libqamr_debug.so")


def rerun_on_debug_build(node_ids, passed, timeout):
    """The tests `node_ids` in a fresh pytest process that loads the debug library: all `passed` of them pass."""
    assert os.path.exists(DEBUG_LIB), "libqamr_debug.so missing: run __graft_entry__.build() (make -C csrc)"
    env = dict(os.environ, QAMR_LIB=DEBUG_LIB, QAMR_DEBUG_ASSERTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", *node_ids], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=timeout)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert f"{passed} passed" in r.stdout, tail
