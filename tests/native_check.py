"""Build and run of the stand-alone host programs under tests/native/ (each has its own ``main``; none is
loaded into Python), shared by the CPU tests that pin host arithmetic and run it under sanitizers.

* ``build``: glibc_tables.inc into the directory (once), then one hipcc line for gfx950.
* ``run``: the program under the sanitizers' option environment; exit status 0 and no sanitizer report.
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "qam-reconciliation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# host code only; -fno-sanitize-recover=all turns any report into a non-zero exit
SANITIZE = [a for f in ("-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=all") for a in ("-Xarch_host", f)]
SANITIZER_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def build(tmp_dir, source_name, *, exe_name=None, opt="-O2", sanitize=False, extra=()):
    """Compile tests/native/<source_name> into tmp_dir and return the executable's path; ``sanitize`` adds debug
    information and the address and undefined-behaviour sanitizers on the host code."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc unavailable")
    tmp_dir = str(tmp_dir)
    inc = os.path.join(tmp_dir, "glibc_tables.inc")
    if not os.path.exists(inc):
        subprocess.run([sys.executable, os.path.join(CSRC, "gen_glibc_tables.py"), inc], check=True)
    exe = os.path.join(tmp_dir, exe_name or os.path.splitext(source_name)[0])
    san = ["-g", "-fno-omit-frame-pointer", *SANITIZE] if sanitize else []
    cc = subprocess.run([HIPCC, "--offload-arch=gfx950", opt, "-ffp-contract=off", "-std=c++17", *extra, *san, "-I" + CSRC,
                         "-I" + os.path.join(ROOT, "include"), "-I" + tmp_dir, "-o", exe,
                         os.path.join(ROOT, "tests", "native", source_name)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


def run(exe, *args, timeout=600):
    """Run the program and return its stdout."""
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **SANITIZER_ENV))
    out = r.stdout + r.stderr
    print(" ".join(args), "\n", out[-3000:])
    assert r.returncode == 0, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out
    return r.stdout
