"""SURVEY.md §5 sanitizers: the host-side code under AddressSanitizer + UndefinedBehavior-
Sanitizer (CPU only; GPU ASan is not available on the MI355X pool).

* oracle/qamr_oracle.c (the C restatement: CSR build, node rules, decode with inf/NaN/-0.0,
  NoiseMapper tables, demap, Bob side) driven by oracle/asan_main.c (`make -C oracle asan`);
* libqamr's host code: the Tanner-graph CSR builder and the NoiseMapper / fast-search table
  builders (csrc/host_build.hpp), glibc/fast-math tables, and the per-symbol demapper on the
  host (tests/native/host_asan_check.cpp, hipcc with -Xarch_host -fsanitize=...).

Both run with -fno-sanitize-recover=all: any report is a non-zero exit."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

from native_check import build, run


def test_oracle_under_asan_ubsan():
    if not shutil.which("gcc"):
        pytest.skip("gcc unavailable")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "asan"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    run(os.path.join(ROOT, "oracle", "_asan", "oracle_asan"))


def test_libqamr_host_code_under_asan_ubsan(tmp_path):
    run(build(tmp_path, "host_asan_check.cpp", opt="-O1", sanitize=True, extra=["-fno-fast-math"]))
