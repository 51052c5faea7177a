"""Host check of glibc_math.hpp, the strict box-plus arithmetic: the restated glibc
exp/log (and h(t) = log(1.0 + exp(-t)), box-plus built on them) must return the same
bits as the host libm -- the reference's own arithmetic (decoder.pyx:41-45) -- on
~16M inputs dense on the decoder's domain.  Compiled for the host with hipcc; the
tables are regenerated from libm into tmp_path (tests/native_check.py: build)."""
from native_check import build, run


def test_glibc_exp_log_restatement_bit_exact(tmp_path):
    run(build(tmp_path, "glibc_math_check.cpp"), "4000000", timeout=300)
