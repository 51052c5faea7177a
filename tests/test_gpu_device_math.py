"""The device build of the exp / log / erf restatements against libm, bit for bit.

tests/native/*.cpp prove glibc_math.hpp, qamr_math.hpp and strict_pack.hpp equal to libm as x86 host code.
What ships is their gfx950 compile: inline assembly instead of C (g_add_ki, g_bfi), g_exp_full instead of libm
inside erfc, wave-level code that exists only there (g_exp_wave, h_packed), per-kernel table homes and
GlibcK::pinned(), and a dependence on the device compiler honouring -ffp-contract=off.  qr_math_eval_host
runs each primitive in a kernel of its own, called as the product kernels call it, at every table home of a
product call site (include/qamr.h); here each is compared with libm through Python's math (numpy's exp and
log are other routines), the oracle's C restatement (box-plus, erf; tests/test_oracle.py pins it to scipy and the
reference) or numpy's IEEE division, over the input sets of tests/math_fixture.py (drawn where the host
harnesses draw theirs, plus the tails realistic frames never reach).  conftest.assert_bit_exact: signed zeros
count, NaN matches NaN."""
import numpy as np
import pytest

from conftest import assert_bit_exact, golden

import math_fixture as MF

pytestmark = pytest.mark.gpu


def compare(fn, home, x, ref, b=None):
    """One launch; on a mismatch the message names the function, the home and the first differing argument."""
    out = MF.device_eval(fn, home, x, b)
    try:
        assert_bit_exact(out, ref)
    except AssertionError as e:
        bad = ~((out.view(np.int64) == ref.view(np.int64)) | (np.isnan(out) & np.isnan(ref)))
        k = int(np.flatnonzero(bad)[0])
        arg = f"{float(x[k]).hex()} ({x[k]!r})" + (f", {float(b[k]).hex()} ({b[k]!r})" if b is not None else "")
        raise AssertionError(f"{fn} [{home}]: first mismatch at element {k}, argument {arg}: got {float(out[k]).hex()} "
                             f"want {float(ref[k]).hex()}; {e}") from None
    return out


@pytest.fixture(scope="module")
def refs():
    """References computed once per input set and shared by the homes (never modified)."""
    cache = {}

    def get(name, make):
        if name not in cache:
            r = make()
            r.setflags(write=False)
            cache[name] = r
        return cache[name]

    return get


@pytest.mark.parametrize("home", MF.HOMES["exp"])
def test_g_exp(gpu, refs, home):
    x = MF.exp_inputs()
    compare("exp", home, x, refs("exp", lambda: MF.ref_exp(x)))


@pytest.mark.parametrize("home", MF.HOMES["exp_neg"])
def test_g_exp_neg(gpu, refs, home):
    """Default and pinned GlibcK, the table stored twice and indexed by the low byte of ki."""
    x = MF.exp_neg_inputs()
    compare("exp_neg", home, x, refs("exp_neg", lambda: MF.ref_exp(x)))


@pytest.mark.parametrize("home", MF.HOMES["exp_full"])
def test_g_exp_full(gpu, refs, home):
    x = MF.exp_full_inputs()
    out = compare("exp_full", home, x, refs("exp_full", lambda: MF.ref_exp(x)))
    assert np.isinf(out).sum() > 1000 and ((out > 0) & (out < MF.DBL_MIN)).sum() > 800 and np.isnan(out).any()


@pytest.mark.parametrize("home", MF.HOMES["exp_wave"])
def test_g_exp_wave(gpu, refs, home):
    """By wavefront: waves without, with exactly one (lane 0, 31, 32, 63; every kind) and with only special
    lanes, a partial last wave.  Equal to libm and to g_exp_full's own output."""
    x, lay = MF.exp_wave_inputs()
    out = compare("exp_wave", home, x, refs("exp_wave", lambda: MF.ref_exp(x)))
    assert_bit_exact(out, MF.device_eval("exp_full", "explog", x))


@pytest.mark.parametrize("home", MF.HOMES["log"])
def test_g_log(gpu, refs, home):
    x = MF.log_inputs()
    compare("log", home, x, refs("log", lambda: MF.ref_log(x)))


@pytest.mark.parametrize("fn", ["log_u", "log_u_sel"])
@pytest.mark.parametrize("home", MF.HOMES["log_u"])
def test_g_log_u(gpu, refs, home, fn):
    x = MF.log_u_inputs()
    compare(fn, home, x, refs("log_u", lambda: MF.ref_log(x)))


@pytest.mark.parametrize("home", MF.HOMES["log_full"])
def test_g_log_full(gpu, refs, home):
    x = MF.log_full_inputs()
    out = compare("log_full", home, x, refs("log_full", lambda: MF.ref_log(x)))
    assert (out == -np.inf).sum() >= 2 and np.isnan(out).sum() > 10000


@pytest.mark.parametrize("fn", ["h_strict", "h_strict_sel"])
@pytest.mark.parametrize("home", MF.HOMES["h_strict"])
def test_h_strict(gpu, refs, home, fn):
    t = MF.h_inputs()
    compare(fn, home, t, refs("h", lambda: MF.ref_h(t)))


@pytest.mark.parametrize("clamp", ["full", "finite", "none"])
def test_h_packed(gpu, clamp):
    """h_packed<CL> for 1..8 arguments per lane: every lane's result is h_strict of its own argument, whatever
    the wave's mix of near-1 and table-path arguments (slice counts 0, 1, 63, 64, 65, 64 nj of either kind)."""
    for nj in range(1, MF.PACK_MAX_JOBS + 1):
        t, _ = MF.h_packed_inputs(nj, clamp)
        compare("h_packed", MF.CLAMP[clamp] * MF.PACK_MAX_JOBS + nj - 1, t, MF.ref_h(t))


@pytest.mark.parametrize("fn", ["box_plus", "box_plus_sel"])
@pytest.mark.parametrize("home", MF.HOMES["box_plus"])
def test_box_plus(gpu, refs, home, fn):
    a, b = MF.box_plus_inputs()
    compare(fn, home, a, refs("box", lambda: MF.ref_box_plus(a, b)), b)


def test_cephes_erf(gpu):
    """The oracle's erf on every double around the three branch points; scipy's own values on the 8 010 points
    of demap.npz, and scipy itself on the whole set where it imports (1.15.3 is what the reference called)."""
    x = MF.erf_inputs()
    out = compare("erf", "const", x, MF.ref_erf(x))
    assert (out[np.abs(x) > 27] == np.sign(x[np.abs(x) > 27])).all()
    g = golden("demap.npz")
    assert g["erf_x"].size == 8010
    compare("erf", "const", g["erf_x"], np.ascontiguousarray(g["erf_y"]))
    try:
        import scipy.special
    except ImportError:
        return
    assert_bit_exact(out, scipy.special.erf(x))


def test_div_two_s2(gpu):
    x, b = MF.div_inputs()
    compare("div_two_s2", "const", x, MF.ref_div(x, b), b)
