"""k_direct_lappr and k_bare_llr (direct and hard-reverse reconciliation) on tests/golden/llr_sources_wide.npz,
written by tests/golden/make_golden_llr_wide.py from the compiled reference: 3, 5, 6 and 8 bits per symbol and a
shaped 16-PAM, a low and a high SNR each, with channel samples that send g_exp_full down to -inf and
g_log_full to subnormal and zero sums (+-inf and NaN LAPPRs).  tests/test_device_math_cpu.py pins the fixture
to a libm restatement of the reference's loop and asserts that it holds those samples.  Bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_exact, golden

import math_fixture as MF

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def rolled(a, B, ld, fill):
    """[S] or [S][bps] host rows -> device [S (* bps)][ld]: frame f < B is `a` rolled by f samples; the padding
    columns hold `fill`."""
    import torch

    a = np.asarray(a)
    m = np.full((a.size, ld), fill, dtype=a.dtype)
    for f in range(B):
        m[:, f] = np.roll(a, f, axis=0).reshape(-1)
    return torch.from_numpy(m).to("cuda")


@pytest.mark.parametrize("c", range(len(MF.LAPPR_WIDE_CASES)))
def test_direct_and_bare_llr_vs_wide_reference(gpu, c):
    import torch
    import qamr
    from make_golden_cases import demap_wide_probs
    from qamr import _lib

    g = golden("llr_sources_wide.npz")
    bps, shape, _ = MF.LAPPR_WIDE_CASES[c]
    k = f"c{c}_"
    M = 1 << bps
    two_var = float(g[k + "two_var"])
    pa = qamr.PAMAlphabet(bps, 2.0, demap_wide_probs(bps, shape))
    nm = qamr.NoiseMapper(pa, two_var / 2)
    y, x = g[k + "y"], g[k + "x"].astype(np.int64)
    S = y.size
    direct, bare_x = g[k + "direct"].reshape(S, bps), g[k + "bare_llr_x"].reshape(S, bps)
    assert np.isinf(direct).any() and np.isnan(direct).any()
    table = torch.tensor(nm.bare_llr_table, dtype=torch.float64, device="cuda")
    L = _lib.load()
    for B, ld in ((70, 128), (1, 64)):
        out = torch.full((S * bps, ld), SENTINEL, dtype=torch.float64, device="cuda")
        yt = rolled(y, B, ld, 0.0)
        _lib.check(L.qr_direct_lappr_device(nm.handle, two_var, B, ld, S, C.c_void_p(yt.data_ptr()),
                                            C.c_void_p(out.data_ptr()), None))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert_bit_exact(o[:, :B], rolled(direct, B, B, 0.0).cpu().numpy())
        assert (o[:, B:] == SENTINEL).all()
        out.fill_(SENTINEL)
        xt = rolled(x, B, ld, 0)
        _lib.check(L.qr_bare_llr_device(bps, C.c_void_p(table.data_ptr()), B, ld, S, C.c_void_p(xt.data_ptr()),
                                        C.c_void_p(out.data_ptr()), None))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert_bit_exact(o[:, :B], rolled(bare_x, B, B, 0.0).cpu().numpy())
        assert (o[:, B:] == SENTINEL).all()
        # symbols outside [0, M): NaN for every bit of that symbol, the others untouched
        x2 = x.copy()
        x2[0], x2[S - 1] = -1, M
        want = bare_x.copy()
        want[0], want[S - 1] = np.nan, np.nan
        out.fill_(SENTINEL)
        xt = rolled(x2, B, ld, 0)
        _lib.check(L.qr_bare_llr_device(bps, C.c_void_p(table.data_ptr()), B, ld, S, C.c_void_p(xt.data_ptr()),
                                        C.c_void_p(out.data_ptr()), None))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert_bit_exact(o[:, :B], rolled(want, B, B, 0.0).cpu().numpy())
        assert np.isnan(o[:bps, 0]).all() and np.isnan(o[(S - 1) * bps:, 0]).all() and (o[:, B:] == SENTINEL).all()
