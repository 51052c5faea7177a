"""CPU-side checks of the quad-integrated mutual-information evaluators: the fixture
(tests/golden/mi_quad.npz, written by tests/golden/make_golden_mi_quad.py), the host integrator and the
two integrands' arithmetic (tests/native/mi_quad_check.cpp runs the very functions the kernel and the
batched driver run, the interpolated g_inv of csrc/grid_interp.hpp included), qr_quad_host through ctypes, the argument checks, the CLIs' parsers and
configuration lists, and the reference's import lines."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT, assert_bit_exact, golden

import native_check
from mapper_fixture import alphabet

CASES = range(1, 11)
HOST_INTEGRAL_CASES = (1, 2, 3, 4, 5, 9, 10)   # the 2-PAM and 4-PAM cases: both integrals wholly on the host


@pytest.fixture(scope="module")
def fx():
    return golden("mi_quad.npz")


def test_fixture_is_well_formed(fx):
    assert int(fx["n_cases"]) == 10
    assert [int(fx[f"c{c}_bps"]) for c in CASES] == [1, 1, 2, 2, 2, 3, 4, 4, 2, 2]
    assert [int(fx[f"c{c}_limit"]) for c in CASES] == [50] * 9 + [5]
    for c in CASES:
        k = f"c{c}_"
        M = 1 << int(fx[k + "bps"])
        pa = alphabet(fx, k)
        assert fx[k + "cfg"].shape == (M,) and fx[k + "p_Xhat"].shape == (M,) and abs(fx[k + "p_Xhat"].sum() - 1) < 1e-9
        assert fx[k + "base_x"].shape == fx[k + "base_f"].shape and fx[k + "xy_x"].shape == fx[k + "xy_f"].shape
        nb, nx = min(64, int(fx[k + "base_neval"])), min(64, int(fx[k + "xy_neval"]))
        assert fx[k + "base_x"].size == nb + 2 and fx[k + "xy_x"].size == nx + 3
        assert fx[k + "base_x"][-2:].tolist() == [0.0, 1.0] and (fx[k + "base_x"][:nb] > 0).all() and (fx[k + "base_x"][:nb] < 1).all()
        sigma = math.sqrt(float(fx[k + "noise_var"]))
        assert fx[k + "xy_x"][-3:].tolist() == [0.0, 1e3 * sigma, -1e3 * sigma]
        assert np.isfinite(fx[k + "base_f"]).all()
        # quad's bookkeeping: 21 points per interval of QAGS, 2 x 15 per interval of QAGI
        assert int(fx[k + "base_neval"]) == 42 * int(fx[k + "base_last"]) - 21
        assert int(fx[k + "xy_neval"]) == 2 * (30 * int(fx[k + "xy_last"]) - 15)
        assert float(fx[k + "noise_var"]) > 0 and pa.order == M
    # the generator's conditions, on the stored data
    assert {int(fx[f"c{c}_base_neval"]) for c in (2, 5)} == {21}
    assert int(fx["c1_base_neval"]) == 1071 and int(fx["c1_base_last"]) == 26 and int(fx["c1_base_warned"]) == 1
    assert int(fx["c10_base_warned"]) == 1 and int(fx["c10_base_last"]) == 5
    assert [c for c in CASES if fx[f"c{c}_xy_I"] == -np.inf] == [5, 6, 8]
    assert all(np.isfinite(fx[f"c{c}_base_I"]) for c in CASES)
    assert all(np.isfinite(fx[f"c{c}_xy_I"]) for c in CASES if c not in (5, 6, 8))
    assert not fx["c9_cfg"].any() and fx["c3_cfg"].tolist() == [0, 1, 0, 1] and not np.all(fx["c3_probs"] == fx["c3_probs"][0])
    assert fx["ig_fn"].size == 24 and set(fx["ig_limit"].tolist()) == {1, 3, 5, 50} and set(fx["ig_eps"].tolist()) == {1.49e-8, 1e-12}
    assert 0 < int(fx["ig_warned"].sum()) < 24 and sorted(set(fx["ig_inf"].tolist())) == [0, 1]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mi_quad.npz")) < os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "interp.npz"))


def dump_integrator(fx, path):
    cols = [fx["ig_" + n].astype(np.float64) for n in ("fn", "inf", "c", "w", "limit", "eps", "result", "abserr", "neval", "warned")]
    np.concatenate([[float(cols[0].size)], np.stack(cols, axis=1).ravel()]).tofile(path)


def dump_case(fx, c, path, integrals):
    """The raw input of `mi_quad_check case`."""
    from qamr.mutual_information import GRID_DEFAULTS

    k = f"c{c}_"
    pa = alphabet(fx, k)
    parts = [np.array([pa.bit_per_symbol, float(fx[k + "noise_var"]), float(fx[k + "limit"]), GRID_DEFAULTS[0], GRID_DEFAULTS[1],
                       float(pa.step), float(integrals)]),
             pa.constellation, pa.probabilities, pa.thresholds, fx[k + "cfg"], fx[k + "p_Xhat"]]
    for name in ("base", "xy"):
        parts += [[float(fx[k + name + "_x"].size)], fx[k + name + "_x"], fx[k + name + "_f"]]
    for name in ("base", "xy"):
        parts += [[float(fx[k + name + "_" + f]) for f in ("I", "abserr", "neval", "warned")]]
    np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]).tofile(path)


def run_check(exe, fx, tmp_path):
    path = str(tmp_path / "integrator.bin")
    dump_integrator(fx, path)
    assert "24 records, 0 mismatches" in native_check.run(exe, "integrator", path)
    for c in CASES:
        path = str(tmp_path / f"case{c}.bin")
        dump_case(fx, c, path, c in HOST_INTEGRAL_CASES)
        out = native_check.run(exe, "case", path)
        npts = fx[f"c{c}_base_x"].size + fx[f"c{c}_xy_x"].size
        assert f"{npts} points, 0 mismatches" in out
        assert ("2 on the host, 0 mismatches" in out) == (c in HOST_INTEGRAL_CASES)


def test_host_driver_and_integrands_bit_exact(fx, tmp_path):
    """The host integrator equals scipy's quad on the 24 integrator-only records; mi_base_arg / mi_xy_arg with
    host providers equal the fixture at every stored abscissa; both integrals of the 2-PAM and 4-PAM cases,
    wholly on the host through the same driver, equal the fixture's."""
    run_check(native_check.build(tmp_path, "mi_quad_check.cpp"), fx, tmp_path)


def test_host_driver_and_integrands_under_sanitizers(fx, tmp_path):
    """The same stand-alone program with the address and undefined-behaviour sanitizers on the host code."""
    run_check(native_check.build(tmp_path, "mi_quad_check.cpp", exe_name="mi_quad_check_san", sanitize=True), fx, tmp_path)


INTEGRANDS = (
    lambda x, c, w: 1.0 / (w * w + (x - c) * (x - c)),
    lambda x, c, w: math.sqrt(abs(x - c)),
    lambda x, c, w: 1.0 / math.sqrt(abs(x - c) + 1e-300),
    lambda x, c, w: (1.0 if x > c else 0.0) + x * x,
)


@pytest.mark.parametrize("r", [0, 5, 14, 23])
def test_quad_host_through_ctypes(fx, r):
    """qr_quad_host over a Python callback on four of the integrator-only records (no device call)."""
    from qamr.mutual_information import quad_host

    fn, c, w = int(fx["ig_fn"][r]), float(fx["ig_c"][r]), float(fx["ig_w"][r])
    eps = float(fx["ig_eps"][r])
    I, abserr, neval, ier, last = quad_host(lambda x: INTEGRANDS[fn](x, c, w), int(fx["ig_inf"][r]), 0.0, 1.0, epsabs=eps,
                                            epsrel=eps, limit=int(fx["ig_limit"][r]))
    assert_bit_exact([I, abserr], [fx["ig_result"][r], fx["ig_abserr"][r]])
    assert neval == int(fx["ig_neval"][r]) and last == int(fx["ig_last"][r])
    assert (ier != 0) == bool(fx["ig_warned"][r])


def test_quad_host_on_a_smooth_function():
    from qamr.mutual_information import quad_host

    I, abserr, neval, ier, last = quad_host(lambda x: x * x, 0, 0.0, 3.0)
    assert abs(I - 9.0) < 1e-13 and neval == 21 and ier == 0 and last == 1
    I, abserr, neval, ier, last = quad_host(lambda x: 1.0 / (1.0 + x * x), 1, 0.0, 0.0)
    assert abs(I - math.pi) < 1e-9 and ier == 0 and neval == 2 * (30 * last - 15)


def fake_nm(bps):
    return types.SimpleNamespace(bit_per_symbol=bps, order=1 << bps, handle=None, _device=0)


def test_argument_validation_before_any_device_call():
    from qamr import _lib
    from qamr.mutual_information import (mutual_information_base_scheme, mutual_information_base_scheme_arg_array,
                                         mutual_information_quad_batch, mutual_information_X_Y, quad_host)

    L = _lib.load()
    for s in ("qr_mi_quad_batch", "qr_mi_quad_stats", "qr_mi_integrand_device", "qr_mi_integrand_host", "qr_quad_host",
              "qr_mi_quad_rule_host"):
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    with pytest.raises(ValueError, match="bit_per_symbol"):
        mutual_information_quad_batch("X_Y", [fake_nm(2), fake_nm(3)])
    with pytest.raises(ValueError, match="p_Xhat"):
        mutual_information_quad_batch("base", [fake_nm(2)], p_Xhats=[np.ones(3) / 3])
    with pytest.raises(ValueError, match="p_Xhat"):
        mutual_information_quad_batch("base", [fake_nm(2), fake_nm(2)], p_Xhats=np.ones((1, 4)) / 4)
    with pytest.raises(ValueError, match="p_Xhat"):
        mutual_information_quad_batch("base", [fake_nm(2)])
    with pytest.raises(ValueError, match="p_Xhat"):
        mutual_information_base_scheme(fake_nm(2), np.ones(5) / 5)
    with pytest.raises(ValueError, match="p_Xhat"):
        mutual_information_base_scheme_arg_array(np.zeros(3), fake_nm(2), np.ones(5) / 5)
    with pytest.raises(ValueError, match="sign_configs"):
        mutual_information_quad_batch("X_Y", [fake_nm(2)], sign_configs=np.zeros((1, 3), np.uint8))
    with pytest.raises(ValueError, match="limit"):
        mutual_information_quad_batch("X_Y", [fake_nm(2)], limit=0)
    with pytest.raises(ValueError, match="limit"):
        mutual_information_X_Y(fake_nm(2), limit=0)
    with pytest.raises(ValueError, match="limit"):
        quad_host(lambda x: x, 0, 0.0, 1.0, limit=0)
    with pytest.raises(ValueError, match="kind"):
        mutual_information_quad_batch("other", [fake_nm(2)])
    # the C-ABI itself
    E = _lib.QR_EVALUE
    z = np.zeros(4)
    zi = np.zeros(4, np.int32)
    args = (_lib.ptr(z), _lib.ptr(z), _lib.ptr(zi), _lib.ptr(zi), None)
    assert L.qr_mi_quad_batch(None, None, None, -1, 1, 1e-8, 1e-8, 50, *args) == E
    assert L.qr_mi_quad_batch(None, None, None, 1, 1, 1e-8, 1e-8, 0, *args) == E and "limit" in _lib.last_error()
    assert L.qr_mi_quad_batch(None, None, None, 1, 2, 1e-8, 1e-8, 50, *args) == E and "kind" in _lib.last_error()
    assert L.qr_mi_quad_batch(None, None, None, 1, 1, 1e-8, 1e-8, 50, *args) == E and "null" in _lib.last_error()
    assert L.qr_mi_quad_batch(None, None, None, 0, 1, 1e-8, 1e-8, 50, *args) == 0
    handles = (C.c_void_p * 1)(None)
    assert L.qr_mi_quad_batch(handles, None, None, 1, 1, 1e-8, 1e-8, 50, *args) == E and "null demapper" in _lib.last_error()
    assert L.qr_mi_integrand_host(None, 0, 4, _lib.ptr(z), _lib.ptr(z)) == E
    assert L.qr_mi_integrand_device(None, 1, 4, None, None, None) == E
    assert L.qr_mi_quad_stats(None) == E
    # QUADPACK's own refusal: epsabs <= 0 with epsrel below 50 eps
    I, abserr, neval, ier, last = quad_host(lambda x: x, 0, 0.0, 1.0, epsabs=0.0, epsrel=1e-20)
    assert (I, abserr, neval, ier, last) == (0.0, 0.0, 0, 6, 0)


def test_reference_import_lines_resolve():
    # sim_mutual_information_base_scheme.py:5-7 and sim_mutual_information_compare_signs.py:5-6
    from qamreconciliation.mutual_information import (mutual_information_base_scheme, mutual_information_X_Xhat,
                                                      mutual_information_X_Y, P_xhat)
    from qamreconciliation.mutual_information import montecarlo_information  # noqa: F401
    from qamreconciliation.mutual_information import mutual_information_base_scheme_arg, mutual_information_X_Y_int_arg
    import qamr.mutual_information as mi

    assert mutual_information_base_scheme is mi.mutual_information_base_scheme
    assert mutual_information_X_Y is mi.mutual_information_X_Y
    assert mutual_information_base_scheme_arg is mi.mutual_information_base_scheme_arg
    assert mutual_information_X_Y_int_arg is mi.mutual_information_X_Y_int_arg
    assert all(callable(f) for f in (P_xhat, mutual_information_X_Xhat, mi.mutual_information_quad_batch,
                                     mi.mutual_information_base_scheme_arg_array, mi.mutual_information_X_Y_int_arg_array))
    for mod in (mi, sys.modules["qamreconciliation.mutual_information"]):
        assert "Out of scope" not in (mod.__doc__ or "") and "not provided" not in (mod.__doc__ or "")


def test_base_scheme_cli_parser_defaults_match_the_reference():
    from qamr.sim_mutual_information_base_scheme import COLUMNS, build_parser

    a = build_parser().parse_args([])
    assert (a.out, a.snr, a.nsnr, a.bps, a.device) == ("out.csv", [0, 5], 11, 2, 0)
    a = build_parser().parse_args(["--snr", "-3", "7.5", "--nsnr", "2", "--bps", "4", "--device", "1", "--out", "x.csv"])
    assert (a.out, a.snr, a.nsnr, a.bps, a.device) == ("x.csv", [-3.0, 7.5], 2, 4, 1)
    assert COLUMNS == ["EsN0dB", "EbN0dB base", "I(N,X;Xhat)", "EbN0dB X;Xhat", "I(X;Xhat)", "EbN0dB X;Y", "I(X;Y)"]
    for flag in ("--display", "--gnuplot"):
        with pytest.raises(SystemExit):
            build_parser().parse_args([flag])   # plotting is out of scope


def test_compare_signs_cli_parser_and_configuration_list(fx):
    from qamr.sim_mutual_information_compare_signs import build_parser, column_list, config_count, config_list

    a = build_parser().parse_args([])
    assert (a.out, a.snr, a.nsnr, a.bps, a.montecarlo, a.nmontecarlo, a.nloops, a.seed, a.device) == (
        "out.csv", [0, 5], 11, 2, False, 1 << 12, 1 << 6, 0, 0)
    a = build_parser().parse_args(["--montecarlo", "--nmontecarlo", "64", "--nloops", "2", "--seed", "3", "--bps", "3"])
    assert (a.montecarlo, a.nmontecarlo, a.nloops, a.seed, a.bps) == (True, 64, 2, 3, 3)
    assert config_count(2) == 10 and config_count(3) == 136
    for bps, key in ((2, "cfg2"), (3, "cfg3")):
        cfgs = config_list(bps)
        assert cfgs.dtype == np.uint8 and np.array_equal(cfgs, fx[key]) and len(cfgs) == config_count(bps)
    # configuration c has a[i] = bit i of c; at bps 2 the list is c = 0, 1, 2, 3, 4, 5, 6, 8, 10, 12
    assert config_list(2)[0].tolist() == [0, 0, 0, 0] and config_list(2)[-1].tolist() == [0, 0, 1, 1]
    assert config_list(3)[0].tolist() == [0] * 8 and config_list(3)[-1].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    cols = column_list(2)
    assert cols == ["EsN0dB"] + [f"I(X,N;Xhat)_{c}" for c in (0, 1, 2, 3, 4, 5, 6, 8, 10, 12)]
