"""CPU-side checks of the LAPPR information rate (DESIGN.md "LAPPR information rate"): the host evaluator's
two forms of a term agree, the entry points refuse bad arguments before any device call, the built kernels
use no scratch, and the condition that motivates the estimator holds on the oracle's LAPPRs."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

import lappr_info_fixture as F

sys.path.insert(0, os.path.join(ROOT, "scripts"))


def same(u, v):
    return (u != u and v != v) or np.float64(u).view(np.int64) == np.float64(v).view(np.int64)


def test_straight_line_term_equals_branch_form():
    rng = np.random.default_rng(41)
    xs = list(F.SPECIALS) + (rng.standard_normal(5000) * 8.0).tolist() + \
        (np.where(rng.integers(0, 2, 5000) == 1, -1.0, 1.0) * 2.0 ** rng.uniform(-60, 10, 5000)).tolist()
    bad = [x for x in xs if not same(F.term(x), F.term_branch(x))]
    assert not bad, bad[:5]
    # the special values of the definition
    assert math.isnan(F.term(F.NAN)) and F.term(F.INF) == F.INF
    assert F.term(-F.INF) == 0.0 and math.copysign(1.0, F.term(-F.INF)) == 1.0
    assert F.term(0.0) == 1.0 and F.term(-0.0) == 1.0


def test_evaluator_sum_order_is_chunked():
    """Three chunks of one level: the evaluator's loss is the sum of the chunk sums, not the running sum."""
    rng = np.random.default_rng(42)
    S = 2 * F.CHUNK + 7
    L = rng.standard_normal((1, S)) * 3.0
    w = rng.integers(0, 2, (1, S)).astype(np.uint8)
    loss, errors, total, terr = F.evaluate(L, w, 1, (0.7,))
    t = [F.term(F.signed(0.7, a, b)) for a, b in zip(L[0].tolist(), w[0].tolist())]
    chunks = [0.0, 0.0, 0.0]
    for q in range(3):
        c = 0.0
        for v in t[q * F.CHUNK:(q + 1) * F.CHUNK]:
            c += v
        chunks[q] = c
    assert loss[0, 0, 0] == (0.0 + chunks[0]) + chunks[1] + chunks[2]
    assert total[0, 0] == loss[0, 0, 0]
    assert errors[0, 0] == terr[0] == sum(int((0 if a >= 0 else 1) != b) for a, b in zip(L[0].tolist(), w[0].tolist()))


def test_chunk_constant_is_exported():
    import qamr.mutual_information as mi

    txt = open(os.path.join(ROOT, "include", "qamr.h")).read()
    q = int(re.search(r"^#define QR_LAPPR_INFO_CHUNK (\d+)$", txt, re.M).group(1))
    assert q == mi.LAPPR_INFO_CHUNK == F.CHUNK == 256


def test_reexported_by_the_reference_package_name():
    import qamr.mutual_information as mi
    import qamreconciliation.mutual_information as rmi

    assert rmi.lappr_information is mi.lappr_information
    assert rmi.lappr_information_device is mi.lappr_information_device


# ------------------------------------------------------------------ argument errors, before the device
def _device_args(**kw):
    """A valid argument list of qr_lappr_info_device over host buffers (never launched: every call made with it
    fails a check first), as a dict the caller spoils."""
    bps, ld, S, A = 2, 64, 5, 2
    bufs = dict(lappr=np.zeros(S * bps * ld), word=np.zeros(S * bps * ld, np.uint8), alphas=np.array([1.0, 0.5]),
                loss=np.zeros(A * bps * ld), errors=np.zeros(bps * ld, np.int32), total=np.zeros(A * bps),
                terr=np.zeros(bps, np.int64), ws=np.zeros(1 << 16, np.uint8))
    a = dict(bps=bps, B=3, ld=ld, S=S, A=A, ws_bytes=bufs["ws"].size, _bufs=bufs)
    a.update({k: v.ctypes.data for k, v in bufs.items()})
    a.update(kw)
    return a


def _call_device(a):
    from qamr import _lib

    vp = C.c_void_p
    return _lib.load().qr_lappr_info_device(a["bps"], a["B"], a["ld"], a["S"], vp(a["lappr"]), vp(a["word"]), a["A"],
                                            vp(a["alphas"]), vp(a["loss"]), vp(a["errors"]), vp(a["total"]), vp(a["terr"]),
                                            vp(a["ws"]), a["ws_bytes"], None)


BAD_DEVICE = [dict(bps=0), dict(bps=9), dict(A=0), dict(A=17), dict(S=0), dict(B=0), dict(B=65), dict(ld=96), dict(ld=0),
              dict(lappr=None), dict(word=None), dict(alphas=None), dict(loss=None), dict(errors=None), dict(total=None),
              dict(terr=None), dict(ws=None), dict(ws_bytes=64)]


@pytest.mark.parametrize("spoil", BAD_DEVICE, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_device_entry_refuses_bad_arguments(spoil):
    from qamr import _lib

    assert _call_device(_device_args(**spoil)) == _lib.QR_EVALUE
    assert _lib.last_error()


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_entries_refuse_a_scale_that_is_not_finite(bad):
    from qamr import _lib

    a = _device_args()
    a["_bufs"]["alphas"][1] = bad
    assert _call_device(a) == _lib.QR_EVALUE
    L, w = np.zeros(4), np.zeros(4, np.uint8)
    loss, err = np.zeros(4), np.zeros(2, np.int64)
    al = np.array([1.0, bad])
    assert _lib.load().qr_lappr_info_host(0, 2, 2, _lib.ptr(L), _lib.ptr(w), 2, _lib.ptr(al), _lib.ptr(loss),
                                          _lib.ptr(err)) == _lib.QR_EVALUE


def test_workspace_query_and_host_entry_refuse_bad_arguments():
    from qamr import _lib

    lib = _lib.load()
    n = C.c_size_t(7)
    for bps, ld, S, A in ((0, 64, 4, 1), (9, 64, 4, 1), (2, 65, 4, 1), (2, 0, 4, 1), (2, 64, 0, 1), (2, 64, 4, 0), (2, 64, 4, 17)):
        assert lib.qr_lappr_info_workspace_size(bps, ld, S, A, C.byref(n)) == _lib.QR_EVALUE
        assert n.value == 0
    assert lib.qr_lappr_info_workspace_size(2, 64, 4, 1, None) == _lib.QR_EVALUE
    # [A][bps][chunks][ld] doubles and [bps][chunks][ld] int32, each rounded up to 256 bytes
    assert lib.qr_lappr_info_workspace_size(2, 128, 513, 3, C.byref(n)) == 0
    assert n.value == 3 * 2 * 3 * 128 * 8 + 2 * 3 * 128 * 4
    L, w, al = np.zeros(4), np.zeros(4, np.uint8), np.array([1.0])
    loss, err = np.zeros(2), np.zeros(2, np.int64)
    p = _lib.ptr
    for bps, S, A in ((0, 2, 1), (9, 2, 1), (2, 0, 1), (2, 2, 0), (2, 2, 17)):
        assert lib.qr_lappr_info_host(0, bps, S, p(L), p(w), A, p(al), p(loss), p(err)) == _lib.QR_EVALUE
    for args in ((None, p(w), 1, p(al), p(loss), p(err)), (p(L), None, 1, p(al), p(loss), p(err)),
                 (p(L), p(w), 1, None, p(loss), p(err)), (p(L), p(w), 1, p(al), None, p(err)),
                 (p(L), p(w), 1, p(al), p(loss), None)):
        assert lib.qr_lappr_info_host(0, 2, 2, *args) == _lib.QR_EVALUE


def test_python_entries_raise_value_error_before_the_device():
    import torch

    from qamr.mutual_information import lappr_information, lappr_information_device

    L, w = np.zeros(8), np.zeros(8, np.uint8)
    for args, kw in (((L.astype(np.float32), w, 2), {}), ((L, w.astype(np.int64), 2), {}), ((L, w[:6], 2), {}),
                     ((L[:7], w[:7], 2), {}), ((L[:0], w[:0], 2), {}), ((L, w, 0), {}), ((L, w, 9), {}), ((L, w, 2.5), {}),
                     ((L, w, 2), dict(alphas=())), ((L, w, 2), dict(alphas=[1.0] * 17)),
                     ((L, w, 2), dict(alphas=[1.0, math.nan])), ((L, w, 2), dict(alphas=[math.inf])),
                     ((L.reshape(2, 4), w.reshape(2, 4), 2), {})):
        with pytest.raises(ValueError):
            lappr_information(*args, **kw)
    Lt, wt = torch.zeros((8, 64), dtype=torch.float64), torch.zeros((8, 64), dtype=torch.uint8)
    for args, kw in (((L, w, 1, 2), {}), ((Lt[:, :60], wt[:, :60], 1, 2), {}), ((Lt, wt, 0, 2), {}), ((Lt, wt, 65, 2), {}),
                     ((Lt[:7], wt[:7], 1, 2), {}), ((Lt, wt, 1, 9), {}), ((Lt, wt, 1, 2), dict(alphas=[math.nan])),
                     ((Lt, wt, 1, 2), dict(alphas=[0.5] * 17)), ((Lt.float(), wt, 1, 2), {}),
                     ((Lt, wt, 1, 2), {})):   # the last: host tensors
        with pytest.raises(ValueError):
            lappr_information_device(*args, **kw)


def test_cli_parser_and_llr_source_mode_check():
    from qamr import sim, sim_lappr_information as cli

    a = cli.build_parser().parse_args([])
    assert a.mode == "softening" and a.demapper == "search" and a.alphas == [1.0] and not a.configuration_base
    a = cli.build_parser().parse_args("--bps 4 --snr 13 14.5 --nsnr 2 --symbols 512 --frames 64 --alphas 0.5 1".split())
    assert (a.bps, a.snr, a.nsnr, a.symbols, a.frames, a.alphas) == (4, [13.0, 14.5], 2, 512, 64, [0.5, 1.0])
    assert cli.header(2) == "EsN0dB,alpha,I,I_0,I_1,ber_0,ber_1"
    assert cli.best_alpha([0.5, 0.8, 1.0], [1.0, 1.5, 1.5]) == 0.8   # the first maximum
    assert callable(sim.llr_source) and sim.MODES == ("softening", "direct", "hard")


# ------------------------------------------------------------------ the built code object
def test_kernels_use_no_scratch():
    import kernel_resources as K
    from qamr import _lib

    ks = K.kernels(_lib.LIB_PATH)
    dm = K.demangle([k.removesuffix(".kd") for k in ks])
    got = {dm[k.removesuffix(".kd")]: v for k, v in ks.items() if "lappr_info" in dm[k.removesuffix(".kd")]}
    assert sorted(n.split("(")[0] for n in got) == ["qr::k_lappr_info", "qr::k_lappr_info_total"], sorted(got)
    for name, r in got.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)


# ------------------------------------------------------------------ the motivating condition
def test_search_demapper_is_overconfident_at_alpha_one():
    """4-PAM, 3.0 dB, 4 000 symbols, the oracle's LAPPRs: I(0.5) > 1.0 > I(1.0) bits per symbol (measured 1.0323
    and 0.9614), i.e. the rate-1/2 code's 1.0 is within reach only at a scale below one."""
    _, _, lappr, word, _ = F.motivating_frame()
    loss, errors, total, terr = F.evaluate(lappr[None], word[None], 2, (0.5, 1.0))
    I, I_level = F.rates(total, 1, 4000)
    print(f"I(0.5) = {I[0]!r}, I(1.0) = {I[1]!r}, per level {I_level.tolist()}, errors {terr.tolist()}")
    assert I[0] > 1.0 > I[1]
