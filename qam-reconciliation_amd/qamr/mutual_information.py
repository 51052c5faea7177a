"""Mutual-information evaluators of the reference (qamreconciliation/mutual_information.pyx) whose
hot path runs on the gfx950 kernels.

``P_xhat`` (:29-39) and ``mutual_information_X_Xhat`` (:152-172) are O(M^2) host loops in the
reference's accumulation order, with ``math.log2`` (libm's, as the reference's ``libc.math.log2``;
numpy's vectorised log2 is a different routine).  They need no device.

``montecarlo_information`` (:218-297) draws one block of N samples from numpy's legacy global stream
exactly as the reference does -- ``pa.random_symbols(N)``, then N scalar ``np.random.randn()``
draws, ``y = a[x] + sigma * z`` -- and evaluates the block on the GPU (qr_mi_montecarlo_host): under
``np.random.seed(s)`` it returns the doubles the reference returns.  ``montecarlo_information_device``
evaluates B such blocks, already in HBM, in one launch pair (qr_mi_montecarlo_device).

Out of scope: ``mutual_information_base_scheme(_arg)`` and ``mutual_information_X_Y(_int_arg)``, the
``scipy.integrate.quad`` drivers of the module.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, check_tensor, ptr

__all__ = ["P_xhat", "mutual_information_X_Xhat", "montecarlo_information", "montecarlo_information_device",
           "which_mask"]


def P_xhat(nm):
    """mutual_information.pyx:29-39: res[i] = sum_j probabilities[j] * fwrd_transition_probability[j, i],
    j ascending from 0.0."""
    M = int(nm.order)
    p = [float(v) for v in nm.probabilities]
    fw = np.asarray(nm.fwrd_transition_probability, np.float64)
    res = np.empty(M, np.float64)
    for i in range(M):
        acc = 0.0
        for j in range(M):
            acc += p[j] * float(fw[j, i])
        res[i] = acc
    return res


def mutual_information_X_Xhat(nm, p_Xhat):
    """mutual_information.pyx:152-172 (closed form of I(X;Xhat) from the transition table)."""
    M = int(nm.order)
    p = [float(v) for v in nm.probabilities]
    fw = np.asarray(nm.fwrd_transition_probability, np.float64)
    pX = [float(v) for v in p_Xhat]
    res = 0.0
    for j in range(M):
        sum_i = 0.0
        for i in range(M):
            f = float(fw[j, i])
            tmp = 0.0
            if f > 0.0:
                tmp += math.log2(f)
            if pX[i] > 0.0:
                tmp -= math.log2(pX[i])
            sum_i += tmp * f
        res += p[j] * sum_i
    return res


def which_mask(which) -> int:
    """The reference's ``which`` (three flags: I(X;Xhat), I(X;Y), I(X,N;Xhat)) as the C-ABI's bit mask."""
    w = np.asarray(which).ravel()
    if w.size < 3:
        raise ValueError("which must hold three flags")
    return (1 if w[0] else 0) | (2 if w[1] else 0) | (4 if w[2] else 0)


def _prepare(nm, p_Xhat):
    """Make the demapper handle ready for the estimator: the interpolation grid in HBM and the
    (p_Xhat, fwrd_transition_probability) tables; uploads only when p_Xhat changed."""
    pX = np.ascontiguousarray(np.asarray(p_Xhat, np.float64).ravel())
    if pX.size != nm.order:
        raise ValueError(f"p_Xhat has {pX.size} entries, the alphabet {nm.order}")
    nm._device_grid()
    key = pX.tobytes()
    if getattr(nm, "_mi_key", None) != key:
        fw = np.ascontiguousarray(nm.fwrd_transition_probability, np.float64)
        check(_lib.load().qr_demap_mi_tables(nm.handle, ptr(pX), ptr(fw)), "mi_tables")
        nm._mi_key = key


def montecarlo_information(pa, nm, p_Xhat, N, which=np.ones(3, dtype=np.uint8), _terms=None):
    """mutual_information.pyx:218-297: (I(X;Xhat), I(X;Y), I(X,N;Xhat)) estimated on N fresh samples
    drawn from numpy's global stream as the reference draws them."""
    N = int(N)
    w = np.ascontiguousarray(np.asarray(which, np.uint8).ravel()[:3])
    if w.size < 3:
        raise ValueError("which must hold three flags")
    x = np.ascontiguousarray(pa.random_symbols(N), np.int64)                 # :239
    y = np.array(pa.index_to_value(x), np.float64)                           # :240
    sigma = float(nm.noise_sigma)
    for p in range(N):                                                       # :241-242
        y[p] += sigma * np.random.randn()
    _prepare(nm, p_Xhat)
    out = np.empty(3, np.float64)
    check(_lib.load().qr_mi_montecarlo_host(nm.handle, N, ptr(x), ptr(y), ptr(w), ptr(out),
                                            None if _terms is None else ptr(_terms)), "montecarlo_information")
    return float(out[0]), float(out[1]), float(out[2])


def montecarlo_information_device(nm, p_Xhat, x_fi, y_fi, B, which=np.ones(3, dtype=np.uint8), terms=False,
                                  stream=None, out=None):
    """B blocks of S samples in one launch pair: x_fi int64 [S, ld] (symbol indices), y_fi float64
    [S, ld] (received samples), block f in column f -> float64 (3, B): row q = quantity q of every
    block.  With terms=True also the per-sample terms, float64 (3, S, ld) (columns [B, ld) and the
    planes of disabled quantities are not written).  `terms` may also be the float64 (3, S, ld) tensor
    to write them into, `out` a float64 (3, ld) tensor for the totals (columns [0, B) are written)."""
    import torch

    if not isinstance(y_fi, torch.Tensor) or y_fi.dim() != 2:
        raise ValueError("montecarlo_information_device: y_fi must be a 2-D tensor [S, ld]")
    S, ld = y_fi.shape
    if ld % 64 or not 0 < int(B) <= ld or S < 1:
        raise ValueError(f"montecarlo_information_device: need ld % 64 == 0, 0 < B <= ld, S >= 1 (B={B}, ld={ld}, S={S})")
    dev = nm._device
    check_tensor(y_fi, "y_fi", (S, ld), torch.float64, dev)
    check_tensor(x_fi, "x_fi", (S, ld), torch.int64, dev)
    mask = which_mask(which)
    _prepare(nm, p_Xhat)
    L = _lib.load()
    info = torch.empty((3, ld), dtype=torch.float64, device=y_fi.device) if out is None else out
    check_tensor(info, "out", (3, ld), torch.float64, dev)
    current = torch.cuda.current_stream(y_fi.device)
    if stream is None:
        stream = current
    want_terms = terms is not False and terms is not None
    if want_terms:
        t = torch.empty((3, S, ld), dtype=torch.float64, device=y_fi.device) if terms is True else terms
        check_tensor(t, "terms", (3, S, ld), torch.float64, dev)
        d_terms, d_ws, ws_bytes = C.c_void_p(t.data_ptr()), None, 0
    else:
        need = C.c_size_t(0)
        check(L.qr_mi_workspace_size(int(ld), int(S), C.byref(need)), "mi_workspace_size")
        t = torch.empty((need.value,), dtype=torch.uint8, device=y_fi.device)
        d_terms, d_ws, ws_bytes = None, C.c_void_p(t.data_ptr()), need.value
    check(L.qr_mi_montecarlo_device(nm.handle, mask, int(B), int(ld), int(S), C.c_void_p(x_fi.data_ptr()),
                                    C.c_void_p(y_fi.data_ptr()), C.c_void_p(info.data_ptr()), d_terms, d_ws, ws_bytes,
                                    C.c_void_p(stream.cuda_stream)), "montecarlo_information_device")
    if stream != current:   # the buffer came from the current stream's pool: keep it until `stream` is done with it
        t.record_stream(stream)
    return (info[:, :B], t) if want_terms else info[:, :B]
