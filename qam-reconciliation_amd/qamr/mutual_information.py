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

``mutual_information_base_scheme`` (:123-148) and ``mutual_information_X_Y`` (:202-208) are
``scipy.integrate.quad`` over ``mutual_information_base_scheme_arg`` (:43-119) and
``mutual_information_X_Y_int_arg`` (:175-199).  Here the integrands run on the GPU and quad's integrator
(QUADPACK's QAGS / QAGI, restated operation by operation) on the host around them
(qr_mi_quad_batch): the floats returned are the reference's, the integrals it returns as ``-inf``
included.  ``mutual_information_quad_batch`` integrates many mappers / sign configurations in one call,
one launch per round of bisections; the ``_arg_array`` forms evaluate an integrand over an array.

``lappr_information`` and ``lappr_information_device`` are not the reference's: they estimate the rate the
per-bit LAPPRs carry to the bit-wise decoder (the BICM generalised mutual information), at several scales
alpha of the LAPPRs in one pass (qr_lappr_info_host / qr_lappr_info_device; DESIGN.md "LAPPR information rate").
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import bool_as_u8, check, check_2d, check_tensor, dptr, ptr, stream_arg

__all__ = ["P_xhat", "mutual_information_X_Xhat", "montecarlo_information", "montecarlo_information_device",
           "which_mask", "mutual_information_base_scheme_arg", "mutual_information_base_scheme_arg_array",
           "mutual_information_X_Y_int_arg", "mutual_information_X_Y_int_arg_array", "mutual_information_base_scheme",
           "mutual_information_X_Y", "mutual_information_quad_batch", "quad_batch_stats", "quad_host", "quad_rule",
           "lappr_information", "lappr_information_device", "LapprInformation"]

GRID_DEFAULTS = (1e-21, 1000)   # NoiseMapper's trunkation_threshold, n_intervals_per_step (noisemapper.pyx:103-105)
QUAD_KINDS = {"base": 0, "X_Y": 1}


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


def _check_pX(p_Xhat, M, what="p_Xhat"):
    pX = np.ascontiguousarray(np.asarray(p_Xhat, np.float64).ravel())
    if pX.size != M:
        raise ValueError(f"{what} has {pX.size} entries, the alphabet {M}")
    return pX


def _prepare(nm, p_Xhat):
    """Make the demapper handle ready for the estimator: the interpolation grid in HBM and the
    (p_Xhat, fwrd_transition_probability) tables; uploads only when p_Xhat changed."""
    pX = _check_pX(p_Xhat, nm.order)
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

    S, ld = check_2d(y_fi, "montecarlo_information_device", "y_fi", "[S, ld]")
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
    stream, sp = stream_arg(stream, y_fi.device)
    want_terms = terms is not False and terms is not None
    if want_terms:
        t = torch.empty((3, S, ld), dtype=torch.float64, device=y_fi.device) if terms is True else terms
        check_tensor(t, "terms", (3, S, ld), torch.float64, dev)
        d_terms, d_ws, ws_bytes = dptr(t), None, 0
    else:
        need = C.c_size_t(0)
        check(L.qr_mi_workspace_size(int(ld), int(S), C.byref(need)), "mi_workspace_size")
        t = torch.empty((need.value,), dtype=torch.uint8, device=y_fi.device)
        d_terms, d_ws, ws_bytes = None, dptr(t), need.value
    check(L.qr_mi_montecarlo_device(nm.handle, mask, int(B), int(ld), int(S), dptr(x_fi), dptr(y_fi), dptr(info), d_terms,
                                    d_ws, ws_bytes, sp), "montecarlo_information_device")
    if stream != current:   # the buffer came from the current stream's pool: keep it until `stream` is done with it
        t.record_stream(stream)
    return (info[:, :B], t) if want_terms else info[:, :B]


# ------------------------------------------------------------------ LAPPR information rate
LAPPR_INFO_CHUNK = 256        # QR_LAPPR_INFO_CHUNK (include/qamr.h): the symbols of one chunk sum
LAPPR_INFO_MAX_SCALES = 16
LAPPR_INFO_MAX_BPS = 8


def _check_info_args(bps, alphas):
    """bit_per_symbol in 1..8 and 1..16 finite scales, as the C-ABI requires them: (bps, float64 [A])."""
    if isinstance(bps, bool) or int(bps) != bps or not 1 <= int(bps) <= LAPPR_INFO_MAX_BPS:
        raise ValueError(f"bps must be an integer in 1..{LAPPR_INFO_MAX_BPS}, got {bps!r}")
    al = np.ascontiguousarray(np.asarray(alphas, np.float64).ravel())
    if not 1 <= al.size <= LAPPR_INFO_MAX_SCALES:
        raise ValueError(f"alphas must hold 1..{LAPPR_INFO_MAX_SCALES} scales, got {al.size}")
    if not np.all(np.isfinite(al)):
        raise ValueError("alphas must be finite")
    return int(bps), al


def _info_rates(total, B, S):
    """I_k(alpha) = 1.0 - total[a][k] / (B S) and I(alpha), their sum from 0.0 over ascending k (float64)."""
    total = np.asarray(total, np.float64)
    A, bps = total.shape
    n = float(int(B) * int(S))
    I_level = np.empty((A, bps), np.float64)
    I = np.empty(A, np.float64)
    for a in range(A):
        acc = 0.0
        for k in range(bps):
            v = 1.0 - float(total[a, k]) / n
            I_level[a, k] = v
            acc += v
        I[a] = acc
    return I, I_level


def lappr_information(lappr, word, bps, alphas=(1.0,), device=0):
    """The information rate one frame's LAPPRs carry to the bit-wise decoder (the BICM generalised mutual
    information, bits per symbol) at every scale of `alphas`: lappr float64 [S * bps] and word uint8
    [S * bps] (the bits the decoder must recover), element s * bps + k as the demappers return them ->
    (I float64 [A], I_level float64 [A, bps], errors int64 [bps]); errors[k] counts level k's hard-decision
    errors (count_errors_from_lappr's rule).  One synchronous host round trip (qr_lappr_info_host)."""
    bps, al = _check_info_args(bps, alphas)
    L = _lib.as_buffer(lappr, np.float64, name="lappr")
    w = _lib.as_buffer(word, np.uint8, name="word")
    if L.size != w.size:
        raise ValueError(f"lappr has {L.size} elements, word {w.size}")
    if L.size < bps or L.size % bps:
        raise ValueError(f"lappr has {L.size} elements: not a positive multiple of bps = {bps}")
    S = L.size // bps
    loss = np.empty((al.size, bps), np.float64)
    errors = np.empty(bps, np.int64)
    check(_lib.load().qr_lappr_info_host(int(device), bps, S, ptr(L), ptr(w), al.size, ptr(al), ptr(loss), ptr(errors)),
          "lappr_information")
    I, I_level = _info_rates(loss, 1, S)
    return I, I_level, errors


class LapprInformation:
    """What lappr_information_device wrote, on the device: loss float64 [A, bps, B] and errors int32
    [bps, B] (views of the frames [0, B) of their [.., ld] buffers), total float64 [A, bps] and
    total_errors int64 [bps]."""

    def __init__(self, loss, errors, total, total_errors, B):
        self.loss, self.errors, self.total, self.total_errors, self.B = loss, errors, total, total_errors, int(B)

    def rates(self, S):
        """-> host (I float64 [A], I_level float64 [A, bps], ber_level float64 [bps]) of a batch of S symbols
        per frame; synchronises with the launches."""
        total = self.total.cpu().numpy()
        terr = self.total_errors.cpu().numpy()
        I, I_level = _info_rates(total, self.B, S)
        ber = np.array([float(e) / float(self.B * int(S)) for e in terr], np.float64)
        return I, I_level, ber


def lappr_information_device(lappr_fi, word_fi, B, bps, alphas=(1.0,), stream=None):
    """B frames already in HBM, frame-innermost as the decoder takes them: lappr_fi float64 [S * bps, ld],
    word_fi uint8 [S * bps, ld], frame f in column f -> LapprInformation.  Two launches on `stream`
    (torch's current stream when None), asynchronous, every scale in one pass over the LAPPRs."""
    import torch

    bps, al = _check_info_args(bps, alphas)
    V, ld = check_2d(lappr_fi, "lappr_information_device", "lappr_fi", "[S * bps, ld]")
    if ld % 64 or not 0 < int(B) <= ld or V < bps or V % bps:
        raise ValueError(f"lappr_information_device: need ld % 64 == 0, 0 < B <= ld and a positive multiple of bps = {bps} "
                         f"rows (B={B}, ld={ld}, rows={V})")
    check_tensor(lappr_fi, "lappr_fi", (V, ld), torch.float64)
    dev = lappr_fi.device
    check_tensor(word_fi, "word_fi", (V, ld), torch.uint8, dev.index)
    S, A = V // bps, al.size
    L = _lib.load()
    need = C.c_size_t(0)
    check(L.qr_lappr_info_workspace_size(bps, int(ld), S, A, C.byref(need)), "lappr_info_workspace_size")
    current = torch.cuda.current_stream(dev)
    stream, sp = stream_arg(stream, dev)
    with torch.cuda.device(dev):
        ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)
        loss = torch.empty((A, bps, ld), dtype=torch.float64, device=dev)
        errors = torch.empty((bps, ld), dtype=torch.int32, device=dev)
        total = torch.empty((A, bps), dtype=torch.float64, device=dev)
        total_errors = torch.empty((bps,), dtype=torch.int64, device=dev)
        check(L.qr_lappr_info_device(bps, int(B), int(ld), S, dptr(lappr_fi), dptr(word_fi), A, ptr(al), dptr(loss),
                                     dptr(errors), dptr(total), dptr(total_errors), dptr(ws), need.value, sp),
              "lappr_information_device")
    if stream != current:   # the buffers came from the current stream's pool: keep them until `stream` is done with them
        for t in (ws, loss, errors, total, total_errors):
            t.record_stream(stream)
    return LapprInformation(loss[:, :, :B], errors[:, :B], total, total_errors, B)


# ------------------------------------------------------------------ quad-integrated evaluators
def _kind(kind) -> int:
    if kind in QUAD_KINDS:
        return QUAD_KINDS[kind]
    if kind in (0, 1) and not isinstance(kind, bool):
        return int(kind)
    raise ValueError(f"kind must be 'base' or 'X_Y' (0 or 1), got {kind!r}")


def _check_limit(limit) -> int:
    if int(limit) < 1:
        raise ValueError(f"limit must be at least 1, got {limit}")
    return int(limit)


QUAD_MESSAGES = {
    1: "The maximum number of subdivisions has been achieved.",
    2: "The occurrence of roundoff error is detected, which prevents the requested tolerance from being achieved.",
    3: "Extremely bad integrand behavior occurs at some points of the integration interval.",
    4: "The algorithm does not converge.  Roundoff error is detected in the extrapolation table.",
    5: "The integral is probably divergent, or slowly convergent.",
    6: "The input is invalid.",
}


def _warn(ier, abserr):
    """quad warns whenever QUADPACK's ier is not 0 (the reference does not silence it)."""
    if not ier:
        return
    import warnings

    try:
        from scipy.integrate import IntegrationWarning as category
    except Exception:
        category = UserWarning   # IntegrationWarning's base class
    warnings.warn(f"{QUAD_MESSAGES.get(int(ier), 'quad: ier = %d' % ier)}  The error may be underestimated "
                  f"(estimate {abserr!r}).", category, stacklevel=3)


def mutual_information_base_scheme_arg_array(n, nm, p_Xhat):
    """mutual_information_base_scheme_arg (:43-119) at every n: one launch (qr_mi_integrand_host)."""
    pX = _check_pX(p_Xhat, int(nm.order))
    n = np.ascontiguousarray(np.asarray(n, np.float64).ravel())
    out = np.empty(n.size, np.float64)
    if n.size:
        _prepare(nm, pX)
        check(_lib.load().qr_mi_integrand_host(nm.handle, 0, n.size, ptr(n), ptr(out)), "mutual_information_base_scheme_arg")
    return out


def mutual_information_base_scheme_arg(n, nm, p_Xhat):
    """mutual_information.pyx:43-119"""
    return float(mutual_information_base_scheme_arg_array(np.array([float(n)]), nm, p_Xhat)[0])


def mutual_information_X_Y_int_arg_array(y, nm):
    """mutual_information_X_Y_int_arg (:175-199) at every y: one launch (qr_mi_integrand_host)."""
    y = np.ascontiguousarray(np.asarray(y, np.float64).ravel())
    out = np.empty(y.size, np.float64)
    if y.size:
        nm._device_grid()
        check(_lib.load().qr_mi_integrand_host(nm.handle, 1, y.size, ptr(y), ptr(out)), "mutual_information_X_Y_int_arg")
    return out


def mutual_information_X_Y_int_arg(y, nm):
    """mutual_information.pyx:175-199"""
    return float(mutual_information_X_Y_int_arg_array(np.array([float(y)]), nm)[0])


def mutual_information_quad_batch(kind, nms, p_Xhats=None, sign_configs=None, *, epsabs=1.49e-8, epsrel=1.49e-8,
                                  limit=50, stream=None):
    """P integrals in one call: kind 'base' (mutual_information_base_scheme of nms[k], p_Xhats[k]) or 'X_Y'
    (mutual_information_X_Y of nms[k]); sign_configs [P][M] uint8, if given, replaces each mapper's own
    configuration (one NoiseMapper per noise variance then serves every configuration; a mapper may appear
    many times).  All mappers share one bit_per_symbol.  -> (I [P], abserr [P], neval [P], ier [P]); ier is
    QUADPACK's, non-zero where scipy's quad would warn.  No warning is raised here."""
    k = _kind(kind)
    limit = _check_limit(limit)
    nms = list(nms)
    P = len(nms)
    I, abserr = np.empty(P, np.float64), np.empty(P, np.float64)
    neval, ier = np.empty(P, np.int32), np.empty(P, np.int32)
    if P == 0:
        return I, abserr, neval, ier
    bps = int(nms[0].bit_per_symbol)
    M = 1 << bps
    for q, nm in enumerate(nms):
        if int(nm.bit_per_symbol) != bps:
            raise ValueError(f"the mappers of one batch must share bit_per_symbol (mapper {q} has {nm.bit_per_symbol}, "
                             f"mapper 0 {bps})")
    pX = None
    if k == 0:
        if p_Xhats is None:
            raise ValueError("the base-scheme integrals need p_Xhats")
        rows = list(p_Xhats)
        if len(rows) != P:
            raise ValueError(f"p_Xhats has {len(rows)} rows for {P} mappers")
        pX = np.ascontiguousarray(np.stack([_check_pX(r, M, f"p_Xhats[{q}]") for q, r in enumerate(rows)]))
    cfg = None
    if sign_configs is not None:
        cfg = bool_as_u8(sign_configs)
        if cfg.dtype != np.uint8 or cfg.shape != (P, M):   # rank 2: not as_buffer's 1-D or ravelled rule
            raise ValueError(f"sign_configs must be uint8 of shape ({P}, {M}), got {cfg.dtype} {cfg.shape}")
        cfg = np.ascontiguousarray(cfg)
    for nm in nms:
        nm._device_grid()
    handles = (C.c_void_p * P)(*[nm.handle for nm in nms])
    check(_lib.load().qr_mi_quad_batch(handles, None if pX is None else ptr(pX), None if cfg is None else ptr(cfg), P, k,
                                       float(epsabs), float(epsrel), limit, ptr(I), ptr(abserr), ptr(neval), ptr(ier),
                                       None if stream is None else stream_arg(stream, None)[1]),
          "mutual_information_quad_batch")
    return I, abserr, neval, ier


def quad_rule(kind, nm, a, b, p_Xhat=None, sign_config=None):
    """One work item of the batch's kernel with its debug output (qr_mi_quad_rule_host): the rule of each
    interval [a[h], b[h]] (one or two).  -> (sums [nh][4] = result, raw error, resabs, resasc;
    nodes [nh][21 or 30][2] = every lane's abscissa and integrand value).  For tests."""
    k = _kind(kind)
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(a, np.float64)))
    b = np.ascontiguousarray(np.atleast_1d(np.asarray(b, np.float64)))
    if a.shape != b.shape or a.ndim != 1 or a.size not in (1, 2):
        raise ValueError("a and b must hold the ends of one or two intervals")
    M = int(nm.order)
    pX = None if k == 1 else _check_pX(p_Xhat, M)
    cfg = None if sign_config is None else np.ascontiguousarray(np.asarray(sign_config, np.uint8).ravel())
    if cfg is not None and cfg.size != M:
        raise ValueError(f"sign_config has {cfg.size} entries, the alphabet {M}")
    nm._device_grid()
    sums = np.empty((a.size, 4), np.float64)
    nodes = np.empty((a.size, 30 if k == 1 else 21, 2), np.float64)
    check(_lib.load().qr_mi_quad_rule_host(nm.handle, None if pX is None else ptr(pX), None if cfg is None else ptr(cfg), k,
                                           a.size, ptr(a), ptr(b), ptr(sums), ptr(nodes)), "quad_rule")
    return sums, nodes


def quad_batch_stats():
    """Of this thread's last mutual_information_quad_batch: rounds, launches, work items, and the seconds of
    host bookkeeping and of the whole call."""
    out = (C.c_int64 * 5)()
    check(_lib.load().qr_mi_quad_stats(out), "quad_batch_stats")
    return {"rounds": int(out[0]), "launches": int(out[1]), "work_items": int(out[2]), "host_s": out[3] * 1e-9,
            "total_s": out[4] * 1e-9}


def mutual_information_base_scheme(nm, p_Xhat, *, epsabs=1.49e-8, epsrel=1.49e-8, limit=50):
    """mutual_information.pyx:123-148: quad(mutual_information_base_scheme_arg, 0, 1, args=(nm, p_Xhat))[0]; the
    keywords are quad's, at quad's defaults."""
    _check_limit(limit)
    pX = _check_pX(p_Xhat, int(nm.order))
    I, abserr, _, ier = mutual_information_quad_batch(0, [nm], [pX], epsabs=epsabs, epsrel=epsrel, limit=limit)
    _warn(int(ier[0]), float(abserr[0]))
    return float(I[0])


def mutual_information_X_Y(nm, *, epsabs=1.49e-8, epsrel=1.49e-8, limit=50):
    """mutual_information.pyx:202-208: quad(mutual_information_X_Y_int_arg, -inf, inf, args=(nm,))[0]."""
    _check_limit(limit)
    I, abserr, _, ier = mutual_information_quad_batch(1, [nm], epsabs=epsabs, epsrel=epsrel, limit=limit)
    _warn(int(ier[0]), float(abserr[0]))
    return float(I[0])


def quad_host(f, kind, a, b, *, epsabs=1.49e-8, epsrel=1.49e-8, limit=50):
    """The host integrator alone over a Python callable (qr_quad_host, no device call): kind 0 / 'base' is
    quad(f, a, b), kind 1 / 'X_Y' quad(f, -inf, inf).  -> (I, abserr, neval, ier, last).  For tests."""
    k = _kind(kind)
    limit = _check_limit(limit)
    L = _lib.load()
    cb = _lib.QUAD_FN(lambda x, _user: float(f(x)))
    I, abserr = C.c_double(0), C.c_double(0)
    neval, ier, last = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(L.qr_quad_host(cb, None, k, float(a), float(b), float(epsabs), float(epsrel), limit, C.byref(I), C.byref(abserr),
                         C.byref(neval), C.byref(ier), C.byref(last)), "quad_host")
    return I.value, abserr.value, neval.value, ier.value, last.value
