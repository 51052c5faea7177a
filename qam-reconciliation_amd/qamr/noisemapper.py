"""Drop-in ``NoiseMapper`` whose soft demap runs on the gfx950 kernels.

Mirrors qamreconciliation.noisemapper.NoiseMapper (noisemapper.pyx:102-559):
constructor signature, read-only tables and the hot-path methods
``demap_lappr_array`` / ``demap_lappr`` (the north-star entry point), plus the
Bob-side ``hard_decide_index`` / ``map_noise`` that produce its inputs.
The hot-path tables (F_Y_thresholds, delta_F_Y) come from libqamr's host code
with the scipy-exact erf; the remaining O(M^2) tables (transition
probabilities, bare LLRs, erf table) are small host-side numpy constructions
of noisemapper.pyx:166-235.

Batched device methods (torch tensors in HBM, frame-innermost layout):
``demap_device`` (fused with the LLR scaling alpha of reconciliation.pyx:144-145,
writing the decoder's input layout directly) and ``bob_map_device``.

The table-interpolated surface (``g_inv``, ``demap_noise``, noisemapper.pyx:295-307, 391-403)
and the formulation-1 demapper on it (``demap_lappr_simplified`` / ``_array``, :563-620,
batched: ``demap_simplified_device``) run on the interpolation grid in HBM, which libqamr
builds on their first use (``qr_demap_grid_create``), never in ``__init__``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import as_buffer, check, check_2d, check_batch, check_tensor, dptr, ptr, stream_arg
from .alphabet import PAMAlphabet


def _pair(n, j, size_message):
    """The (double, long) array pair of the reference's array methods, ravelled; equal sizes."""
    n = as_buffer(n, np.float64, flat=True)
    j = as_buffer(j, np.int64, flat=True)
    if n.size != j.size:
        raise ValueError(size_message)
    return n, j


def _frame_row(values, dtype, device):
    """One frame of S values laid along the frame axis as ONE row of S "frames" ([1, ld] in HBM, ld = S
    rounded up to 64, zero padded): the per-symbol maps are elementwise, so this is S lanes of work
    instead of 64 columns per symbol."""
    import torch

    v = torch.from_numpy(np.ascontiguousarray(np.asarray(values).ravel().astype(dtype, copy=False)))
    row = torch.zeros((1, max(64, -(-v.numel() // 64) * 64)), dtype=v.dtype, device=device)
    row[0, :v.numel()] = v.to(device)
    return row


def F_Z(z, mu, sigma):
    """noisemapper.pyx:66-79: the Gaussian CDF 0.5 (1 + erf((z - mu) / (sqrt(2) sigma))) at every
    z, with scipy's erf as the reference.  Off the hot path (a host helper)."""
    from scipy.special import erf

    z = as_buffer(z, np.float64, flat=True)
    return 0.5 * (1 + erf((z - float(mu)) / (math.sqrt(2) * float(sigma))))


def view_dist_cut(x):
    """noisemapper.pyx:82-98 (``__view_dist_cut``): every x clipped to the probability range,
    0 below 0, 1 from 1 on (NaN stays NaN, as the reference's comparisons leave it)."""
    x = as_buffer(x, np.float64, flat=True)
    return np.where(x < 0, 0.0, np.where(x >= 1, 1.0, x))


def host_tables(a, th, p, sigma, bps):
    """The O(M^2) host tables of NoiseMapper.__cinit__ (noisemapper.pyx:166-235),
    with C erf/log semantics: (fwrd_transition_probability, back_transition_probability,
    bare_llr_table, inf_erf_table)."""
    M = len(a)
    tmp = math.sqrt(2) * sigma
    fw = np.empty((M, M))
    for j in range(M):
        fw[j, 0] = 0.5 * (math.erf((th[1] - a[j]) / tmp) + 1)
        fw[j, M - 1] = 0.5 * (1 - math.erf((th[M - 1] - a[j]) / tmp))
        for i in range(1, M - 1):
            fw[j, i] = 0.5 * (math.erf((th[i + 1] - a[j]) / tmp) - math.erf((th[i] - a[j]) / tmp))
    back = np.empty((M, M))
    for i in range(M):
        t = 0.0   # the reference forms this sum again for every j: the same operations, the same value
        for k in range(M):
            t += p[k] * fw[k, i]
        for j in range(M):
            back[i, j] = p[j] * fw[j, i] / t
    bare = np.empty((M, bps))
    old = np.seterr(divide="ignore")
    try:
        for j in range(M):
            for k in range(bps):
                N = D = 0.0
                for i in range(M):
                    mi = i >> k
                    if (mi * (mi + 1)) & 3:
                        D += fw[j, i]
                    else:
                        N += fw[j, i]
                # libm's log, as the reference's (numpy's log is another routine: 1 ulp off in 15 entries of
                # the 256-PAM table at 10 dB), with C semantics for log(0) rather than math.log's ValueError
                q = float(np.float64(N) / np.float64(D)) if D != 0 else 0.0
                bare[j, k] = 1e300 if D == 0 else -math.inf if q == 0 else math.nan if q < 0 else math.log(q)
    finally:
        np.seterr(**old)
    ierf = np.empty((M, M))
    for j in range(M):
        ierf[0, j] = -1
        for i in range(1, M):
            ierf[i, j] = math.erf((th[i] - a[j]) / tmp)
    return fw, back, bare, ierf


class NoiseMapper:
    def __init__(self, pa: PAMAlphabet, noise_var: float, sign_config=None, trunkation_threshold: float = 1e-21,
                 n_intervals_per_step: int = 1000, device: int = 0):
        noise_var = float(noise_var)
        if noise_var <= 0:  # noisemapper.pyx:111-112
            raise ValueError(f"noise variance must be strictly positive, got {noise_var}")
        if sign_config is None:  # :115-120
            sc = np.zeros(pa.order, dtype=np.uint8)
        else:
            sc = as_buffer(sign_config, np.uint8, flat=True)
            if sc.size < pa.order:
                raise ValueError("Not enough data for a monotonicity sign configuration")
        self.sign_config = sc
        self.order = pa.order
        self.half_order = pa.order >> 1
        self.bit_per_symbol = pa.bit_per_symbol
        self.constellation = np.asarray(pa.constellation, np.float64)
        self.variance = pa.variance
        self.thresholds = np.asarray(pa.thresholds, np.float64)
        self.probabilities = np.ascontiguousarray(pa.probabilities, np.float64)
        self.noise_var = noise_var
        self.noise_sigma = math.sqrt(noise_var)
        self._device = int(device)
        self._trunc = float(trunkation_threshold)
        self._nips = int(n_intervals_per_step)
        self._step = pa.step

        a = np.ascontiguousarray(self.constellation)
        th = np.ascontiguousarray(self.thresholds)
        h = C.c_void_p()
        check(_lib.load().qr_demap_create(int(self.bit_per_symbol), ptr(a), ptr(self.probabilities), ptr(th),
                                          noise_var, ptr(sc), self._device, C.byref(h)), "NoiseMapper")
        self._h = h
        self.F_Y_thresholds = np.empty(self.order + 1, np.float64)
        self.delta_F_Y = np.empty(self.order, np.float64)
        check(_lib.load().qr_demap_tables(h, ptr(self.F_Y_thresholds), ptr(self.delta_F_Y)))
        self._host_tables()
        self._y_range = None
        self._F_Y = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib._lib is not None:
            _lib._lib.qr_demap_destroy(h)
            self._h = None

    # ------------------------------------------------- small host-side tables
    def _host_tables(self):
        (self.fwrd_transition_probability, self.back_transition_probability, self.bare_llr_table,
         self.inf_erf_table) = host_tables(self.constellation, self.thresholds, self.probabilities,
                                           self.noise_sigma, self.bit_per_symbol)

    def _grid(self):
        """Uniform-weighted F_Y on the interpolation grid (noisemapper.pyx:135-144,
        264-275); not on the hot path, built lazily with scipy's erf."""
        if self._y_range is None:
            from scipy.special import erf
            if self._trunc > 1.0:
                lo, hi = self.constellation[0] * 10, self.constellation[-1] * 10
            else:
                t = math.sqrt(-2.0 * math.log(self._trunc)) * self.noise_sigma
                hi, lo = self.constellation[-1] + t, self.constellation[0] - t
            n = int(math.ceil((hi - lo) * self._nips / self._step)) + 1
            y = np.linspace(lo, hi, n)
            den = math.sqrt(2) * self.noise_sigma
            res = 0.5 * (1 + erf((y - self.constellation[0]) / den))
            for i in range(1, self.order):
                res = res + 0.5 * (1 + erf((y - self.constellation[i]) / den))
            self._y_range, self._F_Y = y, res / self.order
        return self._y_range, self._F_Y

    @property
    def y_range(self):
        return np.array(self._grid()[0])

    @property
    def F_Y_values(self):
        return np.array(self._grid()[1])

    @property
    def handle(self):
        return self._h

    def bare_llr(self, symb):
        """noisemapper.pyx:423-432 (hard-reverse LLR table lookup)."""
        s = np.asarray(symb, np.int64)
        return np.ascontiguousarray(self.bare_llr_table[s].reshape(-1))

    def index_to_val(self, index):
        """noisemapper.pyx:362-370"""
        return self.constellation[np.asarray(index, np.int64)]

    # ------------------------------------- CDF and its inverse (GPU, scalar API)
    def F_Y(self, y):
        """noisemapper.pyx:264-275: the uniformly weighted mixture CDF at every y."""
        y = as_buffer(y, np.float64, flat=True)
        out = np.empty(y.size, np.float64)
        if y.size:
            check(_lib.load().qr_F_Y_host(self._h, y.size, ptr(y), ptr(out)), "F_Y")
        return out

    def g(self, y, i):
        """noisemapper.pyx:289-292: the transformed noise of sample y in decision region i."""
        return float(self.map_noise(np.array([float(y)]), np.array([int(i)], np.int64))[0])

    def g_inv_search(self, n_hat, i, y_accuracy=1e-9):
        """noisemapper.pyx:310-345: y with F_Y(y) = the target of (n_hat, i), by doubling
        bracket + bisection to width <= y_accuracy."""
        return float(self.demap_noise_search(np.array([float(n_hat)]), np.array([int(i)], np.int64),
                                             y_accuracy)[0])

    def demap_noise_search(self, n_hat, symb, y_accuracy=1e-9):
        """noisemapper.pyx:407-419: g_inv_search over arrays."""
        n_hat, symb = _pair(n_hat, symb, "Sizes do not match")
        out = np.empty(n_hat.size, np.float64)
        if n_hat.size:
            check(_lib.load().qr_g_inv_search_host(self._h, n_hat.size, ptr(n_hat), ptr(symb), float(y_accuracy),
                                                   ptr(out)), "g_inv_search")
        return out

    # ------------------------------------------------------- hot path (GPU)
    def demap_lappr_array(self, n, j):
        """noisemapper.pyx:544-559: LAPPRs [S*bps], out[s*bps + k] = Gray bit k of symbol s."""
        n, j = _pair(n, j, "Sizes of transformed noise vector and tx symbols do not match")
        out = np.empty(n.size * self.bit_per_symbol, np.float64)
        if n.size:
            check(_lib.load().qr_demap_host(self._h, n.size, ptr(n), ptr(j), ptr(out)), "demap_lappr_array")
        return out

    def demap_lappr(self, n, j):
        """noisemapper.pyx:450-540 for one symbol."""
        return self.demap_lappr_array(np.array([float(n)]), np.array([int(j)], np.int64))

    # ------------------------- table-interpolated g_inv and formulation 1 (GPU)
    def _device_grid(self):
        """The interpolation grid in HBM (noisemapper.pyx:135-144), created on first use of the
        interpolated methods (never in __init__); repeated calls cost one no-op C call."""
        check(_lib.load().qr_demap_grid_create(self._h, self._trunc, self._nips, float(self._step)), "grid")

    def grid_info(self):
        """(n_points, nondecreasing) of the device grid: noisemapper.pyx:142, and whether
        F_Y_values never decreases (the shortcut index search runs only then)."""
        self._device_grid()
        n, nd = C.c_int32(0), C.c_int32(0)
        check(_lib.load().qr_demap_grid_info(self._h, C.byref(n), C.byref(nd)), "grid_info")
        return int(n.value), bool(nd.value)

    def grid_tables(self):
        """(y_range, F_Y_values) as the device built them (equal to the properties' bits)."""
        n, _ = self.grid_info()
        y, F = np.empty(n, np.float64), np.empty(n, np.float64)
        check(_lib.load().qr_demap_grid_host(self._h, ptr(y), ptr(F)), "grid_host")
        return y, F

    def g_inv(self, n_hat, i):
        """noisemapper.pyx:295-307: y_hat by interpolation in the tabulated F_Y."""
        return float(self.demap_noise(np.array([float(n_hat)]), np.array([int(i)], np.int64))[0])

    def demap_noise(self, n_hat, symb):
        """noisemapper.pyx:391-403: g_inv over arrays."""
        n_hat, symb = _pair(n_hat, symb, "Sizes do not match")
        out = np.empty(n_hat.size, np.float64)
        if n_hat.size:
            self._device_grid()
            check(_lib.load().qr_g_inv_host(self._h, n_hat.size, ptr(n_hat), ptr(symb), ptr(out)), "g_inv")
        return out

    def demap_lappr_simplified_array(self, n, j):
        """noisemapper.pyx:605-620 ("Formulation 1"): LAPPRs [S*bps], out[s*bps + k] = Gray bit k
        of symbol s, from the interpolated g_inv."""
        n, j = _pair(n, j, "Sizes of transformed noise vector and tx symbols do not match")
        out = np.empty(n.size * self.bit_per_symbol, np.float64)
        if n.size:
            self._device_grid()
            check(_lib.load().qr_demap_simplified_host(self._h, n.size, ptr(n), ptr(j), ptr(out)),
                  "demap_lappr_simplified_array")
        return out

    def demap_lappr_simplified(self, n, j):
        """noisemapper.pyx:563-601 for one symbol."""
        return self.demap_lappr_simplified_array(np.array([float(n)]), np.array([int(j)], np.int64))

    # ----------------------------------------------- Bob side (GPU, batched)
    # Single-frame (reference-style) calls run one _frame_row through the batched kernels.
    def _bob_host(self, y):
        import torch

        S = np.size(y)
        dev = torch.device("cuda", self._device)
        xh, nh, w = self.bob_map_device(_frame_row(y, np.float64, dev), S)
        torch.cuda.synchronize(dev)
        # word rows k = Gray bit k of the row's symbol; symbol s's bits are s * bps + k
        return (xh[0, :S].cpu().numpy(), nh[0, :S].cpu().numpy(),
                np.ascontiguousarray(w[:, :S].cpu().numpy().T).ravel())

    def hard_decide_index(self, y_samples):
        """noisemapper.pyx:349-359"""
        return self._bob_host(y_samples)[0]

    def map_noise(self, y_samples, index):
        """noisemapper.pyx:373-388: n[j] = g(y[j], index[j])."""
        import torch

        S = np.size(y_samples)
        if S != np.size(index):
            raise ValueError("Input vectors sizes do not match")
        dev = torch.device("cuda", self._device)
        nh = self.map_noise_device(_frame_row(y_samples, np.float64, dev), _frame_row(index, np.int64, dev), S)
        torch.cuda.synchronize(dev)
        return nh[0, :S].cpu().numpy()

    def _check_rows(self, what, B, name, t, index_name=None, index=None):
        """The checks of every batched method on its float64 [S, ld] input (and the int64 one beside
        it, if any) -> (S, ld)."""
        import torch

        S, ld = check_2d(t, what, name, "[S, ld]")
        check_batch(B, ld, what)
        check_tensor(t, name, (S, ld), torch.float64, self._device)
        if index_name is not None:
            check_tensor(index, index_name, (S, ld), torch.int64, self._device)
        return S, ld

    def map_noise_device(self, y_fi, index_fi, B: int, stream=None):
        """y_fi float64 [S, ld], index_fi int64 [S, ld] -> n_hat float64 [S, ld]."""
        import torch

        S, ld = self._check_rows("map_noise_device", B, "y_fi", y_fi, "index_fi", index_fi)
        nh = torch.empty((S, ld), dtype=torch.float64, device=y_fi.device)
        check(_lib.load().qr_map_noise_device(self._h, int(B), int(ld), int(S), dptr(y_fi), dptr(index_fi), dptr(nh),
                                              stream_arg(stream, y_fi.device)[1]), "map_noise_device")
        return nh

    # ------------------------------------------------- device (HBM) batches
    def _demap_device(self, simplified, n_fi, j_fi, B, alpha, out, stream):
        import torch

        what = "demap_simplified_device" if simplified else "demap_device"
        S, ld = self._check_rows(what, B, "n_fi", n_fi, "j_fi", j_fi)
        if out is None:
            out = torch.empty((S * self.bit_per_symbol, ld), dtype=torch.float64, device=n_fi.device)
        check_tensor(out, "out", (S * self.bit_per_symbol, ld), torch.float64, self._device)
        L = _lib.load()
        if simplified:
            self._device_grid()
        entry = L.qr_demap_simplified_batch_device if simplified else L.qr_demap_batch_device
        check(entry(self._h, int(B), int(ld), int(S), dptr(n_fi), dptr(j_fi), float(alpha), dptr(out),
                    stream_arg(stream, n_fi.device)[1]), what)
        return out

    def demap_device(self, n_fi, j_fi, B: int, alpha: float = 1.0, out=None, stream=None):
        """n_fi float64 [S, ld], j_fi int64 [S, ld] -> LAPPRs float64 [S*bps, ld]
        (the decoder's frame-innermost input), scaled by alpha."""
        return self._demap_device(False, n_fi, j_fi, B, alpha, out, stream)

    def demap_simplified_device(self, n_fi, j_fi, B: int, alpha: float = 1.0, out=None, stream=None):
        """demap_device with the formulation-1 demapper (noisemapper.pyx:563-620): n_fi float64
        [S, ld], j_fi int64 [S, ld] -> LAPPRs float64 [S*bps, ld], scaled by alpha."""
        return self._demap_device(True, n_fi, j_fi, B, alpha, out, stream)

    def bob_map_device(self, y_fi, B: int, stream=None):
        """y_fi float64 [S, ld] -> (x_hat int64 [S, ld], n_hat float64 [S, ld], word uint8 [S*bps, ld])."""
        import torch

        S, ld = self._check_rows("bob_map_device", B, "y_fi", y_fi)
        dev = y_fi.device
        xh = torch.empty((S, ld), dtype=torch.int64, device=dev)
        nh = torch.empty((S, ld), dtype=torch.float64, device=dev)
        w = torch.zeros((S * self.bit_per_symbol, ld), dtype=torch.uint8, device=dev)
        check(_lib.load().qr_bob_map_device(self._h, int(B), int(ld), int(S), dptr(y_fi), dptr(xh), dptr(nh), dptr(w),
                                            stream_arg(stream, dev)[1]), "bob_map_device")
        return xh, nh, w


class NoiseDemapper(NoiseMapper):
    """Declared in noisemapper.pxd:89 with no extra behaviour."""
