"""Drop-in ``Decoder`` backed by the gfx950 sum-product kernels of libqamr.so.

Mirrors qamreconciliation.decoder.Decoder (decoder.pyx:92-455): same
constructor, properties, method names, argument order, return tuples and
exception types.  Differences (documented, stricter): input lengths are
validated (the reference reads out of bounds, decoder.pyx:441-455), and check
nodes of degree < 2 are rejected at construction (undefined behaviour in the
reference, decoder.pyx:135-141).

Besides the one-frame API, ``decode_batch`` (host arrays, frame-major) and
``decode_device`` (torch tensors resident in HBM, frame-innermost layout) decode
many independent frames per launch -- the path the benchmark measures.
``decode_frames_device`` takes frame-major tensors in HBM; it, ``decode`` and
``decode_batch`` run up to knob ``few_max`` frames node-parallel (a lane per check or
variable of one frame) instead of frame-parallel.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib
from ._lib import as_buffer, bool_as_u8, check, check_2d, check_batch, check_tensor, dptr, ptr, stream_arg


def _as_inout(a, dtype, name):
    """In/out buffers must be written in place: exact dtype, 1-D, contiguous."""
    if not isinstance(a, np.ndarray):
        raise ValueError(f"{name} must be a numpy array (written in place)")
    as_buffer(a, dtype, name=name, flat=True)   # the dtype rule and its message; the array itself is used
    if a.ndim != 1 or not a.flags.c_contiguous or not a.flags.writeable:
        raise ValueError(f"{name} must be a writeable 1-D C-contiguous array")
    return a


def _stream_key(stream) -> int:
    """The stream's handle as an integer (0 = the default stream)."""
    return stream_arg(stream, None)[1].value or 0


class Decoder:
    """``Decoder(e_to_v, e_to_c)`` -- Tanner graph given as an edge list."""

    def __init__(self, e_to_v, e_to_c, device: int = 0):
        vid = as_buffer(e_to_v, np.int64, name="e_to_v")
        cid = as_buffer(e_to_c, np.int64, name="e_to_c")
        L = _lib.load()
        h = C.c_void_p()
        check(L.qr_code_create(ptr(vid), ptr(cid), vid.size, cid.size, int(device), C.byref(h)), "Decoder")
        self._h = h
        self._device = int(device)
        v, c, e = C.c_int64(), C.c_int64(), C.c_int64()
        dc, dv = C.c_int32(), C.c_int32()
        check(L.qr_code_info(h, C.byref(v), C.byref(c), C.byref(e), C.byref(dc), C.byref(dv)))
        self._V, self._C, self._E = int(v.value), int(c.value), int(e.value)
        self.max_check_degree, self.max_var_degree = int(dc.value), int(dv.value)
        self._ws = OrderedDict()  # per-stream device workspaces of decode_device (LRU, capped)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib._lib is not None:
            _lib._lib.qr_code_destroy(h)
            self._h = None

    # ---------------------------------------------------------- properties
    @property
    def cnum(self):
        """Number of check nodes (decoder.pyx:157-160)"""
        return self._C

    @property
    def vnum(self):
        """Number of variable nodes (decoder.pyx:163-166)"""
        return self._V

    @property
    def ednum(self):
        """Number of edges (decoder.pyx:169-172)"""
        return self._E

    @property
    def handle(self):
        return self._h

    @property
    def device(self):
        return self._device

    # ------------------------------------------------------ syndrome checks
    def _check_nodes(self, values, synd, lappr: bool):
        """Every check against a hard word, or against sign(lappr): (flags uint8 [C], all satisfied)."""
        name = "lappr" if lappr else "word"
        v = as_buffer(values, np.float64 if lappr else np.uint8, name=name)
        s = as_buffer(synd, np.uint8, name="synd")
        if v.size != self._V:
            raise ValueError(f"Size of {name} does not match number of vnodes")
        if s.size != self._C:
            raise ValueError("Size of synd does not match number of cnodes")
        flags = np.empty(self._C, np.uint8)
        allok = C.c_uint8()
        L = _lib.load()
        entry = L.qr_check_lappr_host if lappr else L.qr_check_word_host
        check(entry(self._h, ptr(v), ptr(s), ptr(flags), C.byref(allok)), f"check_{name}")
        return flags, int(allok.value)

    def check_synd_node(self, check_node_index, word, synd):
        """decoder.pyx:190-209: ``parity ^ 1`` of one check for a hard word."""
        return int(self._check_nodes(word, synd, False)[0][int(check_node_index)])

    def check_word(self, word, synd):
        """decoder.pyx:220-232: 1 iff every check is satisfied by the hard word."""
        return self._check_nodes(word, synd, False)[1]

    def check_lappr(self, lappr, synd):
        """decoder.pyx:260-281: 1 iff sign(lappr) (< 0 -> bit 1) satisfies synd."""
        return self._check_nodes(lappr, synd, True)[1]

    # ------------------------------------------------------ node processing
    def process_var_node(self, node_index, lappr_data, check_to_var, var_to_check, updated_lappr):
        """decoder.pyx:301-319 (writes var_to_check and updated_lappr in place)."""
        l = as_buffer(lappr_data, np.float64, name="lappr_data")
        c2v = as_buffer(check_to_var, np.float64, name="check_to_var")
        v2c = _as_inout(var_to_check, np.float64, "var_to_check")
        upd = _as_inout(updated_lappr, np.float64, "updated_lappr")
        if l.size < self._V or upd.size < self._V or c2v.size < self._E or v2c.size < self._E:
            raise ValueError("message/LAPPR arrays are shorter than the graph")
        nodes = np.array([int(node_index)], np.int64)
        check(_lib.load().qr_process_var_nodes_host(self._h, ptr(nodes), 1, ptr(l), ptr(c2v), ptr(v2c), ptr(upd)),
              "process_var_node")

    def process_check_node(self, node_index, synd, check_to_var, var_to_check):
        """decoder.pyx:372-388 (writes check_to_var in place); returns 0."""
        s = as_buffer(synd, np.uint8, name="synd")
        c2v = _as_inout(check_to_var, np.float64, "check_to_var")
        v2c = as_buffer(var_to_check, np.float64, name="var_to_check")
        if s.size < self._C or c2v.size < self._E or v2c.size < self._E:
            raise ValueError("message/syndrome arrays are shorter than the graph")
        nodes = np.array([int(node_index)], np.int64)
        check(_lib.load().qr_process_check_nodes_host(self._h, ptr(nodes), 1, ptr(s), ptr(c2v), ptr(v2c)),
              "process_check_node")
        return 0

    # ---------------------------------------------------------------- decode
    def decode(self, lappr_data, synd, max_iterations):
        """decoder.pyx:441-455 -> (success, iterations, final_lappr)."""
        return self._decode(lappr_data, synd, max_iterations, False)

    def _decode(self, lappr_data, synd, max_iterations, layered):
        l = as_buffer(lappr_data, np.float64, name="lappr_data")
        s = as_buffer(synd, np.uint8, name="synd")
        if l.size != self._V:
            raise ValueError(f"lappr has {l.size} entries, the code has {self._V} variable nodes")
        if s.size != self._C:
            raise ValueError(f"synd has {s.size} entries, the code has {self._C} check nodes")
        succ, its, res = self._decode_batch(l[None, :], s[None, :], max_iterations, layered)
        return int(succ[0]), int(its[0]), res[0]

    def decode_batch(self, lappr, synd, max_iterations):
        """Decode B independent frames from host memory.

        lappr: float64 [B, V]; synd: uint8/bool [B, C].
        Returns (success uint8[B], iterations int32[B], final float64[B, V])."""
        return self._decode_batch(lappr, synd, max_iterations, False)

    def _decode_batch(self, lappr, synd, max_iterations, layered):
        l = np.ascontiguousarray(lappr)
        s = np.ascontiguousarray(bool_as_u8(synd))
        if l.dtype != np.float64 or s.dtype != np.uint8:
            raise ValueError("decode_batch expects float64 LAPPRs and uint8 syndromes")
        if l.ndim != 2 or s.ndim != 2 or l.shape[0] != s.shape[0]:
            raise ValueError("decode_batch expects lappr [B, V] and synd [B, C]")
        if l.shape[1] != self._V or s.shape[1] != self._C:
            raise ValueError("decode_batch: shape does not match the code")
        B = l.shape[0]
        out = np.empty_like(l)
        succ = np.empty(B, np.uint8)
        its = np.empty(B, np.int32)
        L = _lib.load()
        entry = L.qr_decode_layered_host if layered else L.qr_decode_host
        check(entry(self._h, B, ptr(l), ptr(s), int(max_iterations), ptr(out), ptr(succ), ptr(its)), "decode")
        return succ, its, out

    # ------------------------------------------------------- layered schedule
    def layers(self):
        """The layers of the layered schedule: (layer_of int32 [C], n_layers).  ``layer_of[c]`` is the
        smallest l >= 0 such that no check c' < c of layer l shares a variable with c; the schedule
        runs the checks by (layer_of[c], c)."""
        n = C.c_int32()
        layer_of = np.empty(self._C, np.int32)
        check(_lib.load().qr_code_layers(self._h, C.byref(n), ptr(layer_of)), "layers")
        return layer_of, int(n.value)

    def decode_layered(self, lappr_data, synd, max_iterations):
        """``decode`` with the layered (serial-check) schedule: the posteriors are updated after every
        check, in the order of ``layers()`` (include/qamr.h states the definition; the results are
        bit-exact against it).  -> (success, iterations, final_lappr)."""
        return self._decode(lappr_data, synd, max_iterations, True)

    def decode_layered_batch(self, lappr, synd, max_iterations):
        """``decode_batch`` with the layered schedule."""
        return self._decode_batch(lappr, synd, max_iterations, True)

    def layered_workspace_bytes(self, ld: int, max_iterations: int) -> int:
        n = C.c_size_t()
        check(_lib.load().qr_decode_layered_workspace_size(self._h, int(ld), int(max_iterations), C.byref(n)))
        return int(n.value)

    def decode_layered_device(self, lappr_fi, synd_fi, B: int, max_iterations: int, final_fi=None, success=None,
                              iters=None, stream=None):
        """``decode_device`` with the layered schedule: same tensors, same return, asynchronous on
        ``stream``; check degrees up to 16."""
        return self._decode_fi(True, lappr_fi, synd_fi, B, max_iterations, final_fi, success, iters, stream)

    # ------------------------------------------------------- device (HBM) API
    def workspace_bytes(self, ld: int, max_iterations: int) -> int:
        n = C.c_size_t()
        check(_lib.load().qr_decode_workspace_size(self._h, int(ld), int(max_iterations), C.byref(n)))
        return int(n.value)

    def decode_device(self, lappr_fi, synd_fi, B: int, max_iterations: int, final_fi=None, success=None,
                      iters=None, stream=None):
        """Decode B frames resident in HBM (torch tensors, frame-innermost).

        lappr_fi: float64 [V, ld]; synd_fi: uint8 [C, ld]; ld % 64 == 0, 0 < B <= ld.
        Returns (final_fi float64 [V, ld], success uint8 [B], iters int32 [B]).
        Every tensor must be contiguous and on this decoder's GPU (checked).
        Asynchronous on ``stream`` (default: torch's current stream).  The message
        workspace is kept per stream, so calls on different streams never share it."""
        return self._decode_fi(False, lappr_fi, synd_fi, B, max_iterations, final_fi, success, iters, stream)

    def _decode_fi(self, _layered, lappr_fi, synd_fi, B, max_iterations, final_fi, success, iters, stream):
        import torch

        what = "decode_layered_device" if _layered else "decode_device"
        V, ld = check_2d(lappr_fi, what, "lappr_fi", "[V, ld]")
        if V != self._V:
            raise ValueError(f"{what}: tensor shapes do not match the code")
        check_batch(B, ld, what)
        check_tensor(lappr_fi, "lappr_fi", (self._V, ld), torch.float64, self._device)
        check_tensor(synd_fi, "synd_fi", (self._C, ld), torch.uint8, self._device)
        final_fi, success, iters = self._outputs(what, B, lappr_fi, final_fi, "final_fi", (self._V, ld),
                                                 success, iters)
        stream, sp = stream_arg(stream, lappr_fi.device)
        L = _lib.load()
        need = self.layered_workspace_bytes(ld, max_iterations) if _layered else self.workspace_bytes(ld, max_iterations)
        ws = self._workspace(stream, need)
        entry = L.qr_decode_layered_device if _layered else L.qr_decode_batch_device
        check(entry(self._h, int(B), int(ld), dptr(lappr_fi), dptr(synd_fi), int(max_iterations), dptr(final_fi),
                    dptr(success), dptr(iters), dptr(ws), ws.numel(), sp), what)
        return final_fi, success, iters

    def _outputs(self, what, B, lappr, final, final_name, final_shape, success, iters):
        """The outputs of a device decode, allocated beside `lappr` where not given, and checked:
        (final float64 of final_shape, success uint8 [>= B], iters int32 [>= B])."""
        import torch

        if final is None:
            final = torch.empty_like(lappr)
        if success is None:
            success = torch.empty(B, dtype=torch.uint8, device=lappr.device)
        if iters is None:
            iters = torch.empty(B, dtype=torch.int32, device=lappr.device)
        check_tensor(final, final_name, final_shape, torch.float64, self._device)
        if success.numel() < B or iters.numel() < B:
            raise ValueError(f"{what}: success/iters must hold at least B={B} entries")
        check_tensor(success, "success", (success.numel(),), torch.uint8, self._device)
        check_tensor(iters, "iters", (iters.numel(),), torch.int32, self._device)
        return final, success, iters

    def frames_workspace_bytes(self, B: int, max_iterations: int) -> int:
        n = C.c_size_t()
        check(_lib.load().qr_decode_frames_workspace_size(self._h, int(B), int(max_iterations), C.byref(n)))
        return int(n.value)

    def decode_frames_device(self, lappr, synd, max_iterations: int, final=None, success=None, iters=None,
                             stream=None):
        """Decode B frames resident in HBM (torch tensors, frame-major).

        lappr: float64 [B, V]; synd: uint8 [B, C]; any B >= 1.
        Returns (final float64 [B, V], success uint8 [B], iters int32 [B]).
        Every tensor must be contiguous and on this decoder's GPU (checked).  Up to knob
        ``few_max`` frames of a code with check degrees 2..16 run the few-frame schedule on
        these arrays as they are; other calls go through the frame-innermost decode
        (transposed inside the workspace).  Asynchronous on ``stream`` (default: torch's
        current stream), workspace per stream as ``decode_device``."""
        import torch

        if not isinstance(lappr, torch.Tensor) or lappr.dim() != 2 or lappr.shape[0] < 1:
            raise ValueError("decode_frames_device: lappr must be a 2-D tensor [B, V] with B >= 1")
        B = int(lappr.shape[0])
        check_tensor(lappr, "lappr", (B, self._V), torch.float64, self._device)
        check_tensor(synd, "synd", (B, self._C), torch.uint8, self._device)
        rows = B
        if final is not None:   # any number of rows from B up
            if not isinstance(final, torch.Tensor) or final.dim() != 2 or final.shape[0] < B:
                raise ValueError(f"decode_frames_device: final must hold at least B={B} rows of V")
            rows = final.shape[0]
        final, success, iters = self._outputs("decode_frames_device", B, lappr, final, "final", (rows, self._V),
                                              success, iters)
        stream, sp = stream_arg(stream, lappr.device)
        ws = self._workspace(stream, self.frames_workspace_bytes(B, max_iterations))
        check(_lib.load().qr_decode_frames_device(self._h, B, dptr(lappr), dptr(synd), int(max_iterations), dptr(final),
                                                  dptr(success), dptr(iters), dptr(ws), ws.numel(), sp),
              "decode_frames_device")
        return final, success, iters

    def repack_stats(self, ld: int, max_iterations: int, stream=None):
        """Column repack of the last decode_device on ``stream`` (same ld, max_iterations):
        ((repacks of range 0, repacks of range 1), (final width 0, final width 1)).  Waits
        for the device (a synchronous copy); call after the decode has completed."""
        import torch

        ws = self._ws.get(_stream_key(stream_arg(stream, torch.device("cuda", self._device))[0]))
        if ws is None:
            raise ValueError("repack_stats: no decode_device has run on this stream")
        out = (C.c_int32 * 4)()
        check(_lib.load().qr_decode_repack_stats(self._h, int(ld), int(max_iterations), dptr(ws), ws.numel(), out),
              "repack_stats")
        return (int(out[0]), int(out[1])), (int(out[2]), int(out[3]))

    #: how many per-stream workspaces a Decoder keeps (each is E*ld*8 bytes of messages)
    max_workspaces = 2

    def _workspace(self, stream, need: int):
        """Device workspace (c2v messages, flags) of the decodes issued on `stream`.
        Allocated on that stream, so torch's caching allocator orders its reuse after
        the work queued there; one per stream, so concurrent decodes never race.
        Keyed by the stream handle: torch's streams come from a per-device pool and
        live as long as the process, so a handle always names the same stream.  At
        most ``max_workspaces`` are kept (least recently used dropped first): a dropped
        workspace goes back to the caching allocator, which hands its memory out again
        only after the work already queued on its stream."""
        import torch

        key = _stream_key(stream)
        ws = self._ws.pop(key, None)
        if ws is None or ws.numel() < need:
            ws = None  # free the smaller one before allocating
            while len(self._ws) >= max(1, int(self.max_workspaces)):
                self._ws.popitem(last=False)
            with torch.cuda.stream(stream):
                ws = torch.empty(need, dtype=torch.uint8, device=torch.device("cuda", self._device))
        self._ws[key] = ws
        return ws
