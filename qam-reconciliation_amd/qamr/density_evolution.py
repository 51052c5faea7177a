"""Sampled (population) density evolution of a code ensemble on an empirical LLR density: whether a
degree distribution decodes a channel population -- the softened LAPPRs at a scale alpha, say -- within
T iterations, without building a graph or decoding a frame.  Not the reference's: include/qamr.h states
the definition ("sampled density evolution") and the GPU results are bit-exact against it
(csrc/density_evolution.hip; DESIGN.md "Density evolution").

    tables = DETables(*degree_tables(vid, cid))
    u = signed_population(lappr_fi, word_fi, B, alpha=0.7)
    r = evolve_device(u, tables, M=1 << 20, T=50, seed=0)
    r.first_zero(), r.error_rate()

Limitation: the bit levels are mixed i.i.d. over the variables (the usual BICM approximation); which
level sits on which variable of an irregular code is not modelled.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, check_2d, check_batch, check_tensor, dptr, ptr, stream_arg

__all__ = ["degree_tables", "DETables", "DEResult", "signed_population", "evolve_device", "evolve", "rnd"]

MAX_POPULATION = 1 << 30
MAX_ITERATIONS = 10000
_MASK = (1 << 64) - 1


def rnd(seed, t, phase, j, k, n):
    """The definition's random index in [0, n) (Python integers; the kernels compute the same)."""
    def mix(x):
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK
        return x ^ (x >> 31)

    ctr = (((int(t) * 4 + int(phase)) * (1 << 32) + int(j)) * 512 + int(k)) & _MASK
    z = mix((int(seed) + 0x9E3779B97F4A7C15 * (ctr + 1)) & _MASK)
    return ((z >> 32) * int(n)) >> 32


def degree_tables(vid, cid, vnum=None):
    """The three int32 tables of the code with edges (vid[e], cid[e]): edge_vdeg[e] and edge_cdeg[e], the
    degrees of edge e's variable and check (the edge perspective), and node_vdeg[v] for v in [0, vnum)
    (the node perspective; vnum defaults to max(vid) + 1, a variable without an edge has degree 0)."""
    vid = np.asarray(vid, np.int64).ravel()
    cid = np.asarray(cid, np.int64).ravel()
    if vid.size != cid.size or vid.size == 0:
        raise ValueError("vid and cid must hold the same positive number of edges")
    if vid.min() < 0 or cid.min() < 0:
        raise ValueError("negative node id")
    n = int(vid.max()) + 1 if vnum is None else int(vnum)
    if n <= int(vid.max()):
        raise ValueError(f"vnum = {n} does not cover variable {int(vid.max())}")
    node_vdeg = np.bincount(vid, minlength=n).astype(np.int32)
    cdeg = np.bincount(cid).astype(np.int32)
    return np.ascontiguousarray(node_vdeg[vid]), np.ascontiguousarray(cdeg[cid]), node_vdeg


def _table(a, name):
    a = np.asarray(a)
    if a.ndim != 1 or a.size < 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must be a non-empty 1-D integer array")
    if a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max:
        raise ValueError(f"{name} does not fit int32")
    return np.ascontiguousarray(a, np.int32)


class DETables:
    """An ensemble's degree tables in HBM (qr_de_tables): edge_vdeg and edge_cdeg of equal length (variable
    degrees 1..255, check degrees 2..255), node_vdeg (0..255).  Any tables may be given: a design needs no graph."""

    def __init__(self, edge_vdeg, edge_cdeg, node_vdeg, device=0):
        ev, ec, nv = _table(edge_vdeg, "edge_vdeg"), _table(edge_cdeg, "edge_cdeg"), _table(node_vdeg, "node_vdeg")
        if ev.size != ec.size:
            raise ValueError(f"edge_vdeg has {ev.size} entries, edge_cdeg {ec.size}")
        self.device, self.Ne, self.Nv = int(device), int(ev.size), int(nv.size)
        self._h = C.c_void_p()
        check(_lib.load().qr_de_tables_create(self.device, self.Ne, ptr(ev), ptr(ec), self.Nv, ptr(nv), C.byref(self._h)),
              "de_tables_create")

    @property
    def handle(self):
        return self._h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.load().qr_de_tables_destroy(h)


class DEResult:
    """What an evolution wrote: errors int64 [T + 1], v2c and c2v float64 [M] (device tensors from
    evolve_device, numpy arrays from evolve; v2c is None for T == 0)."""

    def __init__(self, errors, v2c, c2v, M):
        self.errors, self.v2c, self.c2v, self.M = errors, v2c, c2v, int(M)

    def _errors(self):
        e = self.errors
        return e if isinstance(e, np.ndarray) else e.cpu().numpy()   # synchronises with the launches

    def error_rate(self):
        """errors[t] / M, float64 [T + 1]."""
        return self._errors().astype(np.float64) / float(self.M)

    def first_zero(self):
        """The first iteration with no error, None if the count never reaches 0."""
        z = np.flatnonzero(self._errors() == 0)
        return int(z[0]) if z.size else None


def _check_evolve(M, T, seed):
    if isinstance(M, bool) or int(M) != M or not 1 <= int(M) <= MAX_POPULATION:
        raise ValueError(f"M must be an integer in [1, 2^30], got {M!r}")
    if isinstance(T, bool) or int(T) != T or not 0 <= int(T) <= MAX_ITERATIONS:
        raise ValueError(f"T must be an integer in [0, {MAX_ITERATIONS}], got {T!r}")
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) <= _MASK:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    return int(M), int(T), int(seed)


def signed_population(lappr_fi, word_fi, B, alpha=1.0, stream=None, out=None):
    """A batch as a channel population: lappr_fi float64 [rows, ld] and word_fi uint8 [rows, ld], frame-innermost
    as the decoder takes them -> u float64 [rows * B], u[r * B + f] = alpha * lappr[r, f] with its sign bit flipped
    where word[r, f] != 0 (u > 0: correct).  The padding columns are not read.  One launch, asynchronous."""
    import torch

    rows, ld = check_2d(lappr_fi, "signed_population", "lappr_fi", "[rows, ld]")
    check_batch(B, ld, "signed_population")
    if rows < 1 or rows * int(B) >= 1 << 31:
        raise ValueError(f"signed_population: need rows >= 1 and rows * B < 2^31 (rows={rows}, B={B})")
    alpha = float(alpha)
    if not math.isfinite(alpha):
        raise ValueError("signed_population: alpha must be finite")
    check_tensor(lappr_fi, "lappr_fi", (rows, ld), torch.float64)
    dev = lappr_fi.device
    check_tensor(word_fi, "word_fi", (rows, ld), torch.uint8, dev.index)
    current = torch.cuda.current_stream(dev)
    stream, sp = stream_arg(stream, dev)
    with torch.cuda.device(dev):
        u = torch.empty((rows * int(B),), dtype=torch.float64, device=dev) if out is None else out
        check_tensor(u, "out", (rows * int(B),), torch.float64, dev.index)
        check(_lib.load().qr_de_population_device(int(B), int(ld), int(rows), dptr(lappr_fi), dptr(word_fi), alpha, dptr(u),
                                                  sp), "signed_population")
    if out is None and stream != current:   # from the current stream's pool: keep it until `stream` is done with it
        u.record_stream(stream)
    return u


def evolve_device(u, tables, M, T, seed, stream=None):
    """T iterations of a population of M messages on the channel population u (float64 [Mu] on the tables'
    device) -> DEResult of device tensors.  1 + 3T launches on `stream` (torch's current stream when None),
    asynchronous, no early exit."""
    import torch

    M, T, seed = _check_evolve(M, T, seed)
    if not isinstance(tables, DETables):
        raise ValueError("evolve_device: tables must be a DETables")
    if not isinstance(u, torch.Tensor) or u.dim() != 1 or not 1 <= u.numel() < 1 << 31:
        raise ValueError("evolve_device: u must be a 1-D tensor of 1 .. 2^31 - 1 elements")
    check_tensor(u, "u", (u.numel(),), torch.float64, tables.device)
    dev = u.device
    current = torch.cuda.current_stream(dev)
    stream, sp = stream_arg(stream, dev)
    with torch.cuda.device(dev):
        v2c = torch.empty((M,), dtype=torch.float64, device=dev)
        c2v = torch.empty((M,), dtype=torch.float64, device=dev)
        errors = torch.empty((T + 1,), dtype=torch.int64, device=dev)
        check(_lib.load().qr_de_evolve_device(tables.handle, u.numel(), dptr(u), M, T, seed, dptr(v2c), dptr(c2v),
                                              dptr(errors), sp), "evolve_device")
    if stream != current:   # the buffers came from the current stream's pool: keep them until `stream` is done with them
        for t in (v2c, c2v, errors):
            t.record_stream(stream)
    return DEResult(errors, v2c if T > 0 else None, c2v, M)


def evolve(u, tables, M, T, seed, device=0):
    """The same on numpy arrays: u float64 [Mu], tables = (edge_vdeg, edge_cdeg, node_vdeg) as degree_tables
    returns them -> DEResult of numpy arrays.  One synchronous host round trip (qr_de_evolve_host)."""
    M, T, seed = _check_evolve(M, T, seed)
    u = _lib.as_buffer(u, np.float64, name="u")
    if not 1 <= u.size < 1 << 31:
        raise ValueError("evolve: u must hold 1 .. 2^31 - 1 elements")
    edge_vdeg, edge_cdeg, node_vdeg = tables
    ev, ec, nv = _table(edge_vdeg, "edge_vdeg"), _table(edge_cdeg, "edge_cdeg"), _table(node_vdeg, "node_vdeg")
    if ev.size != ec.size:
        raise ValueError(f"edge_vdeg has {ev.size} entries, edge_cdeg {ec.size}")
    v2c, c2v = np.empty(M, np.float64), np.empty(M, np.float64)
    errors = np.empty(T + 1, np.int64)
    check(_lib.load().qr_de_evolve_host(int(device), ev.size, ptr(ev), ptr(ec), nv.size, ptr(nv), u.size, ptr(u), M, T, seed,
                                        ptr(v2c), ptr(c2v), ptr(errors)), "evolve")
    return DEResult(errors, v2c if T > 0 else None, c2v, M)
