"""The memory contract of the entries that take a caller's workspace (include/qamr.h): nothing is
written outside the bytes the library asked for, and nothing the workspace holds on entry reaches a
result.  Shared by tests/test_workspace_cpu.py (no GPU) and tests/test_gpu_workspace_contract.py.

* ``guarded`` / ``assert_guards``: one allocation of guard + need + guard bytes, both guards 0xC3,
  compared in full after the run.  The caching allocator rounds every block up and places its
  neighbours wherever it likes, so an overrun of a plain ``torch.empty`` workspace hits nothing a
  test looks at; here it hits a guard.
* ``decode_ws_map``: the layout of the decode workspace (csrc/decoder.hip ws_layout) restated as
  an ordered list of (name, offset, nbytes, kind).  tests/test_gpu_degrees.py holds its total to
  ``Decoder.workspace_bytes`` and tests/test_workspace_cpu.py to the closed form, so a drifted map
  fails there.  That cross-check is by size: it does NOT catch two equal-sized arrays swapped (the
  two column sets ``lappr0`` / ``lappr1`` and ``synd0`` / ``synd1``, ``post`` against a ``lappr``,
  ``alist`` against ``fid``); those pairs also share a kind, so a swap changes no fill.
* ``fill``: what the workspace holds when the call starts.
    "zero"      0x00, the memory a first decode usually sees;
    "typed"     per array of the map: f64 the quiet NaN 0x7FF8_0000_DEAD_0001 (a leak into an
                output fails assert_bit_exact wherever the oracle's value is no NaN, and
                ``assert_no_fill_payload``, since it is not the default NaN, where it is one), flags 0xFF,
                indices ld - 1 - (i % 64) (a valid column, and a wrong one), the count block
                counts 37, finite 1, each RangeSel on = 1, w = 64, repacks = 7, arrive = 3, buf = 1,
                transit = 1;
    "leftover"  no synthetic value: the bytes another call left in ITS workspace (another case or
                shape, another max_iterations, so another layout), copied over the view from the
                start and repeated when the donor's workspace is the shorter one.
  The rule of every fill: no value is an out-of-range index, width or count under the map, so a
  stale read shows as a wrong result and never as a wild address.  ``assert_in_range`` holds the
  host copy of a typed fill to that before it is uploaded.  The RangeSel width 64 lies in
  [64, ld / 2] wherever the two-stream schedule (the only reader of a width) can run, ld % 512 == 0;
  at a narrower ld it is asserted to be at most ld.  Where the layout cannot be cross-checked by
  size (the few-frame route: frames_workspace_bytes is a maximum over two routes; npstream: its
  prefix counts become ranks and store slots) only "zero" and "leftover" are used.
* ``decode_raw`` / ``frames_raw`` / ``repack_stats_raw``: qr_decode_batch_device,
  qr_decode_frames_device and qr_decode_repack_stats on the caller's workspace view
  (Decoder.decode_device sizes and owns its workspace).  ``final`` is pre-filled with
  decode_fixture.PAD, ``success`` / ``iters`` carry 64 extra entries of a sentinel that must
  survive, and the inputs are compared bit for bit with clones taken before the call.
"""
import ctypes as C

import numpy as np

from conftest import assert_bit_exact

GUARD_BYTE = 0xC3
NAN_BITS = 0x7FF80000DEAD0001
SENT_SUCC, SENT_ITERS = 0xEE, -77
EXTRA = 64
# the count block (csrc/decoder.hip DecodeWs::acount, csrc/decode_dev.hpp RangeSelField)
SEL_FIELDS = ("on", "w", "repacks", "arrive", "buf", "transit")
TYPED_SEL = dict(on=1, w=64, repacks=7, arrive=3, buf=1, transit=1)
TYPED_COUNT = 37
FILLS = ("zero", "typed", "leftover")


def A256(n):
    return -(-int(n) // 256) * 256


# ------------------------------------------------------------------ guards
def guard_bytes(ld):
    """A multiple of 256, at least max(65536, 16 * 8 * ld): 16 stray rows of doubles land in it."""
    return A256(max(65536, 16 * 8 * int(ld)))


def guarded(need, guard, device="cuda"):
    """(whole, view): one uint8 allocation of guard + need + guard bytes, both guards 0xC3, and the
    256-aligned view [guard, guard + need) of it.  device="cpu": a host tensor (the CPU tests)."""
    import torch

    assert guard % 256 == 0 and guard >= 65536 and need > 0
    total = guard + need + guard
    raw = torch.empty(total + 256, dtype=torch.uint8, device=device)   # a host allocation is only 64-aligned
    skip = -raw.data_ptr() % 256
    whole = raw[skip:skip + total]
    whole[:guard] = GUARD_BYTE
    whole[guard + need:] = GUARD_BYTE
    view = whole[guard:guard + need]
    assert whole.data_ptr() % 256 == 0 and view.data_ptr() % 256 == 0
    return whole, view


def assert_guards(whole, guard, need, tag):
    """Both guards hold 0xC3 in every byte (after the device has finished)."""
    import torch

    if whole.is_cuda:
        torch.cuda.synchronize()
    assert whole.numel() == guard + need + guard
    for name, part, at in (("front", whole[:guard], 0), ("back", whole[guard + need:], guard + need)):
        bad = torch.nonzero(part != GUARD_BYTE).flatten()
        assert bad.numel() == 0, (f"{tag}: {int(bad.numel())} bytes of the {name} guard were written, the first at "
                                  f"offset {int(bad[0]) + at - guard} from the workspace's start (it is {need} bytes long)")


# ------------------------------------------------------------------ the decode workspace's layout
def graph_counts(vid, cid):
    """(E, V, C, fb_rows, iter_code at 8 E ld <= 2^30) of a graph, as csrc/decoder.hip reads them."""
    E, V, Cn = int(vid.size), int(vid.max()) + 1, int(cid.max()) + 1
    dc, dv = np.bincount(cid), np.bincount(vid)
    classes = np.unique(dc[dc > 0])
    fb_rows = int(sum(int((dc == d).sum()) * (int(d) - 2) for d in classes if d > 16))   # runtime-degree classes
    small = len(classes) == 1 and 2 <= classes[0] <= 10 and dv.max() <= 64
    return E, V, Cn, fb_rows, small


def decode_ws_map(vid, cid, ld, max_it, repack):
    """The decode workspace at leading dimension ld, in order: [(name, offset, nbytes, kind)], every
    array rounded up to 256 bytes (nbytes is the rounded size; the last bytes of an array whose
    size is no multiple of 256 are slack of its kind).  kind: "f64", "flag" (u8), "index" (int32
    column or frame id below ld), "count" (the 256-byte count block: counts[0..1], finite[2],
    rsel[4..16)).  ``repack``: the work set follows the base part (knob repack on and
    ld % 512 == 0).  See the module docstring for what the size cross-check cannot see."""
    E, V, Cn, fb_rows, small = graph_counts(vid, cid)
    iter_code = bool(small and 8 * E * ld <= 1 << 30)
    arrays = [("c2v", 8 * E * ld, "f64")]
    if iter_code:
        arrays.append(("c2v2", 8 * E * ld, "f64"))
    arrays += [("active", ld, "flag"), ("unsat", (max(max_it, 0) + 2) * ld, "flag")]
    if fb_rows:
        arrays.append(("fb", 8 * fb_rows * ld, "f64"))
    arrays += [("alist", 4 * ld, "index"), ("counts", 256, "count")]
    if repack and ld % 512 == 0:
        arrays += [("post", 8 * V * ld, "f64"), ("lappr0", 8 * V * ld, "f64"), ("synd0", Cn * ld, "flag"),
                   ("lappr1", 8 * V * ld, "f64"), ("synd1", Cn * ld, "flag"), ("c2v_alt", 8 * E * ld, "f64"),
                   ("fid", 4 * ld, "index")]
    out, off = [], 0
    for name, n, kind in arrays:
        out.append((name, off, A256(n), kind))
        off += A256(n)
    return out


def map_bytes(m):
    return sum(n for _, _, n, _ in m)


def base_bytes(m):
    """Bytes of the base part: everything up to and including the count block."""
    k = [name for name, _, _, _ in m].index("counts")
    return m[k][1] + m[k][2]


def entry(m, name):
    return next(e for e in m if e[0] == name)


# ------------------------------------------------------------------ fills
def typed_host(m, ld):
    """The typed fill of a map as a host uint8 array of map_bytes(m)."""
    buf = np.zeros(map_bytes(m), np.uint8)
    for name, off, n, kind in m:
        part = buf[off:off + n]
        if kind == "f64":
            part.view(np.uint64)[:] = NAN_BITS
        elif kind == "flag":
            part[:] = 0xFF
        elif kind == "index":
            i = np.arange(n // 4)
            part.view(np.int32)[:] = ld - 1 - (i % 64)
        else:
            assert kind == "count" and n == 256
            c = part.view(np.int32)
            c[:] = 0
            c[0] = c[1] = TYPED_COUNT
            c[2] = 1
            for k in range(2):
                c[4 + 6 * k:10 + 6 * k] = [TYPED_SEL[f] for f in SEL_FIELDS]
    return buf


def assert_in_range(buf, m, ld):
    """The rule of every fill on a host copy: every int32 of an index array lies in [0, ld), the
    counts in [0, ld], the finite flag and the RangeSel flags in {0, 1}, every RangeSel width in
    [64, ld / 2] where the two-stream schedule can run (ld % 512 == 0) and in [1, ld] elsewhere,
    every double of an f64 array is the NaN pattern (a value, never an address)."""
    for name, off, n, kind in m:
        part = buf[off:off + n]
        if kind == "index":
            v = part.view(np.int32)
            assert ((v >= 0) & (v < ld)).all(), (name, int(v.min()), int(v.max()), ld)
        elif kind == "count":
            c = part.view(np.int32)
            assert 0 <= c[0] <= ld and 0 <= c[1] <= ld and c[2] in (0, 1), c[:4]
            for k in range(2):
                sel = dict(zip(SEL_FIELDS, c[4 + 6 * k:10 + 6 * k].tolist()))
                lo, hi = (64, ld // 2) if ld % 512 == 0 else (1, ld)
                assert lo <= sel["w"] <= hi, (sel, ld)
                assert sel["on"] in (0, 1) and sel["buf"] in (0, 1) and sel["transit"] in (0, 1), sel
                assert sel["repacks"] >= 0 and 0 <= sel["arrive"] <= 4096, sel
        elif kind == "f64":
            assert (part.view(np.uint64) == NAN_BITS).all(), name


def fill(view, how, map=None, ld=None, donor=None):
    """Prepare the workspace view (see the module docstring).  "typed" needs the map and ld and
    covers the first map_bytes(map) bytes (the view may be exactly that long, or shorter when the
    decode is handed the base part only); "leftover" needs ``donor``, the workspace view another
    call has just finished with."""
    import torch

    assert how in FILLS, how
    if how == "zero":
        view.zero_()
    elif how == "typed":
        host = typed_host(map, ld)
        assert_in_range(host, map, ld)
        assert view.numel() <= host.size
        view.copy_(torch.from_numpy(host[:view.numel()]).to(view.device))
    else:
        assert donor is not None and donor.numel() > 0
        if donor.is_cuda:
            torch.cuda.synchronize()
        for at in range(0, view.numel(), donor.numel()):
            n = min(donor.numel(), view.numel() - at)
            view[at:at + n] = donor[:n]


# ------------------------------------------------------------------ raw calls
def _stream_ptr():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def outputs(shape, B):
    import torch

    from decode_fixture import PAD

    fin = torch.full(shape, PAD, dtype=torch.float64, device="cuda")
    succ = torch.full((B + EXTRA,), SENT_SUCC, dtype=torch.uint8, device="cuda")
    its = torch.full((B + EXTRA,), SENT_ITERS, dtype=torch.int32, device="cuda")
    return fin, succ, its


def assert_sentinels(succ, its, B, tag):
    assert bool((succ[B:] == SENT_SUCC).all()) and bool((its[B:] == SENT_ITERS).all()), \
        f"{tag}: success / iters were written past their B entries"


def assert_no_fill_payload(a, tag):
    """No double of an output is the typed fill's NaN: conftest.assert_bit_exact lets any NaN stand
    for a NaN of the reference, so a leak into a place where the oracle has a NaN too (the frames
    that carry special values) needs this comparison of the payload."""
    bits = np.ascontiguousarray(a, np.float64).view(np.uint64)
    n = int((bits == NAN_BITS).sum())
    assert n == 0, f"{tag}: {n} output values carry the workspace fill's NaN payload"


def assert_inputs_intact(pairs, tag):
    """[(tensor, clone taken before the call)]: equal bit for bit."""
    import torch

    for k, (t, c) in enumerate(pairs):
        a = t.view(torch.int64) if t.dtype == torch.float64 else t
        b = c.view(torch.int64) if c.dtype == torch.float64 else c
        assert torch.equal(a, b), f"{tag}: input {k} was modified"


def decode_call(dec, L, S, B, mi, view, fin, succ, its, stream=None):
    """qr_decode_batch_device on the caller's workspace view, nothing else (capturable)."""
    from qamr import _lib
    from qamr._lib import dptr

    ld = L.shape[1]
    _lib.check(_lib.load().qr_decode_batch_device(dec.handle, int(B), int(ld), dptr(L), dptr(S), int(mi), dptr(fin),
                                                  dptr(succ), dptr(its), dptr(view), view.numel(),
                                                  stream or _stream_ptr()), "decode_raw")


def repack_stats_raw(dec, ld, mi, view):
    from qamr import _lib
    from qamr._lib import dptr

    out = (C.c_int32 * 4)()
    _lib.check(_lib.load().qr_decode_repack_stats(dec.handle, int(ld), int(mi), dptr(view), view.numel(), out),
               "repack_stats_raw")
    return (int(out[0]), int(out[1])), (int(out[2]), int(out[3]))


def decode_raw(dec, L, S, B, mi, whole, view, guard, ref, tag):
    """One qr_decode_batch_device of the frame-innermost L [V, ld], S [C, ld] on ``view`` (already
    filled): success, iterations and final LAPPRs of the B frames equal ``ref`` (the oracle's), the
    padding columns of final keep PAD, the 64 extra success / iters entries their sentinels, the
    inputs their bits, both guards theirs.  Returns the repack stats read from the view."""
    import torch

    from decode_fixture import PAD

    s2, i2, f2 = ref
    fin, succ, its = outputs(tuple(L.shape), B)
    Lc, Sc = L.clone(), S.clone()
    decode_call(dec, L, S, B, mi, view, fin, succ, its)
    torch.cuda.synchronize()
    assert_guards(whole, guard, view.numel(), tag)
    assert_inputs_intact([(L, Lc), (S, Sc)], tag)
    assert_sentinels(succ, its, B, tag)
    assert bool((fin[:, B:] == PAD).all()), f"{tag}: padding columns of final were written"
    assert np.array_equal(succ[:B].cpu().numpy(), s2[:B]), tag
    assert np.array_equal(its[:B].cpu().numpy(), i2[:B]), tag
    assert_bit_exact(fin[:, :B].cpu().numpy().T, f2[:B])
    assert_no_fill_payload(fin.cpu().numpy(), tag)
    return repack_stats_raw(dec, L.shape[1], mi, view)


def frames_raw(dec, llr, synd, mi, whole, view, guard, ref, tag):
    """One qr_decode_frames_device of the frame-major host arrays llr [B, V], synd [B, C] on
    ``view``; the output has one extra row of PAD.  The assertions of decode_raw."""
    import torch

    from decode_fixture import PAD
    from qamr import _lib
    from qamr._lib import dptr

    B = llr.shape[0]
    s2, i2, f2 = ref
    L = torch.from_numpy(np.array(llr)).cuda()
    S = torch.from_numpy(np.array(synd)).cuda()
    fin, succ, its = outputs((B + 1, llr.shape[1]), B)
    Lc, Sc = L.clone(), S.clone()
    _lib.check(_lib.load().qr_decode_frames_device(dec.handle, B, dptr(L), dptr(S), int(mi), dptr(fin), dptr(succ),
                                                   dptr(its), dptr(view), view.numel(), _stream_ptr()), "frames_raw")
    torch.cuda.synchronize()
    assert_guards(whole, guard, view.numel(), tag)
    assert_inputs_intact([(L, Lc), (S, Sc)], tag)
    assert_sentinels(succ, its, B, tag)
    assert bool((fin[B] == PAD).all()), f"{tag}: the extra row of final was written"
    assert np.array_equal(succ[:B].cpu().numpy(), s2[:B]), tag
    assert np.array_equal(its[:B].cpu().numpy(), i2[:B]), tag
    assert_bit_exact(fin[:B].cpu().numpy(), f2[:B])
    assert_no_fill_payload(fin.cpu().numpy(), tag)
