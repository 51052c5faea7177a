"""tests/workspace_fixture.py without a GPU: the restated layout of the decode workspace against
the closed form of its size, the in-range rule of the typed fill, and the helpers' own ability to
see a fault -- a fake "kernel" in plain numpy on host tensors that writes one byte past either end
of its workspace, or reads a workspace double before writing it.  No library is mutated and
nothing here runs on a GPU."""
import numpy as np
import pytest

from conftest import assert_bit_exact

import workspace_fixture as W
from decode_fixture import himix_code, small_code


def _closed_form(vid, cid, ld, max_it, repack):
    """The decode workspace's size from the code's counts, as tests/test_gpu_degrees.py stated it
    before it became the sum of the map: (bytes, fb_rows, iter_code)."""
    A = lambda n: -(-n // 256) * 256   # noqa: E731
    E, V, C = vid.size, int(vid.max()) + 1, int(cid.max()) + 1
    dc, dv = np.bincount(cid), np.bincount(vid)
    classes = np.unique(dc)
    fb_rows = int(sum(int((dc == d).sum()) * (int(d) - 2) for d in classes if d > 16))
    iter_code = len(classes) == 1 and 2 <= classes[0] <= 10 and dv.max() <= 64 and 8 * E * ld <= 1 << 30
    base = (A(8 * E * ld) * (2 if iter_code else 1) + A(ld) + A((max(max_it, 0) + 2) * ld) + A(8 * fb_rows * ld) +
            A(4 * ld) + 256)
    work_set = 3 * A(8 * V * ld) + 2 * A(C * ld) + A(8 * E * ld) + A(4 * ld)
    return base + (work_set if repack and ld % 512 == 0 else 0), fb_rows, iter_code


def _cases():
    """The five cases of tests/test_gpu_degrees.py::test_workspace_bytes_closed_form."""
    from qamr import codes
    from test_gpu_degrees import _high_degree_code

    high = _high_degree_code(np.random.default_rng(17))
    mixed = himix_code()
    return [(codes.regular_code(1008), 64), (codes.regular_code(1008), 512), (high, 128), (mixed, 512), (mixed, 64)]


def test_map_total_is_the_closed_form():
    seen = set()
    for (vid, cid), ld in _cases():
        for max_it in (0, 30):
            for repack in (1, 0):
                m = W.decode_ws_map(vid, cid, ld, max_it, repack)
                want, fb_rows, iter_code = _closed_form(vid, cid, ld, max_it, repack)
                assert W.map_bytes(m) == want, (vid.size, ld, max_it, repack)
                names = [e[0] for e in m]
                assert ("c2v2" in names) == iter_code and ("fb" in names) == (fb_rows > 0)
                assert ("fid" in names) == bool(repack and ld % 512 == 0)
                # ascending, 256-aligned, disjoint, no gap
                off = 0
                for name, o, n, kind in m:
                    assert o == off and o % 256 == 0 and n % 256 == 0 and n > 0, (name, o, n)
                    assert kind in ("f64", "flag", "index", "count")
                    off += n
                assert W.base_bytes(m) == _closed_form(vid, cid, ld, max_it, 0)[0]
                seen.update(names)
    assert seen == {"c2v", "c2v2", "active", "unsat", "fb", "alist", "counts", "post", "lappr0", "synd0", "lappr1",
                    "synd1", "c2v_alt", "fid"}


@pytest.mark.parametrize("ld", [64, 128, 512])
def test_typed_fill_is_in_range(ld):
    for vid, cid in (himix_code(), small_code("reg7"), small_code("mix12_16_5")):
        m = W.decode_ws_map(vid, cid, ld, 30, 1)
        host = W.typed_host(m, ld)
        assert host.size == W.map_bytes(m)
        W.assert_in_range(host, m, ld)
        for name in ("alist",) + (("fid",) if ld % 512 == 0 else ()):
            _, off, n, _ = W.entry(m, name)
            v = host[off:off + n].view(np.int32)
            assert v[0] == ld - 1 and v[63] == ld - 64 and v[-64] == ld - 1 and (v[:ld] != np.arange(ld)).any()
        c = host[W.entry(m, "counts")[1]:][:256].view(np.int32)
        assert c[:16].tolist() == [37, 37, 1, 0, 1, 64, 7, 3, 1, 1, 1, 64, 7, 3, 1, 1] and not c[16:].any()
    # and the rule itself sees a bad value
    bad = host.copy()
    bad[W.entry(m, "alist")[1]:][:4].view(np.int32)[0] = ld
    with pytest.raises(AssertionError):
        W.assert_in_range(bad, m, ld)
    bad = host.copy()
    bad[W.entry(m, "counts")[1]:][:256].view(np.int32)[5] = ld   # a RangeSel width past ld / 2
    if ld % 512 == 0:
        with pytest.raises(AssertionError):
            W.assert_in_range(bad, m, ld)


def test_guards_see_one_byte_past_either_end():
    need, guard = 4096 + 256, W.guard_bytes(64)
    assert guard == 65536 and W.guard_bytes(1024) == 16 * 8 * 1024
    for at in (None, need, -1):
        whole, view = W.guarded(need, guard, device="cpu")
        assert view.numel() == need and bool((whole[:guard] == W.GUARD_BYTE).all())
        mem = whole.numpy()[guard:]   # the fake kernel's pointer: the workspace's start
        mem[:need] = 0x11             # all of the workspace is its to write
        if at is None:
            W.assert_guards(whole, guard, need, "in bounds")
            continue
        whole.numpy()[guard + at] = 0x11
        with pytest.raises(AssertionError, match=f"offset {at} "):
            W.assert_guards(whole, guard, need, "one byte out")


def _fake_kernel(ws, x):
    """out = c2v[0] + x, then c2v[0] = x: it relies on "c2v == 0" without writing it first."""
    c2v = ws.numpy().view(np.float64)
    out = c2v[0] + x
    c2v[0] = x[0]
    return out


def test_fills_tell_a_stale_read():
    vid, cid = small_code("reg12")
    m = W.decode_ws_map(vid, cid, 64, 30, 1)
    need, guard = W.map_bytes(m), W.guard_bytes(64)
    x = np.array([1.5])
    ref = 0.0 + x
    whole, view = W.guarded(need, guard, device="cpu")
    W.fill(view, "zero")
    assert_bit_exact(_fake_kernel(view, x), ref)
    W.assert_guards(whole, guard, need, "zero")
    W.fill(view, "typed", m, 64)
    assert view.numpy()[:8].view(np.uint64)[0] == W.NAN_BITS
    with pytest.raises(AssertionError):
        assert_bit_exact(_fake_kernel(view, x), ref)
    # a leaked NaN of the fill is not the default NaN: it differs from an oracle's NaN by bits
    W.fill(view, "typed", m, 64)
    leak = view.numpy()[:8].view(np.float64).copy()
    assert np.isnan(leak[0]) and leak.view(np.uint64)[0] != np.array([np.nan]).view(np.uint64)[0]
    assert_bit_exact(leak, np.array([np.nan]))   # assert_bit_exact alone lets it stand for the oracle's NaN
    with pytest.raises(AssertionError):
        W.assert_no_fill_payload(leak, "leak")
    W.assert_no_fill_payload(np.array([np.nan, 1.0]), "clean")
    # "leftover": the donor's bytes, repeated over a longer view
    donor = whole[guard:guard + 1000].clone()
    donor[:] = 0x42
    donor[0] = 0x07
    W.fill(view, "leftover", donor=donor)
    got = view.numpy()
    assert got[0] == got[1000] == got[2000] == 0x07 and got[999] == 0x42 and (got != 0x07).sum() == need - -(-need // 1000)
    W.assert_guards(whole, guard, need, "leftover")
