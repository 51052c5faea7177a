"""numpy's legacy global stream continued on the GPU (csrc/npstream.hip).

The reference draws every frame from ``np.random``'s global MT19937 stream
(sims/reconciliation.pyx:129-132: ``np.random.choice(M, size=S, p=p)``, then
``np.random.randn(S)``).  A ``NumpyStream`` starts at a state of that stream, by default
``np.random.get_state()``, and hands out on the device the words, doubles, symbols and normals
numpy would hand out next, bit for bit and in numpy's order, whole batches of frames at a time;
``commit()`` puts numpy's global stream where the draws left it.

    np.random.seed(7)
    ns = NumpyStream()
    x, y, frame_words = ns.frames(p, constellation, sigma, S, B)   # B frames, frame f in column f
    ns.commit()                                                    # np.random continues after them

Every draw synchronises the host with the current stream (the state after it is read back).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import dptr, ptr, stream_arg


def cdf_of(p):
    """np.random.choice's cdf of probabilities p, formed as numpy forms it."""
    cdf = np.asarray(p, np.float64).cumsum()
    cdf /= cdf[-1]
    return cdf


class NumpyStream:
    def __init__(self, state=None, device: int = 0):
        import torch

        _lib.require_gpu()
        name, key, pos, has_gauss, gauss = np.random.get_state() if state is None else state
        if name != "MT19937":
            raise ValueError(f"NumpyStream: the state of a {name} generator, expected MT19937")
        key = np.ascontiguousarray(key, np.uint32)
        if key.shape != (624,):
            raise ValueError("NumpyStream: key must hold 624 words")
        self.device = torch.device("cuda", device)
        self._h = C.c_void_p()
        _lib.check(_lib.load().qr_npstream_create(ptr(key), int(pos), int(has_gauss), float(gauss), device,
                                                  C.byref(self._h)), "npstream_create")
        self._ws = None   # the last frames call's workspace: seek_frame reads its words

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.load().qr_npstream_destroy(h)

    def _stream(self):
        return stream_arg(None, self.device)[1]

    def _draw(self, fn, n, dtype, *args):
        import torch

        n = int(n)
        if n < 0:
            raise ValueError("negative count")
        out = torch.empty(n, dtype=dtype, device=self.device)
        self._ws = None
        _lib.check(fn(self._h, n, *args, dptr(out) if n else None, self._stream()), "npstream")
        return out

    # ------------------------------------------------------------------ draws
    def words(self, n):
        """The next n words, uint32 [n]: np.frombuffer(np.random.bytes(4 * n), '<u4')."""
        import torch

        return self._draw(_lib.load().qr_npstream_words_device, n, torch.uint32)

    def random_sample(self, n):
        """np.random.random_sample(n), float64 [n]."""
        import torch

        return self._draw(_lib.load().qr_npstream_random_sample_device, n, torch.float64)

    def standard_normal(self, n):
        """np.random.randn(n), float64 [n]."""
        import torch

        return self._draw(_lib.load().qr_npstream_standard_normal_device, n, torch.float64)

    def choice(self, p, n):
        """np.random.choice(len(p), size=n, p=p), int64 [n]."""
        import torch

        cdf = cdf_of(p)
        if not 2 <= cdf.size <= 256:
            raise ValueError("choice: 2..256 probabilities")
        d_cdf = torch.tensor(cdf, dtype=torch.float64, device=self.device)
        return self._draw(_lib.load().qr_npstream_choice_device, n, torch.int64, int(cdf.size), dptr(d_cdf))

    def frames(self, p, constellation, sigma, S, B, ld=None):
        """B frames in sequence, each x = np.random.choice(M, size=S, p=p) and then
        y = constellation[x] + sigma * np.random.randn(S): (x int64 [S, ld], y float64 [S, ld],
        frame_words int64 [B]), frame f in column f, columns B..ld-1 zero, frame_words[f] the words
        consumed through frame f.  ld defaults to B rounded up to a multiple of 64."""
        import torch

        S, B = int(S), int(B)
        ld = (B + 63) // 64 * 64 if ld is None else int(ld)
        cdf = cdf_of(p)
        a = np.ascontiguousarray(constellation, np.float64)
        if a.shape != cdf.shape:
            raise ValueError("frames: p and constellation differ in length")
        if S <= 0:
            raise ValueError("frames: S must be positive")
        _lib.check_batch(B, ld, "frames")
        size = C.c_size_t(0)
        _lib.check(_lib.load().qr_npstream_frames_workspace_size(S, B, C.byref(size)), "npstream_frames_workspace_size")
        dev = self.device
        if self._ws is None or self._ws.numel() < size.value:
            self._ws = None
            self._ws = torch.empty(size.value, dtype=torch.uint8, device=dev)
        ws = self._ws
        d_cdf = torch.tensor(cdf, dtype=torch.float64, device=dev)
        d_a = torch.tensor(a, dtype=torch.float64, device=dev)
        x = torch.empty((S, ld), dtype=torch.int64, device=dev)
        y = torch.empty((S, ld), dtype=torch.float64, device=dev)
        fw = torch.empty(B, dtype=torch.int64, device=dev)
        _lib.check(_lib.load().qr_npstream_frames_device(self._h, B, ld, S, int(cdf.size), dptr(d_cdf), dptr(d_a),
                                                         float(sigma), dptr(x), dptr(y), dptr(fw), dptr(ws),
                                                         ws.numel(), self._stream()), "npstream_frames")
        return x, y, fw

    # ------------------------------------------------------------------ state
    def seek_frame(self, w):
        """The state becomes the one after frame w of the last ``frames`` call."""
        _lib.check(_lib.load().qr_npstream_seek_frame(self._h, int(w)), "npstream_seek_frame")

    def get_state(self):
        """The state as np.random.get_state() returns it (np.random.set_state accepts it)."""
        key = np.empty(624, np.uint32)
        pos, hg, g = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        _lib.check(_lib.load().qr_npstream_state(self._h, ptr(key), C.byref(pos), C.byref(hg), C.byref(g)),
                   "npstream_state")
        return ("MT19937", key, int(pos.value), int(hg.value), float(g.value))

    def commit(self):
        """numpy's global stream continues where this stream stands."""
        np.random.set_state(self.get_state())
