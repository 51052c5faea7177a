"""Drop-in ``Matrix`` (matrix.pyx:20-60): the syndrome producer of the
softening pipeline.  ``eval_syndrome`` runs the frame-innermost XOR kernel of
libqamr (bit-exact integer work); ``eval_syndrome_device`` does it for a
batch resident in HBM."""
from __future__ import annotations

import numpy as np

from ._lib import as_buffer, check_2d, check_batch, check_tensor
from .decoder import Decoder
from .pipeline import syndrome_device


class Matrix:
    def __init__(self, vnode_array, cnode_array, device: int = 0):
        vid = as_buffer(vnode_array, np.int64, name="vnode_array")
        cid = as_buffer(cnode_array, np.int64, name="cnode_array")
        if vid.shape[0] != cid.shape[0]:
            raise ValueError("Incompatible sizes for input vectors")  # matrix.pyx:22-23
        self._code = Decoder(vid, cid, device=device)
        self.vnum = self._code.vnum
        self.cnum = self._code.cnum
        self.ednum = self._code.ednum

    @property
    def code(self) -> Decoder:
        return self._code

    def eval_syndrome(self, word):
        """matrix.pyx:55-60: synd[cid[e]] ^= word[vid[e]]."""
        w = as_buffer(word, np.uint8, name="word")
        if w.size != self.vnum:
            raise ValueError("Size of word does not match number of vnodes")
        # one frame: lane = check node (the node-level surface, qr_check_word_host): against
        # an all-zero syndrome each check reports (XOR of its word bytes) ^ 1
        ok, _ = self._code._check_nodes(w, np.zeros(self.cnum, np.uint8), False)
        return ok ^ np.uint8(1)

    def eval_syndrome_device(self, word_fi, B: int, stream=None):
        """word_fi uint8 [V, ld] -> synd uint8 [C, ld]."""
        import torch

        _, ld = check_2d(word_fi, "eval_syndrome_device", "word_fi", "[V, ld]")
        check_batch(B, ld, "eval_syndrome_device")
        check_tensor(word_fi, "word_fi", (self.vnum, ld), torch.uint8, self._code.device)
        return syndrome_device(self._code, word_fi, int(B), int(ld), stream)
