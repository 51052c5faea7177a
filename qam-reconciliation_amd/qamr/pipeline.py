"""Batched, GPU-resident softening reconciliation (Monte-Carlo frame pipeline).

The reference runs one frame at a time on the CPU (sims/reconciliation.pyx:93-168,
``simulate_softening_snr_dB``).  Here a whole batch of B independent frames
lives in HBM in the frame-innermost layout ([node][ld], ld % 64 == 0) and each
stage is one HIP kernel of libqamr:

  Alice  x  ~ p (torch RNG)               reconciliation.pyx:129
  channel y = a[x] + sigma * n            :132
  Bob    x_hat, n_hat, word   (k_bob)     :135-138  noisemapper.pyx:349-388
  Bob    synd = H word        (k_syndrome) :139     matrix.pyx:55-60
  Alice  lappr = alpha * demap(n_hat, x)  :143-145  (k_demap, decoder layout; or, with
         demapper="simplified", formulation 1: k_demap_interp_wave)
  Alice  decode (k_check / k_status / k_var) :147  (or, with schedule="layered", the layered
         schedule of this library: k_layer_check per layer, no counterpart in the reference)
  count  BER/FER/iterations   (k_count_*)  :149-157

The RNG stream of this pipeline is torch's: its parity is established on the fixtures
and the oracle.  The reference's own frames, drawn from numpy's legacy
stream on the GPU, are the switch of the simulations: qamr.sim ``stream="numpy"`` (qamr.npstream).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import dptr, stream_arg
from .alphabet import PAMAlphabet
from .decoder import Decoder
from .noisemapper import NoiseMapper


def noise_variance(pa: PAMAlphabet, snr_db: float) -> float:
    """N0 = Es * 10^(-snr/10) / 2 (reconciliation.pyx:109-110)."""
    return pa.variance * (10 ** (-snr_db / 10)) / 2


def alternating_config(order: int) -> np.ndarray:
    """Default sign configuration of sim_reconciliation.py:84-86."""
    cfg = np.zeros(order, np.uint8)
    cfg[1::2] = 1
    return cfg


DEMAPPERS = ("search", "simplified")


def check_demapper(demapper: str) -> str:
    """The soft demapper of the softening scheme: "search" = demap_lappr_array (g_inv_search,
    noisemapper.pyx:450-559), "simplified" = demap_lappr_simplified_array (formulation 1 on the
    interpolated g_inv, noisemapper.pyx:563-620)."""
    if demapper not in DEMAPPERS:
        raise ValueError(f"demapper must be one of {DEMAPPERS}, got {demapper!r}")
    return demapper


SCHEDULES = ("flooding", "layered")


def check_schedule(schedule: str) -> str:
    """The decode schedule: "flooding" = the reference's (decoder.pyx:391-436, Decoder.decode_device),
    "layered" = the posteriors updated after every check (Decoder.decode_layered_device; this
    library's own definition, include/qamr.h: about half the iterations, other LAPPRs)."""
    if schedule not in SCHEDULES:
        raise ValueError(f"schedule must be one of {SCHEDULES}, got {schedule!r}")
    return schedule


def decode_entry(dec: Decoder, schedule: str):
    """The device decode of a schedule (both take decode_device's arguments)."""
    return dec.decode_layered_device if check_schedule(schedule) == "layered" else dec.decode_device


def leading_dim(B: int) -> int:
    return ((B + 255) // 256) * 256 if B >= 256 else ((B + 63) // 64) * 64


# ------------------------------------------------- stages shared with qamr.sim and qamr.sim_binary
def draw_symbols(p, S: int, ld: int, gen, uniform: bool):
    """Symbol indices int64 [S, ld] drawn from the probabilities `p` (a device tensor): one randint
    when they are uniform, else one multinomial."""
    import torch

    if uniform:
        return torch.randint(0, p.numel(), (S, ld), generator=gen, device=p.device, dtype=torch.int64)
    return torch.multinomial(p, S * ld, replacement=True, generator=gen).view(S, ld)


def syndrome_device(dec: Decoder, word_fi, B: int, ld: int, stream=None):
    """word_fi uint8 [V, ld] -> synd uint8 [C, ld] = H word of the first B columns (k_syndrome)."""
    import torch

    synd = torch.empty((dec.cnum, ld), dtype=torch.uint8, device=word_fi.device)
    _lib.check(_lib.load().qr_syndrome_device(dec.handle, B, ld, dptr(word_fi), dptr(synd),
                                              stream_arg(stream, word_fi.device)[1]), "syndrome")
    return synd


def count_errors_device(neg: bool, B: int, ld: int, K: int, final, word, success, iters, ferr, counters, stream=None):
    """Per-frame bit errors of the first K bits into ferr int32 [B] and {bit_errors, frame_errors,
    successes, iter_sum, frames} added to counters int64 [5]; neg: the `final < 0` rule of the
    binary-channel scripts in place of reconciliation.pyx:149-157."""
    L = _lib.load()
    entry = L.qr_count_errors_neg_device if neg else L.qr_count_errors_device
    _lib.check(entry(B, ld, K, dptr(final), dptr(word), dptr(success), dptr(iters), dptr(ferr), dptr(counters),
                     stream_arg(stream, final.device)[1]), "count_neg" if neg else "count")
    return counters


@dataclass
class Batch:
    B: int
    ld: int
    x: object      # int64 [S, ld]   transmitted symbol index
    nhat: object   # float64 [S, ld] Bob's transformed noise
    word: object   # uint8 [V, ld]   Bob's hard bits
    synd: object   # uint8 [C, ld]   syndrome of word


class SofteningPipeline:
    """One GPU's share of ``simulate_softening_snr_dB`` for a batch of frames."""

    def __init__(self, decoder: Decoder, bps: int, snr_db: float, batch: int, alpha: float = 1.0,
                 max_iterations: int = 50, sign_config=None, step: float = 2.0, device: int = 0,
                 demapper: str = "search", schedule: str = "flooding"):
        self.demapper = check_demapper(demapper)
        self.schedule = check_schedule(schedule)
        import torch

        self.dec = decoder
        self.pa = PAMAlphabet(bps, step)
        self.snr_db = float(snr_db)
        self.noise_var = noise_variance(self.pa, snr_db)
        cfg = alternating_config(self.pa.order) if sign_config is None else np.asarray(sign_config, np.uint8)
        self.nm = NoiseMapper(self.pa, self.noise_var, cfg, device=device)
        self.alpha = float(alpha)
        self.max_iterations = int(max_iterations)
        self.V, self.C = decoder.vnum, decoder.cnum
        if self.V % bps:
            raise ValueError(f"V={self.V} is not a multiple of bit_per_symbol={bps}")
        self.S = self.V // bps
        self.K = self.V - self.C  # info bits = first K variable nodes (reconciliation.pyx:120-121)
        self.B = int(batch)
        self.ld = leading_dim(self.B)
        self.device = torch.device("cuda", device)
        self._a = torch.tensor(self.pa.constellation, dtype=torch.float64, device=self.device)
        self._p = torch.tensor(self.pa.probabilities, dtype=torch.float64, device=self.device)
        self._uniform = bool(np.all(self.pa.probabilities == self.pa.probabilities[0]))
        self.counters = torch.zeros(5, dtype=torch.int64, device=self.device)
        self._ferr = torch.empty(self.B, dtype=torch.int32, device=self.device)

    # -------------------------------------------------------------- inputs
    def generate(self, gen=None) -> Batch:
        import torch

        S, ld = self.S, self.ld
        x = draw_symbols(self._p, S, ld, gen, self._uniform)
        y = self._a[x] + self.nm.noise_sigma * torch.randn((S, ld), generator=gen, device=self.device,
                                                           dtype=torch.float64)
        _, nhat, word = self.nm.bob_map_device(y, self.B)
        return Batch(self.B, ld, x, nhat, word, self.dec_syndrome(word))

    def dec_syndrome(self, word_fi):
        return syndrome_device(self.dec, word_fi, self.B, self.ld)

    # ---------------------------------------------------------- hot path
    def demap(self, batch: Batch, out=None):
        if self.demapper == "simplified":
            return self.nm.demap_simplified_device(batch.nhat, batch.x, batch.B, self.alpha, out=out)
        return self.nm.demap_device(batch.nhat, batch.x, batch.B, self.alpha, out=out)

    def decode(self, lappr_fi, batch: Batch, final=None, success=None, iters=None):
        return decode_entry(self.dec, self.schedule)(lappr_fi, batch.synd, batch.B, self.max_iterations, final,
                                                     success, iters)

    def count(self, final_fi, batch: Batch, success, iters):
        """Accumulate {bit_errors, frame_errors, successes, iter_sum, frames}."""
        return count_errors_device(False, batch.B, batch.ld, self.K, final_fi, batch.word, success, iters, self._ferr,
                                   self.counters)

    def run_batch(self, gen=None):
        b = self.generate(gen)
        l = self.demap(b)
        fin, succ, its = self.decode(l, b)
        self.count(fin, b, succ, its)
        return b, l, fin, succ, its

    @staticmethod
    def summarize(counters, K: int, snr_db: float):
        """(snr, ber, fer, avg_iters_of_successes) as reconciliation.pyx:163-168."""
        be, fe, su, it, fr = [int(v) for v in counters]
        ber = be / (fr * K) if fr else 0.0
        fer = fe / fr if fr else 0.0
        return snr_db, ber, fer, (0 if su == 0 else it / su)
