"""Batched, GPU-resident evaluation of an LDPC code on a binary channel.

GPU counterpart of the frame loops of sims/sim_decode.py and sims/sim_direct.py (binary-input
AWGN, soft :90-117 or hard-decided :64-88; the two scripts differ only in the name of their CSV's
first column) and of sims/sim_bsc.py:54-76 (binary symmetric channel).  Per frame the reference
draws a uniform word, takes its syndrome, forms the channel LLRs, decodes, and counts the bits
whose final LAPPR is < 0 against the word.  Here a batch of B frames is drawn by torch, turned into
LLRs by one libqamr kernel (csrc/binary_channel.hip), decoded and counted in HBM, sharded over the
ranks and cut at the reference's stopping frame exactly as qamr.sim does (run_frames with the
script's own stopping rule).  RNG streams are torch's (per seed, rank and batch); numpy's legacy
stream on the GPU is the switch of qamr.sim alone (``stream="numpy"``: these scripts draw from
np.random.default_rng, another generator).
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from ._lib import dptr, stream_arg
from .decoder import Decoder
from .pipeline import check_schedule, count_errors_device, decode_entry, leading_dim, syndrome_device
from .sim import StopRule, run_seeded

CHANNELS = ("biawgn", "biawgn_hard", "bsc")


def check_channel(channel: str) -> str:
    """"biawgn" = sim_decode.py without --hard, "biawgn_hard" = with it, "bsc" = sim_bsc.py."""
    if channel not in CHANNELS:
        raise ValueError(f"channel must be one of {CHANNELS}, got {channel!r}")
    return channel


def biawgn_stop_rule(simulation_loops: int, min_errors: int) -> StopRule:
    """sim_decode.py:86: err_count >= minerr and wordcount > simloops / 20 (0-based wordcount)."""
    return StopRule(0, int(min_errors), math.floor(simulation_loops / 20) + 1)


def bsc_stop_rule(simulation_loops: int, min_errors: int, index_bound: int | None = None) -> StopRule:
    """sim_bsc.py:75: error_count > minerr and it > max(20, niters // 100) with the 1-based frame
    number it, i.e. the 0-based index >= that bound (index_bound replaces it when given)."""
    bound = max(20, simulation_loops // 100) if index_bound is None else int(index_bound)
    return StopRule(0, int(min_errors) + 1, bound)


def biawgn_coefficients(snr_dB: float, alpha: float = 1.0, hard: bool = False):
    """(coef, vsqrt) of sim_decode.py:43-44 with :98 (soft: 2 alpha / v) or :61-62 (hard: LLR0,
    inf once err_prob underflows to 0), as host doubles."""
    v = (10 ** (-snr_dB / 10)) / 2
    vsqrt = np.sqrt(v)
    if not hard:
        return float(2 * alpha / v), float(vsqrt)
    from scipy.special import erfc

    err_prob = 0.5 * erfc(1 / (np.sqrt(2) * vsqrt))
    with np.errstate(divide="ignore"):
        llr0 = np.log((1 - err_prob) / err_prob)
    return float(llr0), float(vsqrt)


def bsc_coefficient(rber: float) -> float:
    """sim_bsc.py:58: log2(1 - rber) - log2(rber)."""
    r = np.float64(rber)
    with np.errstate(divide="ignore"):
        return float(np.log2(1 - r) - np.log2(r))


class BinaryChannelSimulator:
    def __init__(self, decoder: Decoder, channel: str, max_iterations: int = 30, alpha: float = 1.0,
                 batch: int = 4096, device: int = 0, schedule: str = "flooding"):
        self.channel = check_channel(channel)
        self.schedule = check_schedule(schedule)   # "layered": Decoder.decode_layered_device
        import torch

        self.dec = decoder
        self.max_iterations = int(max_iterations)
        self.alpha = float(alpha)
        self.batch = int(batch)
        self.V, self.C = decoder.vnum, decoder.cnum
        # sim_decode.py:56-57, 80: the first N - cnum bits; sim_bsc.py:66: every bit
        self.K = self.V if channel == "bsc" else self.V - self.C
        self.device = torch.device("cuda", device)

    def _stream(self):
        return stream_arg(None, self.device)[1]

    def frames(self, point: float, B: int, gen):
        """One batch of inputs at `point` (dB, or the raw BER of the BSC):
        (llr [V, ld], synd [C, ld], word [V, ld], ld)."""
        import torch

        L = _lib.load()
        ld = leading_dim(B)
        word = torch.randint(0, 2, (self.V, ld), generator=gen, device=self.device, dtype=torch.uint8)
        synd = syndrome_device(self.dec, word, B, ld)
        llr = torch.empty((self.V, ld), dtype=torch.float64, device=self.device)
        if self.channel == "bsc":
            u = torch.rand((self.V, ld), generator=gen, device=self.device, dtype=torch.float64)
            _lib.check(L.qr_bsc_llr_device(bsc_coefficient(point), float(point), B, ld, self.V, dptr(word), dptr(u),
                                           dptr(llr), None, self._stream()), "bsc_llr")
        else:
            hard = self.channel == "biawgn_hard"
            coef, vsqrt = biawgn_coefficients(point, self.alpha, hard)
            z = torch.randn((self.V, ld), generator=gen, device=self.device, dtype=torch.float64)
            _lib.check(L.qr_biawgn_llr_device(int(hard), coef, vsqrt, B, ld, self.V, dptr(word), dptr(z), dptr(llr),
                                              self._stream()), "biawgn_llr")
        return llr, synd, word, ld

    def batch_results(self, point: float, B: int, gen, hook=None):
        """Generate, decode and count one shard of B frames: (ferr int32[B], succ uint8[B],
        its int32[B], delta int64[5]) on the GPU.  hook(llr, synd, word, B) sees the inputs."""
        import torch

        llr, synd, word, ld = self.frames(point, B, gen)
        if hook is not None:
            hook(llr, synd, word, B)
        fin, succ, its = decode_entry(self.dec, self.schedule)(llr, synd, B, self.max_iterations)
        ferr = torch.empty(B, dtype=torch.int32, device=self.device)
        delta = torch.zeros(5, dtype=torch.int64, device=self.device)
        count_errors_device(True, B, ld, self.K, fin, word, succ, its, ferr, delta)
        return ferr, succ[:B], its[:B], delta

    def stop_rule(self, simulation_loops: int, min_errors: int) -> StopRule:
        if self.channel == "bsc":
            return bsc_stop_rule(simulation_loops, min_errors)
        return biawgn_stop_rule(simulation_loops, min_errors)

    def run_point(self, point: float, simulation_loops: int, min_errors: int, seed: int = 0, hook=None):
        """Frames until `simulation_loops` or the script's early stop; returns the script's tuple
        (point, ber, fer, avg_iterations_of_successes).  hook(batch_index, llr, synd, word, B):
        optional view of every shard's inputs (tests)."""
        be, fe, su, it, fr = run_seeded(lambda B, gen, h: self.batch_results(point, B, gen, h), seed, hook, self.batch,
                                        simulation_loops, min_errors, self.device,
                                        self.stop_rule(simulation_loops, min_errors))
        return (point, be / (fr * self.K), fe / fr, 0 if su == 0 else it / su)
