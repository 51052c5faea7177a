"""Batched, GPU-resident Monte-Carlo reconciliation simulations.

GPU counterpart of sims/reconciliation.pyx:
  * ``simulate_softening_snr_dB``   (reconciliation.pyx:93-168)  -- the hot path
  * ``simulate_direct_snr_dB``      (reconciliation.pyx:173-249)
  * ``simulate_hard_reverse_snr_dB`` (reconciliation.pyx:253-329)
The reference decodes one frame at a time; here every batch of B independent
frames is generated, mapped, decoded and counted by libqamr kernels in HBM
(frame-innermost layout), and with several GPUs each rank takes a contiguous
share of every batch (frame sharding: global frame order = batch order, then
rank order, then the frame's column).  The five counters are all-reduced once
per batch (qamr.dist).  The ``ferr_count_min`` early stop is the reference's
per-frame rule (reconciliation.pyx:159-161): when it holds at the end of a
batch, the first global frame at which it held is located from the per-frame
error counts of every rank (``first_stop_frame``) and every counter is cut
there, so the returned tuple is the one the reference's sequential loop
returns for the same frames (tests/test_gpu_sim.py).  Returned tuples have the
reference's shape: (snr_dB, ber, fer, average iterations of successful frames).
RNG streams: ``stream="torch"`` (the default) draws every batch from torch's generator, seeded
per seed, rank and batch; ``stream="numpy"`` draws the frames from numpy's legacy global stream on
the GPU (qamr.npstream), frame after frame as the reference's loop does, so that after
``np.random.seed(s)`` the returned tuple is the reference's and ``np.random.get_state()`` is left
where the reference leaves it (one rank only: the frames of one stream are sequential).
Rate adaptation (``adapt=RateAdaption(...)``, qamr.rate_adapt; this library's, not the reference's):
only the n = V - p - s payload variables are drawn from the channel, n / bps symbols; the p punctured
and s shortened variables are filled with random bits drawn after them, and the bit errors are counted
over the payload rows (BER over n bits per frame).  torch's stream only.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import _lib, dist
from ._lib import dptr, stream_arg
from .alphabet import PAMAlphabet
from .decoder import Decoder
from .noisemapper import NoiseMapper
from .pipeline import (alternating_config, check_demapper, check_schedule, count_errors_device, decode_entry,
                       draw_symbols, leading_dim, syndrome_device)

MODES = ("softening", "direct", "hard")
STREAMS = ("torch", "numpy")


def check_stream(stream: str) -> str:
    """The `stream` keyword of the simulations; numpy's stream is sequential, so it has no ranks."""
    if stream not in STREAMS:
        raise ValueError(f"stream must be one of {STREAMS}")
    if stream == "numpy" and dist.env_world()[0] > 1:
        raise ValueError('stream="numpy" runs on one rank: the frames of one stream are sequential')
    return stream


def source_tables(pa: PAMAlphabet, device):
    """What llr_source reads of the alphabet, on the device: (constellation, probabilities, uniform?)."""
    import torch

    return (torch.tensor(pa.constellation, dtype=torch.float64, device=device),
            torch.tensor(pa.probabilities, dtype=torch.float64, device=device),
            bool(np.all(pa.probabilities == pa.probabilities[0])))


def llr_source(nm: NoiseMapper, pa: PAMAlphabet, S: int, B: int, gen, mode: str = "softening",
               demapper: str = "search", alpha: float = 1.0, two_variance: float | None = None,
               stream: str = "torch", tables=None):
    """One batch of B frames of S symbols for `mode`, with no code involved: (lappr [S * bps, ld],
    word [S * bps, ld]), the LAPPRs the decoder would be given and the word it must recover.
    gen: a torch generator, or the NumpyStream the frames are drawn from (stream="numpy").
    two_variance: the direct mode's 2 sigma^2 (reconciliation.pyx:191-192).  tables: source_tables(pa,
    device), for a caller that keeps them."""
    import torch

    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}")
    device = torch.device("cuda", nm._device)
    a, p, uniform = source_tables(pa, device) if tables is None else tables
    bps = pa.bit_per_symbol
    ld = leading_dim(B)
    sp = stream_arg(None, device)[1]
    if stream == "numpy":                              # reconciliation.pyx:129-132, frame after frame
        x, y, _ = gen.frames(pa.probabilities, pa.constellation, nm.noise_sigma, S, B, ld=ld)
    else:
        x = draw_symbols(p, S, ld, gen, uniform)
        y = a[x] + nm.noise_sigma * torch.randn((S, ld), generator=gen, device=device, dtype=torch.float64)
    lappr = torch.empty((S * bps, ld), dtype=torch.float64, device=device)
    if mode == "softening":                            # reconciliation.pyx:129-145
        _, nhat, word = nm.bob_map_device(y, B)
        if check_demapper(demapper) == "simplified":   # noisemapper.pyx:605-620 in place of :544-559
            nm.demap_simplified_device(nhat, x, B, alpha, out=lappr)
        else:
            nm.demap_device(nhat, x, B, alpha, out=lappr)
    elif mode == "direct":                             # reconciliation.pyx:209-221
        if two_variance is None:
            raise ValueError("the direct mode needs two_variance")
        word = torch.empty((S * bps, ld), dtype=torch.uint8, device=device)
        _lib.check(_lib.load().qr_symbols_to_bits_device(bps, B, ld, S, dptr(x), dptr(word), sp), "symbols_to_bits")
        _lib.check(_lib.load().qr_direct_lappr_device(nm.handle, float(two_variance), B, ld, S, dptr(y), dptr(lappr), sp),
                   "direct_lappr")
    else:                                              # reconciliation.pyx:290-303
        _, _, word = nm.bob_map_device(y, B)
        table = torch.tensor(np.ascontiguousarray(nm.bare_llr_table), dtype=torch.float64, device=device)
        _lib.check(_lib.load().qr_bare_llr_device(bps, dptr(table), B, ld, S, dptr(x), dptr(lappr), sp), "bare_llr")
    return lappr, word


class Simulator:
    def __init__(self, decoder: Decoder, bps: int, mode: str = "softening", max_iterations: int = 50,
                 alpha: float = 1.0, batch: int = 4096, configuration_base: bool = False, step: float = 2.0,
                 device: int = 0, demapper: str = "search", stream: str = "torch", schedule: str = "flooding",
                 adapt=None):
        self.stream = check_stream(stream)
        if adapt is not None and self.stream == "numpy":
            raise ValueError('adapt needs stream="torch": the reference\'s stream has no draws for the filler bits')
        self.schedule = check_schedule(schedule)   # "layered": this library's schedule, not the reference's
        self.demapper = check_demapper(demapper)   # softening mode only; the other modes have no soft demap
        import torch

        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}")
        self.dec = decoder
        self.mode = mode
        self.pa = PAMAlphabet(bps, step)
        self.max_iterations = int(max_iterations)
        self.alpha = float(alpha)
        self.batch = int(batch)
        self.V, self.C = decoder.vnum, decoder.cnum
        if self.V % bps and adapt is None:   # with an adaptation the payload must be whole symbols, not V
            raise ValueError(f"V={self.V} is not a multiple of bit_per_symbol={bps}")
        self.S = self.V // bps
        self.K = self.V - self.C  # reconciliation.pyx:120-121
        self.adapt = adapt        # qamr.rate_adapt.RateAdaption: the payload is S' = n / bps symbols
        self.ber_bits = self.K    # the bits per frame the BER is over: the first K, or the payload's n
        if adapt is not None:
            if adapt.V != self.V:
                raise ValueError(f"the adaptation is for V={adapt.V}, the code has V={self.V}")
            self.S_pay = adapt.check_bps(bps)
            self.ber_bits = adapt.n
        self.cfg = np.zeros(self.pa.order, np.uint8) if configuration_base else alternating_config(self.pa.order)
        self.device = torch.device("cuda", device)
        self._dev_index = device
        self._tables = source_tables(self.pa, self.device)

    # ---------------------------------------------------------------- pieces
    def frames(self, nm: NoiseMapper, B: int, gen, two_variance: float):
        """One batch of inputs for the selected mode: (lappr [V, ld], synd [C, ld], word [V, ld], ld).
        gen: a torch generator, or the NumpyStream the frames are drawn from (stream="numpy")."""
        ld = leading_dim(B)
        if self.adapt is not None:
            lappr, word = self.adapt.expand_device(*self.payload(nm, B, gen, two_variance)[:3], B)
        else:
            lappr, word = llr_source(nm, self.pa, self.S, B, gen, self.mode, self.demapper, self.alpha, two_variance,
                                     self.stream, self._tables)
        synd = syndrome_device(self.dec, word, B, ld)
        return lappr, synd, word, ld

    def payload(self, nm: NoiseMapper, B: int, gen, two_variance: float):
        """With an adaptation, what a batch is expanded from: (lappr_pay [n, ld], word_pay [n, ld],
        fill uint8 [p + s, ld], ld).  The n / bps payload symbols go through the unchanged llr_source;
        the filler bits are drawn after them."""
        import torch

        ld = leading_dim(B)
        lappr_pay, word_pay = llr_source(nm, self.pa, self.S_pay, B, gen, self.mode, self.demapper, self.alpha,
                                         two_variance, self.stream, self._tables)
        fill = torch.randint(0, 2, (self.adapt.p + self.adapt.s, ld), dtype=torch.uint8, generator=gen,
                             device=self.device)
        return lappr_pay, word_pay, fill, ld

    # ------------------------------------------------------------------ run
    def batch_results(self, nm: NoiseMapper, B: int, gen, two_var: float, hook=None):
        """Generate, map, decode and count one shard of B frames: (ferr int32[B], succ uint8[B],
        its int32[B], delta int64[5]) on the GPU.  hook(lappr, synd, word, B) sees the inputs."""
        import torch

        lappr, synd, word, ld = self.frames(nm, B, gen, two_var)
        if hook is not None:
            hook(lappr, synd, word, B)
        fin, succ, its = decode_entry(self.dec, self.schedule)(lappr, synd, B, self.max_iterations)
        ferr = torch.empty(B, dtype=torch.int32, device=self.device)
        delta = torch.zeros(5, dtype=torch.int64, device=self.device)
        if self.adapt is not None:
            self.adapt.count_errors_device(B, ld, fin, word, succ, its, ferr, delta)
        else:
            count_errors_device(False, B, ld, self.K, fin, word, succ, its, ferr, delta)
        return ferr, succ[:B], its[:B], delta

    def run_snr(self, snr_dB: float, simulation_loops: int, ferr_count_min: int, seed: int = 0, hook=None):
        """Frames until `simulation_loops` or the early stop; returns
        (snr_dB, ber, fer, avg_iterations_of_successes).  hook(batch_index, lappr, synd, word, B):
        optional view of every shard's inputs (tests).  With stream="numpy" the frames come from
        numpy's global stream, which is left after the last frame counted; `seed` is not read (the
        caller seeds numpy, as for montecarlo_information).  With schedule="layered" the frames are
        the same (stream="numpy": still the reference's frames), but the decoder is this library's
        layered one, so the returned tuple is NOT the reference's."""
        Es = self.pa.variance
        two_var = Es * (10 ** (-snr_dB / 10))          # reconciliation.pyx:191-192, 272-273
        N0 = Es * (10 ** (-snr_dB / 10)) / 2           # reconciliation.pyx:109-110
        cfg = self.cfg if self.mode == "softening" else None
        nm = NoiseMapper(self.pa, N0, cfg, device=self._dev_index)

        batch_fn = lambda B, gen, h: self.batch_results(nm, B, gen, two_var, h)   # noqa: E731
        if self.stream == "numpy":
            be, fe, su, it, fr = run_numpy_stream(batch_fn, hook, self.batch, simulation_loops, ferr_count_min,
                                                  self.device)
        else:
            be, fe, su, it, fr = run_seeded(batch_fn, seed, hook, self.batch, simulation_loops, ferr_count_min,
                                            self.device)
        return (snr_dB, be / (fr * self.ber_bits), fe / fr, 0 if su == 0 else it / su)


def shard_counters(ferr, succ, its, n: int):
    """The five counters {bit_errors, frame_errors, successes, iteration_sum_of_successes,
    frames} of a shard's first n frames (reconciliation.pyx:149-157)."""
    import torch

    e = ferr[:n].to(torch.int64)
    s = succ[:n].to(torch.int64)
    return torch.stack([e.sum(), (e > 0).sum(), s.sum(), (its[:n].to(torch.int64) * s).sum(),
                        torch.tensor(n, dtype=torch.int64, device=ferr.device)])


@dataclass(frozen=True)
class StopRule:
    """A sequential frame loop's stopping rule, both parts monotone in the frame index: the loop
    stops after the first 0-based frame w at which the running sum of counter `counter` (0 = bit
    errors, 1 = frame errors) over frames 0..w is >= `need` and w >= `first_index`.  The rule of
    reconciliation.pyx:159-161 is StopRule(1, ferr_count_min, floor(simulation_loops / 20) + 1):
    what run_frames and first_stop_frame apply when no rule is given."""
    counter: int
    need: int
    first_index: int

    def holds(self, counters) -> bool:
        """After the last frame counted (counters[4] frames)."""
        return int(counters[self.counter]) >= self.need and int(counters[4]) - 1 >= self.first_index


def first_stop_frame(prev_frame_errors: int, ferr, start: int, done: int, ferr_count_min: int,
                     simulation_loops: int, rule: StopRule | None = None) -> int:
    """Global index of the first frame of this batch after which reconciliation.pyx:159-161
    holds: frame_error_count >= ferr_count_min and wordcount > simulation_loops / 20.  Both
    parts are monotone in the frame index, so it is max(first frame where the running frame-error
    count reaches the minimum, first index above loops / 20).  ferr: this rank's per-frame bit
    errors of its frames [done + start, done + start + len(ferr)); a collective over the ranks.
    With a `rule`, that rule instead: prev_frame_errors is then the rule's counter before this
    batch, and ferr_count_min and simulation_loops are not read."""
    import torch

    world, rank, _ = dist.env_world()
    dev = ferr.device
    if rule is None:
        rule = StopRule(1, ferr_count_min, math.floor(simulation_loops / 20) + 1)
    flags = (ferr > 0).to(torch.int64) if rule.counter == 1 else ferr.to(torch.int64)
    per_rank = torch.zeros(world, dtype=torch.int64, device=dev)
    per_rank[rank] = flags.sum()
    dist.all_reduce_sum(per_rank)                               # the counter's share of every rank's shard
    before = prev_frame_errors + int(per_rank[:rank].sum())     # shards are in rank order
    big = 1 << 62
    g_fe = big
    if flags.numel():
        hit = torch.nonzero(before + torch.cumsum(flags, 0) >= rule.need)
        if hit.numel():
            g_fe = done + start + int(hit[0, 0])
    t = torch.tensor([g_fe], dtype=torch.int64, device=dev)
    dist.all_reduce_min(t)
    return max(int(t.item()), rule.first_index)


def run_frames(frame_fn, batch: int, simulation_loops: int, ferr_count_min: int, device=None,
               rule: StopRule | None = None, on_stop=None):
    """The frame loop of reconciliation.pyx:127-168 over batches of batch * world frames,
    each rank taking its contiguous shard (dist.shard).  frame_fn(batch_index, start, B) ->
    (ferr, succ, its, delta) for this rank's B frames [done + start, done + start + B) of the
    batch (delta = their five counters).  Returns the five global counters at the reference's
    stopping frame: {bit_errors, frame_errors, successes, iteration_sum, frames = wordcount+1}.
    `rule`: another monotone stopping rule in place of :159-161 (ferr_count_min is then not read).
    on_stop(i): called when the loop stops early after frame i of this rank's shard of the batch."""
    import torch

    world, rank, _ = dist.env_world()
    total = torch.zeros(5, dtype=torch.int64, device=device)
    done, bidx = 0, 0
    while done < simulation_loops:
        n_global = min(batch * world, simulation_loops - done)
        start, B = dist.shard(n_global, world, rank)
        if B > 0:
            ferr, succ, its, delta = frame_fn(bidx, start, B)
        else:
            ferr = torch.zeros(0, dtype=torch.int32, device=device)
            succ = torch.zeros(0, dtype=torch.uint8, device=device)
            its = torch.zeros(0, dtype=torch.int32, device=device)
            delta = torch.zeros(5, dtype=torch.int64, device=device)
        dist.all_reduce_sum(delta)
        after = (total + delta).cpu().numpy()
        if dist.early_stop(after, ferr_count_min, simulation_loops) if rule is None else rule.holds(after):
            # the reference stopped at some frame of this batch: cut every counter there
            prev = int(total[1 if rule is None else rule.counter])
            g = first_stop_frame(prev, ferr, start, done, ferr_count_min, simulation_loops, rule)
            keep = min(max(g - (done + start) + 1, 0), B)
            if on_stop is not None and keep:
                on_stop(keep - 1)
            part = shard_counters(ferr, succ, its, keep) if keep else torch.zeros(5, dtype=torch.int64,
                                                                                 device=device)
            dist.all_reduce_sum(part)
            total += part.to(total.device)
            break
        total += delta
        done += n_global
        bidx += 1
    return [int(v) for v in total.cpu().numpy()]


def run_seeded(batch_fn, seed: int, hook, batch: int, simulation_loops: int, ferr_count_min: int, device,
               rule: StopRule | None = None):
    """run_frames over batch_fn(B, gen, hook(inputs..., B) or None) -> (ferr, succ, its, delta): every batch gets
    its own generator, seeded by (seed, rank, batch index), and `hook` is called with the batch index
    first."""
    _, rank, _ = dist.env_world()

    def frame_fn(bidx, start, B):
        import torch

        gen = torch.Generator(device=device).manual_seed(dist.rank_seed(seed, rank, bidx))
        h = None if hook is None else (lambda l, s, w, b: hook(bidx, l, s, w, b))
        return batch_fn(B, gen, h)

    return run_frames(frame_fn, batch, simulation_loops, ferr_count_min, device, rule)


def run_numpy_stream(batch_fn, hook, batch: int, simulation_loops: int, ferr_count_min: int, device,
                     rule: StopRule | None = None):
    """run_frames over batch_fn(B, stream, hook or None) with every batch drawn from one NumpyStream
    that starts at numpy's global state.  When the loop stops early at a frame, the stream seeks to
    that frame; in every case numpy's global state is committed at return, so np.random stands where
    the reference's sequential loop leaves it."""
    from .npstream import NumpyStream

    check_stream("numpy")
    ns = NumpyStream(device=device.index)

    def frame_fn(bidx, start, B):
        h = None if hook is None else (lambda l, s, w, b: hook(bidx, l, s, w, b))
        return batch_fn(B, ns, h)

    try:
        return run_frames(frame_fn, batch, simulation_loops, ferr_count_min, device, rule, on_stop=ns.seek_frame)
    finally:
        ns.commit()


def simulate_softening_snr_dB(snr_dB, dec, bps, nmconfig, decoder_iterations, simulation_loops, ferr_count_min,
                              alpha=1.0, batch=4096, seed=0, demapper="search", stream="torch",
                              schedule="flooding", adapt=None):
    """reconciliation.pyx:93-168 (the Matrix is the decoder's own graph).  demapper="simplified"
    swaps demap_lappr_array (:143) for demap_lappr_simplified_array.  stream="numpy": after
    np.random.seed(s), the tuple the reference returns after that seed (`seed` is not read).
    schedule="layered" decodes with the layered schedule (Decoder.decode_layered_device): with
    stream="numpy" the frames are still the reference's, but the returned tuple is not.
    adapt: a qamr.rate_adapt.RateAdaption (puncturing / shortening; stream="torch" only)."""
    sim = Simulator(dec, bps, "softening", decoder_iterations, alpha, batch, demapper=demapper, stream=stream,
                    schedule=schedule, adapt=adapt)
    sim.cfg = np.ascontiguousarray(nmconfig, np.uint8)
    return sim.run_snr(snr_dB, simulation_loops, ferr_count_min, seed)


def simulate_direct_snr_dB(snr_dB, dec, bps, decoder_iterations, simulation_loops, ferr_count_min, batch=4096, seed=0,
                           stream="torch", schedule="flooding", adapt=None):
    """reconciliation.pyx:173-249.  schedule="layered": the layered decode; with stream="numpy" the
    frames are still the reference's, but the returned tuple is not."""
    return Simulator(dec, bps, "direct", decoder_iterations, 1.0, batch, stream=stream, schedule=schedule,
                     adapt=adapt).run_snr(
        snr_dB, simulation_loops, ferr_count_min, seed)


def simulate_hard_reverse_snr_dB(snr_dB, dec, bps, decoder_iterations, simulation_loops, ferr_count_min, batch=4096,
                                 seed=0, stream="torch", schedule="flooding", adapt=None):
    """reconciliation.pyx:253-329.  schedule="layered": the layered decode; with stream="numpy" the
    frames are still the reference's, but the returned tuple is not."""
    return Simulator(dec, bps, "hard", decoder_iterations, 1.0, batch, stream=stream, schedule=schedule,
                     adapt=adapt).run_snr(
        snr_dB, simulation_loops, ferr_count_min, seed)
