"""Rate adaptation of one mother code: puncturing, shortening and blind rounds.

Not a reference interface: the reference has no rate adaptation; the definition below is this
library's (DESIGN.md "Rate adaptation"; Elkouss, Martinez-Mateo, Martin 2010 and Martinez-Mateo,
Elkouss, Martin 2012).

Of the mother code's V variables, p are *punctured* (random bits nobody discloses: Alice's LAPPR
is 0), s are *shortened* (random bits Bob discloses: Alice's LAPPR is +-SHORTENED_LAPPR) and the
other n = V - p - s carry the payload, n / bps symbols.  With K = V - C the code rate is
(K - s) / n and the syndrome leaks (C - p + s) / n bits per payload bit.  In a blind round Bob
discloses some of the punctured bits of a frame that failed, and Alice decodes again.

The host side (this module's numpy part) is importable without a GPU; ``expand_host`` is the
normative definition of what the kernel of csrc/rate_adapt.hip computes.
"""
from __future__ import annotations

import numpy as np

# A shortened LAPPR must be finite: box_plus(inf, inf) is NaN in the reference's arithmetic
# (|a - b| is NaN), and a decode with +-inf at the shortened positions returns NaN for every
# LAPPR of every frame.  1e300 is the value the reference itself uses for a certain bit
# (noisemapper.pyx:218), and box_plus(1e300, 1e300) is 1e300.
SHORTENED_LAPPR = 1e300


def untainted_order(vid, cid, seed: int):
    """(order int64[V], u): the variables in the order they are punctured.  Walk
    ``np.random.default_rng(seed).permutation(V)``; a variable is picked if its checks are pairwise
    distinct and none of them is a neighbour of an earlier pick, and its checks are then marked.
    `order` is the picks in pick order followed by the rest in walk order, u the number of picks:
    among the first u no check sees two of them, so each is recovered in one iteration."""
    vid = np.asarray(vid, np.int64)
    cid = np.asarray(cid, np.int64)
    if vid.shape != cid.shape or vid.ndim != 1 or vid.size == 0:
        raise ValueError("vid and cid must be 1-D arrays of one size")
    V, C = int(vid.max()) + 1, int(cid.max()) + 1
    by_var = np.argsort(vid, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(vid, minlength=V))])
    chk = cid[by_var]
    marked = np.zeros(C, bool)
    picks, rest = [], []
    for v in np.random.default_rng(seed).permutation(V):
        c = chk[ptr[v]:ptr[v + 1]]
        if np.unique(c).size == c.size and not marked[c].any():
            marked[c] = True
            picks.append(v)
        else:
            rest.append(v)
    return np.array(picks + rest, np.int64), len(picks)


class RateAdaption:
    """Which variables of a V-variable code are punctured and which are shortened.

    Filler order: filler j < s is shortened[j], filler s + i is punctured[i] (so `revealed` = r
    discloses punctured[0..r-1]).  payload_rows: the other variables in increasing order; payload row
    k is bit k % bps of symbol k // bps, as the demappers write them.  slot int32[V]: payload row k
    maps to k, filler j to -1 - j."""

    def __init__(self, V: int, punctured, shortened):
        V = int(V)
        pun = np.array(punctured, np.int64).reshape(-1)
        sho = np.array(shortened, np.int64).reshape(-1)
        both = np.concatenate([sho, pun])
        if V < 1:
            raise ValueError("V must be positive")
        if both.size and (both.min() < 0 or both.max() >= V):
            raise ValueError(f"punctured / shortened indices must be in [0, {V})")
        if np.unique(both).size != both.size:
            raise ValueError("punctured and shortened indices must be disjoint and without repeats")
        if both.size > V - 1:
            raise ValueError(f"p + s = {both.size} leaves no payload (V = {V})")
        self.V, self.p, self.s = V, int(pun.size), int(sho.size)
        self.n = V - self.p - self.s
        self.punctured, self.shortened, self.fillers = pun, sho, both
        is_pay = np.ones(V, bool)
        is_pay[both] = False
        self.payload_rows = np.flatnonzero(is_pay).astype(np.int64)
        slot = np.empty(V, np.int32)
        slot[self.payload_rows] = np.arange(self.n, dtype=np.int32)
        slot[both] = -1 - np.arange(both.size, dtype=np.int32)
        self.slot = slot
        self._dev = {}   # device index -> (slot int32[V], payload_rows int32[n]) on it

    @classmethod
    def from_order(cls, order, p: int, s: int):
        """Puncture the first p of `order`, last first (the last-picked punctured variable is disclosed
        first), and shorten the last s."""
        order = np.asarray(order, np.int64).reshape(-1)
        V, p, s = order.size, int(p), int(s)
        if p < 0 or s < 0 or p + s > V:
            raise ValueError(f"need p >= 0, s >= 0, p + s <= V (p={p} s={s} V={V})")
        return cls(V, order[:p][::-1], order[V - s:])

    def check_bps(self, bps: int) -> int:
        """The payload is whole symbols of `bps` bits, at least one: the payload's symbol count."""
        bps = int(bps)
        if self.p + self.s > self.V - bps:
            raise ValueError(f"p + s = {self.p + self.s} > V - bit_per_symbol = {self.V - bps}")
        if self.n % bps:
            raise ValueError(f"the payload of {self.n} bits is not a multiple of bit_per_symbol={bps}")
        return self.n // bps

    def rate(self, K: int, revealed: float = 0.0) -> float:
        """(K - s - revealed) / (V - p - s) with the mother code's K = V - C."""
        return (K - self.s - revealed) / (self.V - self.p - self.s)

    # ---------------------------------------------------------------- device
    def _device_tables(self, device):
        import torch

        key = torch.device(device).index
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.slot).to(device),
                              torch.from_numpy(self.payload_rows.astype(np.int32)).to(device))
        return self._dev[key]

    def expand_device(self, lappr_pay_fi, word_pay_fi, fill_fi, B: int, revealed=None, out=None, L=SHORTENED_LAPPR,
                      stream=None):
        """expand_host in the frame-innermost layout (qr_rate_adapt_expand_device): lappr_pay_fi float64
        [n, ld], word_pay_fi uint8 [n, ld], fill_fi uint8 [p + s, ld], revealed int32 [ld] or None ->
        (lappr float64 [V, ld], word uint8 [V, ld]), columns [0, B) written.  out: the two outputs to
        write into.  One launch, asynchronous on `stream` (default: torch's current stream)."""
        import torch

        from . import _lib
        from ._lib import check_batch, check_tensor, dptr, stream_arg

        what = "expand_device"
        _, ld = _lib.check_2d(lappr_pay_fi, what, "lappr_pay_fi", "[n, ld]")
        check_batch(B, ld, what)
        dev = lappr_pay_fi.device
        check_tensor(lappr_pay_fi, "lappr_pay_fi", (self.n, ld), torch.float64)
        check_tensor(word_pay_fi, "word_pay_fi", (self.n, ld), torch.uint8, dev.index)
        check_tensor(fill_fi, "fill_fi", (self.p + self.s, ld), torch.uint8, dev.index)
        if revealed is not None:
            check_tensor(revealed, "revealed", (ld,), torch.int32, dev.index)
        if out is None:
            out = (torch.empty((self.V, ld), dtype=torch.float64, device=dev),
                   torch.empty((self.V, ld), dtype=torch.uint8, device=dev))
        lappr, word = out
        check_tensor(lappr, "out[0]", (self.V, ld), torch.float64, dev.index)
        check_tensor(word, "out[1]", (self.V, ld), torch.uint8, dev.index)
        slot, _ = self._device_tables(dev)
        fill_ptr = dptr(fill_fi if self.p + self.s else word_pay_fi)   # no filler: any address, never read
        _lib.check(_lib.load().qr_rate_adapt_expand_device(
            self.V, self.n, self.p, self.s, dptr(slot), int(B), ld, dptr(lappr_pay_fi), dptr(word_pay_fi), fill_ptr,
            dptr(revealed), float(L), dptr(lappr), dptr(word), stream_arg(stream, dev)[1]), what)
        return lappr, word

    def count_errors_device(self, B: int, ld: int, final, word, success, iters, ferr, counters, stream=None):
        """pipeline.count_errors_device over payload_rows in place of the first K rows
        (qr_count_errors_rows_device): per-frame bit errors into ferr int32 [B], the five counters added
        to counters int64 [5]."""
        from . import _lib
        from ._lib import dptr, stream_arg

        _, rows = self._device_tables(final.device)
        _lib.check(_lib.load().qr_count_errors_rows_device(
            int(B), int(ld), self.n, dptr(rows), dptr(final), dptr(word), dptr(success), dptr(iters), dptr(ferr),
            dptr(counters), stream_arg(stream, final.device)[1]), "count_rows")
        return counters


def expand_host(adapt: RateAdaption, lappr_pay, word_pay, fill, revealed=None, L: float = SHORTENED_LAPPR):
    """The normative definition: lappr_pay float64 [B, n], word_pay uint8 [B, n], fill uint8
    [B, p + s], revealed int [B] or None -> (lappr float64 [B, V], word uint8 [B, V]).
    A payload variable takes the LAPPR and the bit of its payload row, bit for bit.  Filler j takes
    the bit fill[j] != 0; it is known iff j < s + max(revealed[b], 0); a known filler takes +L for
    bit 0 and -L for bit 1, an unknown one +0.0."""
    lappr_pay = np.asarray(lappr_pay, np.float64)
    word_pay = np.asarray(word_pay, np.uint8)
    fill = np.asarray(fill, np.uint8)
    B = lappr_pay.shape[0]
    nf = adapt.p + adapt.s
    if lappr_pay.shape != (B, adapt.n) or word_pay.shape != (B, adapt.n) or fill.shape != (B, nf):
        raise ValueError("expand_host: need lappr_pay [B, n], word_pay [B, n], fill [B, p + s]")
    if not (np.isfinite(L) and L > 0):
        raise ValueError("expand_host: L must be finite and positive")
    r = np.zeros(B, np.int64) if revealed is None else np.maximum(np.asarray(revealed, np.int64).reshape(B), 0)
    lappr = np.empty((B, adapt.V), np.float64)
    word = np.empty((B, adapt.V), np.uint8)
    lappr[:, adapt.payload_rows] = lappr_pay
    word[:, adapt.payload_rows] = word_pay
    bit = (fill != 0).astype(np.uint8)
    known = np.arange(nf, dtype=np.int64)[None, :] < adapt.s + r[:, None]
    word[:, adapt.fillers] = bit
    lappr[:, adapt.fillers] = np.where(known, np.where(bit == 0, L, -L), 0.0)
    return lappr, word


def blind_batch(sim, nm, B: int, gen, two_var: float, rounds: int, step: int, hook=None):
    """Blind reconciliation of one batch of sim = Simulator(..., adapt=...): round 0 decodes all B
    frames with revealed = 0; in each of up to `rounds` further rounds the frames that failed and
    still have revealed < p get revealed = min(revealed + step, p), the batch is expanded again,
    those frames' columns are gathered into a batch of leading_dim(count) columns, decoded from
    scratch and scattered back.  Stops early when no such frame is left.  hook(lappr_pay, word_pay,
    fill, B) sees the payload.  Returns a dict of per-frame tensors: final [V, ld] (columns [0, B)),
    success, iterations (of the last attempt), iterations_total, revealed, attempts (all [B]),
    success_round0, and word [V, ld]."""
    import torch

    from .pipeline import decode_entry, leading_dim, syndrome_device

    adapt = sim.adapt
    if adapt is None:
        raise ValueError("blind_batch needs a Simulator with an adaptation")
    if rounds < 0 or step < 1:
        raise ValueError("need rounds >= 0 and step >= 1")
    lappr_pay, word_pay, fill, ld = sim.payload(nm, B, gen, two_var)
    if hook is not None:
        hook(lappr_pay, word_pay, fill, B)
    decode = decode_entry(sim.dec, sim.schedule)
    revealed = torch.zeros(ld, dtype=torch.int32, device=sim.device)
    lappr, word = adapt.expand_device(lappr_pay, word_pay, fill, B, revealed)
    synd = syndrome_device(sim.dec, word, B, ld)     # the word does not change with what is disclosed
    final, success, iterations = decode(lappr, synd, B, sim.max_iterations)
    success, iterations = success[:B], iterations[:B]
    success0 = success.clone()
    total = iterations.to(torch.int64)
    attempts = torch.ones(B, dtype=torch.int32, device=sim.device)
    for _ in range(rounds):
        idx = torch.nonzero((success == 0) & (revealed[:B] < adapt.p)).reshape(-1)
        count = int(idx.numel())
        if count == 0:
            break
        revealed[idx] = torch.clamp(revealed[idx] + step, max=adapt.p)
        adapt.expand_device(lappr_pay, word_pay, fill, B, revealed, out=(lappr, word))
        ld2 = leading_dim(count)
        l2 = torch.zeros((adapt.V, ld2), dtype=torch.float64, device=sim.device)
        s2 = torch.zeros((sim.C, ld2), dtype=torch.uint8, device=sim.device)
        l2[:, :count] = lappr[:, idx]
        s2[:, :count] = synd[:, idx]
        f2, ok2, it2 = decode(l2, s2, count, sim.max_iterations)
        final[:, idx] = f2[:, :count]
        success[idx] = ok2[:count]
        iterations[idx] = it2[:count]
        total[idx] += it2[:count].to(torch.int64)
        attempts[idx] += 1
    return {"final": final, "success": success, "iterations": iterations, "iterations_total": total,
            "revealed": revealed[:B], "attempts": attempts, "success_round0": success0, "word": word}
