"""Shared by tests/test_binary_cpu.py and tests/test_gpu_binary.py: tests/golden/binary_channel.npz
unpacked, the scripts' frame loops written out frame by frame, and numpy's form of the three LLRs."""
import functools

import numpy as np

from conftest import golden

N, K, CHECKS, FRAMES, MAXITER = 1008, 504, 504, 16, 30


class Case:
    def __init__(self, g, c):
        k = f"c{c}_"
        self.index = c
        self.channel = str(g[k + "channel"])
        self.point = float(g[k + "point"])
        self.alpha = float(g[k + "alpha"])
        self.coef = float(g[k + "coef"])
        self.vsqrt = float(g[k + "vsqrt"]) if k + "vsqrt" in g.files else None
        self.word = np.unpackbits(g[k + "word"], axis=1)[:, :N]
        self.noise = g[k + ("u" if self.channel == "bsc" else "z")].astype(np.float64)   # stored as float32
        self.llr, self.final = g[k + "llr"], g[k + "final"]
        self.synd = np.unpackbits(g[k + "synd"], axis=1)[:, :CHECKS]
        self.success, self.iters = g[k + "success"], g[k + "iters"]
        self.err_k, self.err_n = g[k + "err_k"], g[k + "err_n"]
        self.loop_args, self.loop_counts, self.loop_tuple = g[k + "loop_args"], g[k + "loop_counts"], g[k + "loop_tuple"]
        self.count_bits = N if self.channel == "bsc" else K
        self.errors = self.err_n if self.channel == "bsc" else self.err_k

    def numpy_llr(self):
        """The three formulas in numpy, operation by operation, for all 16 frames."""
        w = self.word.astype(np.float64)
        if self.channel == "bsc":
            rx = self.word ^ (self.noise < self.point).astype(np.uint8)
            return self.coef * (1 - 2 * rx.astype(np.float64))
        y = (1 - 2 * w) + self.vsqrt * self.noise
        return self.coef * (np.sign(y) if self.channel == "biawgn_hard" else y)


@functools.lru_cache(maxsize=None)
def fixture():
    return golden("binary_channel.npz")


@functools.lru_cache(maxsize=None)
def cases():
    g = fixture()
    return tuple(Case(g, c) for c in range(int(g["n_cases"])))


def sequential(rule, per_frame, loops):
    """A plain sequential loop under a qamr.sim.StopRule: per_frame[w] = (bit errors, success,
    iterations); returns the five counters after the stopping frame."""
    total = [0, 0, 0, 0, 0]
    for w in range(loops):
        e, s, i = per_frame[w]
        total[0] += e
        total[1] += 1 if e else 0
        total[2] += 1 if s else 0
        total[3] += i if s else 0
        total[4] = w + 1
        if total[rule.counter] >= rule.need and w >= rule.first_index:
            break
    return total


def result_tuple(point, counters, bits):
    be, fe, su, it, fr = counters
    return (point, be / (fr * bits), fe / fr, 0 if su == 0 else it / su)


def biawgn_script_loop(per_frame, simloops, minerr):
    """sims/sim_decode.py's loop as the issue states it: stop after 0-based frame wc when
    err_count >= minerr and wc > simloops / 20."""
    total = [0, 0, 0, 0, 0]
    for wc in range(simloops):
        e, s, i = per_frame[wc]
        total = [total[0] + e, total[1] + (e > 0), total[2] + (s > 0), total[3] + (i if s else 0), wc + 1]
        if total[0] >= minerr and wc > simloops / 20:
            break
    return total


def bsc_script_loop(per_frame, niters, minerr, bound=None):
    """sims/sim_bsc.py's loop: stop after 1-based frame it when error_count > minerr and
    it > max(20, niters // 100) (or > bound)."""
    m = max(20, niters // 100) if bound is None else bound
    total = [0, 0, 0, 0, 0]
    for it in range(1, niters + 1):
        e, s, i = per_frame[it - 1]
        total = [total[0] + e, total[1] + (e > 0), total[2] + (s > 0), total[3] + (i if s else 0), it]
        if total[0] > minerr and it > m:
            break
    return total
