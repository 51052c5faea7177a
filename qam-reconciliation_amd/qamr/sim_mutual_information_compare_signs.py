"""I(X,N;Xhat) vs SNR for every sign configuration of the noise mapper, the GPU counterpart of
sims/sim_mutual_information_compare_signs.py (its flags and defaults, its CSV columns).

    PYTHONPATH=qam-reconciliation_amd python -m qamr.sim_mutual_information_compare_signs \\
        [--out out.csv] [--snr 0 5] [--nsnr 11] [--bps 2] [--montecarlo] [--nmontecarlo 4096] \\
        [--nloops 64] [--seed 0] [--device 0]

The configuration list is the reference's (:33-62): every c in [0, 2^M) with reverse_flip_bits(c) >= c,
a[i] = bit i of c -- with M, the alphabet's order, as the bit count, as the reference has it (10
configurations at bps 2, 136 at bps 3).  Without --montecarlo (:87-93) p_Xhat comes from configuration
0's mapper and every (SNR point, configuration) integral goes into ONE batch: one NoiseMapper per SNR
point, the configurations passed as sign_configs (the configuration enters the integrand only through
g_inv's target).  With --montecarlo (:74-85) each (SNR point, configuration) is estimated on nloops
blocks of nmontecarlo samples, which = [0, 0, 1], drawn on the device with a seeded torch.Generator as
qamr.sim_montecarlo_information draws them.  One GPU.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(prog="mutual_information_base_scheme",
                                description="Evaluate mutual information vs SNR of the base scheme")
    p.add_argument("--out", default="out.csv")
    p.add_argument("--snr", type=float, nargs=2, default=[0, 5])
    p.add_argument("--nsnr", type=int, default=11)
    p.add_argument("--bps", type=int, default=2)
    p.add_argument("--montecarlo", action="store_true")
    p.add_argument("--nmontecarlo", type=int, default=1 << 12)
    p.add_argument("--nloops", type=int, default=1 << 6)
    p.add_argument("--seed", type=int, default=0, help="seed of the device generator the samples are drawn from")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def config_indices(bps):
    """sim_mutual_information_compare_signs.py:33-37, :53-54: the c with reverse_flip_bits(c) >= c."""
    M = 1 << bps
    if M > 16:
        raise ValueError(f"2^{M} candidate configurations at bps {bps}: not enumerable")

    def reverse_flip_bits(n):
        res = 0
        for k in range(M):
            res += (((n >> k) & 0b1) ^ 0b1) << (M - 1 - k)
        return res

    return [c for c in range(1 << M) if reverse_flip_bits(c) >= c]


def config_list(bps):
    """:40-59: one row per configuration, a[i] = bit i of c."""
    M = 1 << bps
    return np.array([[(c >> i) & 1 for i in range(M)] for c in config_indices(bps)], np.uint8)


def config_count(bps):
    """:60"""
    M = 1 << bps
    return (1 << ((M >> 1) - 1)) * ((1 << (M >> 1)) + 1)


def column_list(bps):
    return ["EsN0dB"] + [f"I(X,N;Xhat)_{c}" for c in config_indices(bps)]


def sweep_quad(bps, EsN0dB, device=0):
    """:87-93 for every SNR point, one batch."""
    from .alphabet import PAMAlphabet
    from .mutual_information import P_xhat, _warn, mutual_information_quad_batch
    from .noisemapper import NoiseMapper

    pa = PAMAlphabet(bps, 2)
    Es = pa.variance
    cfgs = config_list(bps)
    nc = len(cfgs)
    nms, pXs = [], []
    for e in EsN0dB:
        nm = NoiseMapper(pa, Es * (10 ** (-float(e) / 10)) / 2, cfgs[0], device=device)
        pX = P_xhat(nm)
        nms += [nm] * nc
        pXs += [pX] * nc
    I, abserr, _, ier = mutual_information_quad_batch("base", nms, pXs, np.tile(cfgs, (len(EsN0dB), 1)))
    for k in np.flatnonzero(ier):
        _warn(int(ier[k]), float(abserr[k]))
    return [(float(e), *map(float, I[s * nc:(s + 1) * nc])) for s, e in enumerate(EsN0dB)]


def sweep_montecarlo(bps, EsN0dB, nmontecarlo, nloops, seed=0, device=0):
    """:74-85 for every SNR point: the mean, in call order, of nloops estimates per configuration."""
    import torch

    from .alphabet import PAMAlphabet
    from .mutual_information import P_xhat, montecarlo_information_device
    from .noisemapper import NoiseMapper

    pa = PAMAlphabet(bps, 2)
    Es = pa.variance
    cfgs = config_list(bps)
    dev = torch.device("cuda", device)
    gen = torch.Generator(device=dev).manual_seed(seed)
    a = torch.from_numpy(np.ascontiguousarray(pa.constellation, np.float64)).to(dev)
    B, S = nloops, nmontecarlo
    ld = -(-B // 64) * 64
    which = np.array([0, 0, 1], dtype=np.uint8)
    rows = []
    for e in EsN0dB:
        N0 = Es * (10 ** (-float(e) / 10)) / 2
        res = [float(e)]
        for cfg in cfgs:
            nm = NoiseMapper(pa, N0, cfg, device=device)
            p_Xhat = P_xhat(nm)
            x = torch.randint(0, pa.order, (S, ld), generator=gen, device=dev, dtype=torch.int64)
            y = a[x] + nm.noise_sigma * torch.randn((S, ld), generator=gen, device=dev, dtype=torch.float64)
            info = montecarlo_information_device(nm, p_Xhat, x, y, B, which=which).cpu().numpy()
            acc = 0
            for f in range(B):
                acc += float(info[2, f])
            res.append(acc / nloops)
        rows.append(tuple(res))
    return rows


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.nsnr < 1 or args.nmontecarlo < 1 or args.nloops < 1:
        raise SystemExit("--nsnr, --nmontecarlo and --nloops must be positive")
    from ._lib import require_gpu
    from .sim_mutual_information_base_scheme import write_csv

    require_gpu()
    print(config_count(args.bps))   # :61-62
    print(config_list(args.bps))
    EsN0dB = np.linspace(args.snr[0], args.snr[1], args.nsnr)
    if args.montecarlo:
        rows = sweep_montecarlo(args.bps, EsN0dB, args.nmontecarlo, args.nloops, args.seed, args.device)
    else:
        rows = sweep_quad(args.bps, EsN0dB, args.device)
    write_csv(args.out, column_list(args.bps), rows)
    return rows


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
