"""Mutual information vs SNR by Monte-Carlo, the GPU counterpart of
sims/sim_montecarlo_information.py (its flags and defaults, its CSV columns).

    PYTHONPATH=qam-reconciliation_amd python -m qamr.sim_montecarlo_information \\
        [--out out.csv] [--snr -20 20] [--nsnr 401] [--bps 2] [--niters 256] \\
        [--samples-per-iter 4096] [--seed 0] [--device 0]

Per SNR point the reference calls montecarlo_information `niters` times on `samples-per-iter`
fresh samples and averages the three results in call order; here the niters calls are the B =
niters blocks of one launch pair (montecarlo_information_device), S = samples-per-iter samples
each, the inputs drawn on the device with a seeded torch.Generator as qamr/sim.py draws its frames,
and the mean over the blocks is taken in block order.  One GPU; the reference's --display and
--gnuplot (plotting) are not offered.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(prog="mutual_information_base_scheme",
                                description="Evaluate mutual information vs SNR of the base scheme")
    p.add_argument("--out", default="out.csv")
    p.add_argument("--snr", type=float, nargs=2, default=[-20, 20])
    p.add_argument("--nsnr", type=int, default=401)
    p.add_argument("--bps", type=int, default=2)
    p.add_argument("--niters", type=int, default=(1 << 8))
    p.add_argument("--samples-per-iter", type=int, default=(1 << 12))
    p.add_argument("--seed", type=int, default=0, help="seed of the device generator the samples are drawn from")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def point(pa, esn0db, niters, samples, gen, device):
    """One SNR point (sim_montecarlo_information.py:38-67): the means of the niters blocks' estimates."""
    import torch

    from .mutual_information import P_xhat, montecarlo_information_device
    from .noisemapper import NoiseMapper

    Es = pa.variance
    N0 = Es * (10 ** (-esn0db / 10)) / 2
    nm = NoiseMapper(pa, N0, device=device)
    p_Xhat = P_xhat(nm)
    dev = torch.device("cuda", device)
    B, S = niters, samples
    ld = -(-B // 64) * 64
    a = torch.from_numpy(np.ascontiguousarray(pa.constellation, np.float64)).to(dev)
    x = torch.randint(0, pa.order, (S, ld), generator=gen, device=dev, dtype=torch.int64)
    y = a[x] + nm.noise_sigma * torch.randn((S, ld), generator=gen, device=dev, dtype=torch.float64)
    info = montecarlo_information_device(nm, p_Xhat, x, y, B).cpu().numpy()
    res = [0.0, 0.0, 0.0]
    for f in range(B):          # :53-61, in call order
        for q in range(3):
            res[q] += float(info[q, f])
    return (float(esn0db), res[0] / niters, res[1] / niters, res[2] / niters)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.niters < 1 or args.samples_per_iter < 1:
        raise SystemExit("--niters and --samples-per-iter must be positive")

    import torch

    from ._lib import require_gpu
    from .alphabet import PAMAlphabet

    require_gpu()
    gen = torch.Generator(device=torch.device("cuda", args.device)).manual_seed(args.seed)
    pa = PAMAlphabet(args.bps, 2)
    rows = []
    for esn0db in np.linspace(args.snr[0], args.snr[1], args.nsnr):
        rows.append(point(pa, float(esn0db), args.niters, args.samples_per_iter, gen, args.device))
        print("EsN0dB=%.3f I(X;Xhat)=%.6g I(X;Y)=%.6g I(N,X;Xhat)=%.6g" % rows[-1], flush=True)
    with open(args.out, "w") as fh:  # pandas DataFrame.to_csv layout (sim_montecarlo_information.py:72-78)
        fh.write(",EsN0dB,I(X;Xhat),I(X;Y),I(N,X;Xhat)\n")
        for i, r in enumerate(rows):
            fh.write(f"{i},{r[0]!r},{r[1]!r},{r[2]!r},{r[3]!r}\n")
    return rows


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
