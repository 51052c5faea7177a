"""The information rate the LAPPRs carry to the bit-wise decoder (the BICM generalised mutual
information, bits per symbol) vs SNR and vs the scale alpha of the LAPPRs: the curve that says which
``--alpha`` to give the reconciliation simulations, without running a decoder.

    PYTHONPATH=qam-reconciliation_amd python -m qamr.sim_lappr_information \\
        [--out out.csv] [--bps 2] [--snr 0 6] [--nsnr 13] [--symbols 32400] [--frames 256] \\
        [--alphas 0.5 0.6 0.7 0.8 0.9 1.0] [--mode softening|direct|hard] [--demapper search|simplified] \\
        [--configuration-base] [--seed 0] [--device 0]

Per SNR point one batch of `frames` frames of `symbols` symbols is drawn and mapped as qamr/sim.py
does it (llr_source: no code is involved), the demapper runs once at alpha = 1, and one launch pair
(lappr_information_device) evaluates every scale.  One CSV row per (SNR point, alpha):
EsN0dB,alpha,I,I_0..I_{bps-1},ber_0..ber_{bps-1}; the best alpha of every point (the first maximum of
I) is printed.  One GPU.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(prog="sim_lappr_information",
                                description="Information rate of the LAPPRs vs SNR and LAPPR scale")
    p.add_argument("--out", default="out.csv")
    p.add_argument("--bps", type=int, default=2)
    p.add_argument("--snr", type=float, nargs=2, default=[0, 6], metavar=("LO", "HI"))
    p.add_argument("--nsnr", type=int, default=13)
    p.add_argument("--symbols", type=int, default=32400, help="symbols per frame")
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--alphas", type=float, nargs="+", default=[1.0])
    p.add_argument("--mode", choices=("softening", "direct", "hard"), default="softening")
    p.add_argument("--demapper", choices=("search", "simplified"), default="search")
    p.add_argument("--configuration-base", action="store_true", help="all-zero sign configuration (default: alternating)")
    p.add_argument("--seed", type=int, default=0, help="seed of the device generator the frames are drawn from")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def header(bps: int) -> str:
    return ",".join(["EsN0dB", "alpha", "I"] + [f"I_{k}" for k in range(bps)] + [f"ber_{k}" for k in range(bps)])


def best_alpha(alphas, I) -> float:
    """The scale of the first maximum of I."""
    return float(alphas[int(np.argmax(np.asarray(I, np.float64)))])


def point_seed(seed: int, index: int) -> int:
    """The generator seed of SNR point `index`: every point draws from its own stream."""
    return int(seed) * 1000003 + int(index)


def point(pa, esn0db, symbols, frames, alphas, mode, demapper, configuration_base, seed, device):
    """One SNR point: (I [A], I_level [A, bps], ber_level [bps]) of `frames` seeded frames."""
    import torch

    from .mutual_information import lappr_information_device
    from .noisemapper import NoiseMapper
    from .pipeline import alternating_config
    from .sim import llr_source

    Es = pa.variance
    two_var = Es * (10 ** (-esn0db / 10))
    N0 = two_var / 2
    cfg = None
    if mode == "softening":
        cfg = np.zeros(pa.order, np.uint8) if configuration_base else alternating_config(pa.order)
    nm = NoiseMapper(pa, N0, cfg, device=device)
    gen = torch.Generator(device=torch.device("cuda", device)).manual_seed(seed)
    lappr, word = llr_source(nm, pa, symbols, frames, gen, mode, demapper, 1.0, two_var)
    return lappr_information_device(lappr, word, frames, pa.bit_per_symbol, alphas).rates(symbols)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.nsnr < 1 or args.symbols < 1 or args.frames < 1:
        raise SystemExit("--nsnr, --symbols and --frames must be positive")
    from .mutual_information import _check_info_args

    try:
        _check_info_args(args.bps, args.alphas)
    except ValueError as e:
        raise SystemExit(str(e))

    from ._lib import require_gpu
    from .alphabet import PAMAlphabet

    require_gpu()
    pa = PAMAlphabet(args.bps, 2)
    rows = []
    for i, esn0db in enumerate(np.linspace(args.snr[0], args.snr[1], args.nsnr)):
        I, I_level, ber = point(pa, float(esn0db), args.symbols, args.frames, args.alphas, args.mode, args.demapper,
                                args.configuration_base, point_seed(args.seed, i), args.device)
        for a, alpha in enumerate(args.alphas):
            rows.append((float(esn0db), float(alpha), float(I[a]), *[float(v) for v in I_level[a]], *[float(v) for v in ber]))
        print("EsN0dB=%.3f best alpha=%g I=%.6g  (%s)" % (
            esn0db, best_alpha(args.alphas, I), float(np.max(I)),
            " ".join("I(%g)=%.6g" % (al, v) for al, v in zip(args.alphas, I))), flush=True)
    with open(args.out, "w") as fh:
        fh.write(header(args.bps) + "\n")
        for r in rows:
            fh.write(",".join(repr(v) for v in r) + "\n")
    return rows


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
