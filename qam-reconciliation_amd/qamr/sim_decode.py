"""Eb/N0-sweep CLI of an LDPC code on the binary-input AWGN channel, the GPU counterpart of
sims/sim_decode.py (arguments of sim_decode.py:13-33, CSV of :127-133).

    PYTHONPATH=qam-reconciliation_amd python -m qamr.sim_decode EDGEFILE \\
        [--out out.csv] [--maxiter 30] [--minerr 20] [--simloops 30] [--snr 0 5] [--nsnr 11] \\
        [--alpha 1.0] [--hard] [--batch 4096] [--seed 0] [--schedule {flooding,layered}]

Instead of one OS process per point (parfor), every point runs batched on the GPU(s); launched
under torchrun, each rank takes its share of every batch (qamr.sim_binary, qamr.dist).
qamr.sim_direct is the same program with the reference's other column name.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np


def build_parser(prog: str = "sim_decode"):
    p = argparse.ArgumentParser(prog=prog, description="Evaluate BER for LDPC codes vs Raw BER")
    p.add_argument("edgefile", help="CSV with a 'vid' and a 'cid' columns representing an edge per line")
    p.add_argument("--out", default="out.csv")
    p.add_argument("--maxiter", default=30, type=int, help="Maximum number of iterations for the decoder")
    p.add_argument("--minerr", default=20, type=int, help="Minimum number of bit errors for early exit")
    p.add_argument("--first_row", default=True, action="store_true",
                   help="Flag: does the first line of the csv contain the number of edges")
    p.add_argument("--simloops", default=30, type=int, help="Number of frames per SNR point")
    p.add_argument("--snr", type=float, nargs=2, default=[0, 5], help="Initial and final SNR [dB]")
    p.add_argument("--nsnr", type=int, default=11, help="Number of equally spaced SNR [dB] points")
    p.add_argument("--alpha", type=float, default=1.0, help="Extra multiplicative coefficient for the LLR")
    p.add_argument("--hard", action="store_true", default=False, help="Hard-decide the channel output")
    p.add_argument("--batch", type=int, default=4096, help="frames per GPU per batch")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--schedule", choices=("flooding", "layered"), default="flooding",
                   help="Decode schedule: the reference's flooding one, or the layered (serial-check) one of this "
                        "library, which needs about half the iterations (its LAPPRs and iteration counts differ)")
    return p


def write_csv(path: str, column: str, rows):
    """pandas DataFrame.to_csv layout (sim_decode.py:127-133): an unnamed index column, then
    `column`, ber, fer, iters."""
    with open(path, "w") as fh:
        fh.write(f",{column},ber,fer,iters\n")
        for i, r in enumerate(rows):
            fh.write(f"{i},{r[0]!r},{r[1]!r},{r[2]!r},{r[3]!r}\n")


def sweep(args, channel: str, points, column: str):
    """Run `points` on `channel` and, on rank 0, write the CSV with `column` first; returns the rows."""
    from . import dist
    from .codes import load_edge_csv
    from .decoder import Decoder
    from .sim_binary import BinaryChannelSimulator

    world, rank, local = dist.init()
    vid, cid = load_edge_csv(args.edgefile)  # counts row skipped (sim_decode.py:52-53: vid[1:])
    dec = Decoder(vid, cid, device=local)
    sim = BinaryChannelSimulator(dec, channel, args.maxiter, getattr(args, "alpha", 1.0), args.batch, device=local,
                                 schedule=args.schedule)
    rows = []
    for x in points:
        rows.append(sim.run_point(float(x), args.simloops, args.minerr, args.seed))
        if rank == 0:
            print(f"{column}=%.6g ber=%.6g fer=%.6g iters=%.3f" % rows[-1], flush=True)
    if rank == 0:
        write_csv(args.out, column, rows)
    dist.finalize()
    return rows


def main(argv=None, column: str = "EbN0dB", prog: str = "sim_decode"):
    args = build_parser(prog).parse_args(argv)
    return sweep(args, "biawgn_hard" if args.hard else "biawgn", np.linspace(args.snr[0], args.snr[1], args.nsnr),
                 column)


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
