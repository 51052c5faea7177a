"""Raw-BER-sweep CLI of an LDPC code on the binary symmetric channel, the GPU counterpart of
sims/sim_bsc.py (arguments of sim_bsc.py:10-28, CSV of :85-89).

    PYTHONPATH=qam-reconciliation_amd python -m qamr.sim_bsc EDGEFILE \\
        [--out out.csv] [--maxiter 30] [--minerr 20] [--simloops 30] [--rber 0.01 0.04] \\
        [--rpoints 31] [--batch 4096] [--seed 0] [--schedule {flooding,layered}]
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from .sim_decode import sweep


def build_parser():
    p = argparse.ArgumentParser(prog="sim_bsc", description="Evaluate BER for LDPC codes vs Raw BER")
    p.add_argument("edgefile", help="CSV with a 'vid' and a 'cid' columns representing an edge per line")
    p.add_argument("--out", default="out.csv")
    p.add_argument("--maxiter", default=30, type=int, help="Maximum number of iterations for the decoder")
    p.add_argument("--minerr", default=20, type=int, help="Bit errors to exceed for early exit")
    p.add_argument("--first_row", default=True, action="store_true",
                   help="Flag: does the first line of the csv contain the number of edges")
    p.add_argument("--simloops", default=30, type=int, help="Number of frames per raw-BER point")
    p.add_argument("--rber", type=float, nargs=2, default=[0.01, 0.04], help="Initial and final raw BER")
    p.add_argument("--rpoints", type=int, default=31, help="Number of equally spaced raw-BER points")
    p.add_argument("--batch", type=int, default=4096, help="frames per GPU per batch")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--schedule", choices=("flooding", "layered"), default="flooding",
                   help="Decode schedule: the reference's flooding one, or the layered (serial-check) one of this "
                        "library, which needs about half the iterations (its LAPPRs and iteration counts differ)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    return sweep(args, "bsc", np.linspace(args.rber[0], args.rber[1], args.rpoints), "f")


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
