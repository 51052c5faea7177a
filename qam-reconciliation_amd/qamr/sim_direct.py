"""Es/N0-sweep CLI, the GPU counterpart of sims/sim_direct.py: qamr.sim_decode with the first
CSV column named EsN0dB (the two reference scripts compute the same thing).

    PYTHONPATH=qam-reconciliation_amd python -m qamr.sim_direct EDGEFILE [options of qamr.sim_decode]
"""
from __future__ import annotations

import sys

from . import sim_decode


def build_parser():
    return sim_decode.build_parser("sim_direct")


def main(argv=None):
    return sim_decode.main(argv, column="EsN0dB", prog="sim_direct")


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
