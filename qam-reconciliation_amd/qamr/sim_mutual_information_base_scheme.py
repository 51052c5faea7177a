"""I(N,X;Xhat), I(X;Xhat) and I(X;Y) vs SNR by quadrature, the GPU counterpart of
sims/sim_mutual_information_base_scheme.py (its flags and defaults, its CSV columns).

    PYTHONPATH=qam-reconciliation_amd python -m qamr.sim_mutual_information_base_scheme \\
        [--out out.csv] [--snr 0 5] [--nsnr 11] [--bps 2] [--device 0]

Per SNR point the reference builds a NoiseMapper (all-zero sign configuration) and calls
mutual_information_base_scheme, mutual_information_X_Xhat and mutual_information_X_Y on it
(:36-59); here all SNR points form one batch per integral kind (mutual_information_quad_batch: one
launch per round of bisections for the whole sweep) and I(X;Xhat) is the host's closed form.  An
integral for which quad would warn is reported on stderr.  One GPU; the reference's --display and
--gnuplot (plotting) are not offered.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

COLUMNS = ["EsN0dB", "EbN0dB base", "I(N,X;Xhat)", "EbN0dB X;Xhat", "I(X;Xhat)", "EbN0dB X;Y", "I(X;Y)"]


def build_parser():
    p = argparse.ArgumentParser(prog="mutual_information_base_scheme",
                                description="Evaluate mutual information vs SNR of the base scheme")
    p.add_argument("--out", default="out.csv")
    p.add_argument("--snr", type=float, nargs=2, default=[0, 5])
    p.add_argument("--nsnr", type=int, default=11)
    p.add_argument("--bps", type=int, default=2)
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def sweep(bps, EsN0dB, device=0):
    """The rows of sim_mutual_information_base_scheme.py:36-59 for every SNR point."""
    from .alphabet import PAMAlphabet
    from .mutual_information import (P_xhat, _warn, mutual_information_quad_batch, mutual_information_X_Xhat)
    from .noisemapper import NoiseMapper

    pa = PAMAlphabet(bps, 2)
    Es = pa.variance
    nms = [NoiseMapper(pa, Es * (10 ** (-float(e) / 10)) / 2, device=device) for e in EsN0dB]
    pXs = [P_xhat(nm) for nm in nms]
    Ib, eb, _, ib = mutual_information_quad_batch("base", nms, pXs)
    Iy, ey, _, iy = mutual_information_quad_batch("X_Y", nms)
    rows = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, e in enumerate(EsN0dB):
            _warn(int(ib[k]), float(eb[k]))
            _warn(int(iy[k]), float(ey[k]))
            e = float(e)
            I_base, I_XY = float(Ib[k]), float(Iy[k])
            I_XXhat = mutual_information_X_Xhat(nms[k], pXs[k])
            rows.append((e, float(e - 10 * np.log10(I_base)), I_base, float(e - 10 * np.log10(I_XXhat)), I_XXhat,
                         float(e - 10 * np.log10(I_XY)), I_XY))
    return rows


def write_csv(path, columns, rows):
    with open(path, "w") as fh:  # pandas DataFrame.to_csv layout
        fh.write("," + ",".join(columns) + "\n")
        for i, r in enumerate(rows):
            fh.write(f"{i}," + ",".join(repr(float(v)) for v in r) + "\n")


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.nsnr < 1:
        raise SystemExit("--nsnr must be positive")
    from ._lib import require_gpu

    require_gpu()
    rows = sweep(args.bps, np.linspace(args.snr[0], args.snr[1], args.nsnr), args.device)
    for r in rows:
        print("EsN0dB=%.3f I(N,X;Xhat)=%.6g I(X;Xhat)=%.6g I(X;Y)=%.6g" % (r[0], r[2], r[4], r[6]), flush=True)
    write_csv(args.out, COLUMNS, rows)
    return rows


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
