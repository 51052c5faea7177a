#!/usr/bin/env python3
"""Rate of the Monte-Carlo mutual-information estimator's two launches on resident inputs:
`mi_terms` (k_mi_terms: the three per-sample terms) and `mi_sum` (k_mi_sum: the sequential block sums),
each timed by the library's own hipEvent pair (qr_profile_*).

Shapes: S = 4096 samples per block (the CLI's --samples-per-iter default), B = 256 blocks (its --niters
default, i.e. one SNR point of the CLI) and B = 4096, for 4-PAM and 16-PAM.  Every shape is warmed up,
then the shapes are timed in turn, `--rounds` times over (alternating, so a drift of the clock or the
host hits all of them); a shape's launch pair is repeated `--reps` times per round so that the timed
window is not a single short launch.  Printed per shape: the median, minimum and maximum ms per launch
of both kernels, samples/s and ns per sample of mi_terms (S B samples over the median), and mi_sum's
share of the pair.

    python scripts/mi_rate.py [--samples 4096] [--batches 256,4096] [--rounds 7] [--reps 3] [--cases 2:4.0,4:13.0]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qam-reconciliation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--batches", default="256,4096")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="2:4.0,4:13.0", help="bps:snr_dB,...")
    args = ap.parse_args()
    import torch
    import qamr
    from qamr import _lib
    from qamr.mutual_information import P_xhat, montecarlo_information_device
    from qamr.pipeline import leading_dim, noise_variance

    _lib.require_gpu()
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; hip {torch.version.hip}", flush=True)
    S = args.samples
    shapes = []
    for case in args.cases.split(","):
        bps, snr = case.split(":")
        bps, snr = int(bps), float(snr)
        pa = qamr.PAMAlphabet(bps, 2.0)
        nm = qamr.NoiseMapper(pa, noise_variance(pa, snr))   # the CLI's NoiseMapper: default configuration
        pX = P_xhat(nm)
        a = torch.tensor(pa.constellation, dtype=torch.float64, device="cuda")
        for B in (int(v) for v in args.batches.split(",")):
            ld = leading_dim(B)
            gen = torch.Generator(device="cuda").manual_seed(0)
            x = torch.randint(0, pa.order, (S, ld), generator=gen, device="cuda", dtype=torch.int64)
            y = a[x] + nm.noise_sigma * torch.randn((S, ld), generator=gen, device="cuda", dtype=torch.float64)
            info = torch.empty((3, ld), dtype=torch.float64, device="cuda")
            terms = torch.empty((3, S, ld), dtype=torch.float64, device="cuda")
            shapes.append({"bps": bps, "snr_dB": snr, "B": B, "ld": ld, "nm": nm, "pX": pX, "x": x, "y": y, "info": info,
                           "terms": terms, "t": [], "s": []})

    def launch(sh):
        montecarlo_information_device(sh["nm"], sh["pX"], sh["x"], sh["y"], sh["B"], terms=sh["terms"], out=sh["info"])

    for sh in shapes:   # warm-up: code objects, the grid, the tables, the clocks
        for _ in range(2):
            launch(sh)
    torch.cuda.synchronize()
    first = [sh["info"][:, :sh["B"]].clone() for sh in shapes]
    _lib.profile_enable(True)
    _lib.profile_select("mi_terms,mi_sum")
    for _ in range(args.rounds):
        for sh in shapes:
            _lib.profile_reset()
            for _ in range(args.reps):
                launch(sh)
            torch.cuda.synchronize()
            (t, nt), (s, ns) = _lib.profile_query("mi_terms"), _lib.profile_query("mi_sum")
            assert nt == args.reps and ns == args.reps, (nt, ns)
            sh["t"].append(t / nt)
            sh["s"].append(s / ns)
    _lib.profile_enable(False)
    _lib.profile_select(None)
    ok = True
    for sh, f in zip(shapes, first):
        same = torch.equal(sh["info"][:, :sh["B"]].view(torch.int64), f.view(torch.int64))
        ok &= same
        t, s = sorted(sh["t"]), sorted(sh["s"])
        tm, sm = t[len(t) // 2], s[len(s) // 2]
        n = S * sh["B"]
        print(json.dumps({
            "bps": sh["bps"], "snr_dB": sh["snr_dB"], "S": S, "B": sh["B"], "rounds": args.rounds, "reps": args.reps,
            "repeatable_bits": same,
            "mi_terms": {"ms_median": round(tm, 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4),
                         "Msamples_per_s": round(n / tm / 1e3, 1), "ns_per_sample": round(tm * 1e6 / n, 4)},
            "mi_sum": {"ms_median": round(sm, 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4),
                       "share_of_pair": round(sm / (sm + tm), 4)},
            "mean_info": [float(v) for v in sh["info"][:, :sh["B"]].mean(dim=1).cpu()]}), flush=True)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
