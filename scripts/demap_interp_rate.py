#!/usr/bin/env python3
"""Rate of the two soft demappers on one resident batch, in the same process on the same GPU:
`demap` (k_demap_wave, the g_inv_search demapper) and `demap_interp` (k_demap_interp_wave,
formulation 1 on the interpolated g_inv) with both index searches (knob interp_fast 1 / 0; the
shortcut search at every coarse-table segment size of --seg, knob interp_seg = log2 entries).

Shapes: the bench's frames of N = 64800 bits, B = 4096: S = 32400 symbols (4-PAM) at 3 dB and
S = 16200 (16-PAM) at 13 dB.  Every variant is warmed up, then the variants are timed in turn,
`--rounds` times over (alternating, so a drift of the clock or the host hits all of them), each
launch by the library's own hipEvent pair (qr_profile_*).  Printed per variant: the median,
minimum and maximum ms per launch and the algorithmic GB/s, (16 + 8 bps) S B bytes (n, j in, bps
LAPPRs out) over the median.  All interp variants must agree bit for bit.

    python scripts/demap_interp_rate.py [--batch 4096] [--rounds 9] [--seg 4] [--cases 2:3.0:32400,4:13.0:16200]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qam-reconciliation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--seg", default=None, help="interp_seg values to time, e.g. 6,5,4,3 (default: the knob's value)")
    ap.add_argument("--cases", default="2:3.0:32400,4:13.0:16200", help="bps:snr_dB:S,...")
    args = ap.parse_args()
    import torch
    import qamr
    from qamr import _lib
    from qamr.pipeline import alternating_config, leading_dim, noise_variance

    _lib.require_gpu()
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; hip {torch.version.hip}", flush=True)
    B, ld = args.batch, leading_dim(args.batch)
    saved = _lib.tune_get("interp_fast"), _lib.tune_get("interp_seg")
    ok = True
    segs = [saved[1]] if args.seg is None else [int(v) for v in args.seg.split(",")]
    # (label, profile name, interp_fast, interp_seg); the literal search does not read the coarse table
    variants = ([("demap", "demap", None, None)] +
                [(f"demap_interp fast=1 seg={1 << g}", "demap_interp", 1, g) for g in segs] +
                [("demap_interp fast=0", "demap_interp", 0, segs[-1])])
    try:
        for case in args.cases.split(","):
            bps, snr, S = case.split(":")
            bps, snr, S = int(bps), float(snr), int(S)
            pa = qamr.PAMAlphabet(bps, 2.0)
            nm = qamr.NoiseMapper(pa, noise_variance(pa, snr), alternating_config(pa.order))
            gen = torch.Generator(device="cuda").manual_seed(0)
            x = torch.randint(0, pa.order, (S, ld), generator=gen, device="cuda", dtype=torch.int64)
            a = torch.tensor(pa.constellation, dtype=torch.float64, device="cuda")
            y = a[x] + nm.noise_sigma * torch.randn((S, ld), generator=gen, device="cuda", dtype=torch.float64)
            _, nhat, _ = nm.bob_map_device(y, B)
            del y
            n_points, nondecreasing = nm.grid_info()
            outs = {v[0]: torch.empty((S * bps, ld), dtype=torch.float64, device="cuda") for v in variants}

            def launch(name, fast, seg):
                if fast is None:
                    nm.demap_device(nhat, x, B, 1.0, out=outs[name])
                else:
                    _lib.tune_set("interp_fast", fast)
                    _lib.tune_set("interp_seg", seg)   # another value: the grid is rebuilt before the launch
                    nm.demap_simplified_device(nhat, x, B, 1.0, out=outs[name])

            for name, _, fast, seg in variants:   # warm-up: code objects, the grid, the clocks
                for _ in range(2):
                    launch(name, fast, seg)
            torch.cuda.synchronize()
            _lib.profile_enable(True)
            _lib.profile_select("demap,demap_interp")
            ms = {v[0]: [] for v in variants}
            for _ in range(args.rounds):
                for name, prof, fast, seg in variants:
                    _lib.profile_reset()
                    launch(name, fast, seg)
                    torch.cuda.synchronize()
                    t, n = _lib.profile_query(prof)
                    assert n == 1, (name, n)
                    ms[name].append(t)
            _lib.profile_enable(False)
            _lib.profile_select(None)
            ref = outs[variants[-1][0]][:, :B].view(torch.int64)
            same = all(torch.equal(outs[v[0]][:, :B].view(torch.int64), ref) for v in variants[1:-1])
            ok &= same
            nbytes = (16 + 8 * bps) * S * B
            row = {"bps": bps, "snr_dB": snr, "S": S, "B": B, "n_points": n_points, "nondecreasing": nondecreasing,
                   "interp_bodies_bit_identical": same, "bytes": nbytes, "rounds": args.rounds, "variants": {}}
            for name in ms:
                t = sorted(ms[name])
                med = t[len(t) // 2]
                row["variants"][name] = {"ms_median": round(med, 3), "ms_min": round(t[0], 3), "ms_max": round(t[-1], 3),
                                         "GBps": round(nbytes / med / 1e6, 1)}
            print(json.dumps(row), flush=True)
            del outs, x, nhat, nm
            torch.cuda.empty_cache()
    finally:
        _lib.tune_set("interp_fast", saved[0])
        _lib.tune_set("interp_seg", saved[1])
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
