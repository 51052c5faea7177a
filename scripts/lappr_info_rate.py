#!/usr/bin/env python3
"""Rate of the LAPPR information-rate estimator's two launches on resident LAPPRs: `lappr_info`
(k_lappr_info: every term at A scales, the chunk sums) and `lappr_info_total` (k_lappr_info_total: the
ordered sums), each timed by the library's own hipEvent pair (qr_profile_*).  Beside them, on the same
batch: the `demap` launch that produced the LAPPRs (the search demapper) and a device-to-device copy of the
bytes the estimator reads (the LAPPRs and the word), timed by a torch event pair.

Shapes: frames of N = 64 800 bits, B = 4 096 frames, 4-PAM at 3.5 dB and 16-PAM at 13 dB, A = 1, 8 and 16
scales.  Everything is warmed up, then the launches are timed in turn, `--rounds` times over (alternating, so
a drift of the clock hits all of them).  One JSON line per (shape, A).

    python scripts/lappr_info_rate.py [--bits 64800] [--batch 4096] [--rounds 5] [--cases 2:3.5,4:13.0] [--scales 1,8,16]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qam-reconciliation_amd"))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=64800)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="2:3.5,4:13.0", help="bps:snr_dB,...")
    ap.add_argument("--scales", default="1,8,16")
    args = ap.parse_args()
    import numpy as np
    import torch
    import qamr
    from qamr import _lib
    from qamr.mutual_information import lappr_information_device
    from qamr.pipeline import alternating_config, leading_dim, noise_variance

    _lib.require_gpu()
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; hip {torch.version.hip}", flush=True)
    B, ld = args.batch, leading_dim(args.batch)
    ok = True
    for case in args.cases.split(","):
        bps, snr = case.split(":")
        bps, snr = int(bps), float(snr)
        S = args.bits // bps
        pa = qamr.PAMAlphabet(bps, 2.0)
        nm = qamr.NoiseMapper(pa, noise_variance(pa, snr), alternating_config(pa.order))
        a = torch.tensor(pa.constellation, dtype=torch.float64, device="cuda")
        gen = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randint(0, pa.order, (S, ld), generator=gen, device="cuda", dtype=torch.int64)
        y = a[x] + nm.noise_sigma * torch.randn((S, ld), generator=gen, device="cuda", dtype=torch.float64)
        _, nh, word = nm.bob_map_device(y, B)
        del y
        lappr = torch.empty((S * bps, ld), dtype=torch.float64, device="cuda")
        l2, w2 = torch.empty_like(lappr), torch.empty_like(word)
        scales = {A: [float(v) for v in np.linspace(0.4, 1.3, A)] if A > 1 else [1.0] for A in (int(v) for v in args.scales.split(","))}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def copy_ms():
            ev[0].record()
            l2.copy_(lappr)
            w2.copy_(word)
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1])

        for _ in range(2):   # warm-up: code objects, the tables, the clocks
            nm.demap_device(nh, x, B, 1.0, out=lappr)
            copy_ms()
            for al in scales.values():
                lappr_information_device(lappr, word, B, bps, al)
        torch.cuda.synchronize()
        first = {A: lappr_information_device(lappr, word, B, bps, al).total.clone() for A, al in scales.items()}
        t = {"demap": [], "copy": [], **{A: ([], []) for A in scales}}
        _lib.profile_enable(True)
        _lib.profile_select("demap,lappr_info,lappr_info_total")
        last = {}
        for _ in range(args.rounds):
            _lib.profile_reset()
            nm.demap_device(nh, x, B, 1.0, out=lappr)
            torch.cuda.synchronize()
            t["demap"].append(_lib.profile_query("demap")[0])
            t["copy"].append(copy_ms())
            for A, al in scales.items():
                _lib.profile_reset()
                last[A] = lappr_information_device(lappr, word, B, bps, al)
                torch.cuda.synchronize()
                (m, n1), (s, n2) = _lib.profile_query("lappr_info"), _lib.profile_query("lappr_info_total")
                assert n1 == 1 and n2 == 1, (n1, n2)
                t[A][0].append(m)
                t[A][1].append(s)
        _lib.profile_enable(False)
        _lib.profile_select(None)
        nbytes = lappr.numel() * 8 + word.numel()
        for A, al in scales.items():
            same = torch.equal(last[A].total.view(torch.int64), first[A].view(torch.int64))
            ok &= same
            m, s = median(t[A][0]), median(t[A][1])
            I, _, ber = last[A].rates(S)
            terms = S * bps * B * A
            print(json.dumps({
                "bps": bps, "snr_dB": snr, "bits": S * bps, "B": B, "ld": ld, "A": A, "rounds": args.rounds,
                "repeatable_bits": same,
                "lappr_info": {"ms_median": round(m, 4), "ms_min": round(min(t[A][0]), 4), "ms_max": round(max(t[A][0]), 4),
                               "Gterms_per_s": round(terms / m / 1e6, 2), "GB_per_s_read": round(nbytes / m / 1e6, 1)},
                "lappr_info_total": {"ms_median": round(s, 4), "ms_min": round(min(t[A][1]), 4), "ms_max": round(max(t[A][1]), 4)},
                "demap_ms_median": round(median(t["demap"]), 4),
                "copy": {"bytes": nbytes, "ms_median": round(median(t["copy"]), 4),
                         "GB_per_s_read": round(nbytes / median(t["copy"]) / 1e6, 1)},
                "alphas": al, "I": [float(v) for v in I], "ber_level": [float(v) for v in ber]}), flush=True)
        del lappr, l2, w2, word, nh, x, last, first
        torch.cuda.empty_cache()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
