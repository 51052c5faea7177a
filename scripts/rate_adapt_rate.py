#!/usr/bin/env python3
"""Rate adaptation, measured: the launch times of the expand (`rate_adapt_expand`) and of the row-listed
count (`count_rows`) beside the `demap` launch that feeds them and beside device-to-device copies, and what
shortening, puncturing and blind rounds do to `codes.dvbs2_like_half()`.

Launch times: frames of N = 64 800 bits, B = 4 096, 4-PAM, (p, s) = (6 480, 0) and (0, 6 480).  The three
launches are timed by the library's own hipEvent pairs (qr_profile_*), the copies (`dst.copy_(src)`, LAPPRs and
bits) by a torch event pair: one of the payload's n rows, one of the output's V rows.  The expand reads the n
rows and writes the V rows, so the copy "of the same bytes" is the mean of the two.  Everything is warmed up
twice, then timed in turn `--rounds` times over.  One JSON line per (p, s).

Effect (`--effect`): dvbs2_like_half, 4-PAM, alpha 0.7, the search demapper, 50 iterations, `--frames` frames
per row through qamr.sim_rate_adapt.run_point.  One JSON line per row.

    python scripts/rate_adapt_rate.py [--bits 64800] [--batch 4096] [--rounds 5] [--effect] [--frames 1024]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qam-reconciliation_amd"))


def stats(v):
    s = sorted(v)
    return {"ms_median": round(s[len(s) // 2], 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4)}


def launches(args):
    import numpy as np
    import torch
    import qamr
    from qamr import _lib
    from qamr.pipeline import alternating_config, leading_dim, noise_variance
    from qamr.rate_adapt import RateAdaption

    V, B, ld, bps, snr = args.bits, args.batch, leading_dim(args.batch), 2, 4.0
    pa = qamr.PAMAlphabet(bps, 2.0)
    nm = qamr.NoiseMapper(pa, noise_variance(pa, snr), alternating_config(pa.order))
    a = torch.tensor(pa.constellation, dtype=torch.float64, device="cuda")
    order = np.random.default_rng(0).permutation(V)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def copy_ms(dst, src):
        ev[0].record()
        for d, s in zip(dst, src):
            d.copy_(s)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    for p, s in ((V // 10, 0), (0, V // 10)):
        ad = RateAdaption.from_order(order, p, s)
        S = ad.n // bps
        gen = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randint(0, pa.order, (S, ld), generator=gen, device="cuda", dtype=torch.int64)
        y = a[x] + nm.noise_sigma * torch.randn((S, ld), generator=gen, device="cuda", dtype=torch.float64)
        _, nh, word_pay = nm.bob_map_device(y, B)
        del y
        fill = torch.randint(0, 2, (p + s, ld), dtype=torch.uint8, generator=gen, device="cuda")
        lappr_pay = torch.empty((ad.n, ld), dtype=torch.float64, device="cuda")
        out = (torch.empty((V, ld), dtype=torch.float64, device="cuda"), torch.empty((V, ld), dtype=torch.uint8, device="cuda"))
        pay2 = (torch.empty_like(lappr_pay), torch.empty_like(word_pay))
        out2 = (torch.empty_like(out[0]), torch.empty_like(out[1]))
        succ = torch.ones(B, dtype=torch.uint8, device="cuda")
        its = torch.ones(B, dtype=torch.int32, device="cuda")
        ferr = torch.empty(B, dtype=torch.int32, device="cuda")
        counters = torch.zeros(5, dtype=torch.int64, device="cuda")

        def once():
            nm.demap_device(nh, x, B, 1.0, out=lappr_pay)
            ad.expand_device(lappr_pay, word_pay, fill, B, out=out)
            ad.count_errors_device(B, ld, out[0], out[1], succ, its, ferr, counters)

        for _ in range(2):   # warm-up: code objects, the tables, the clocks
            once()
            copy_ms(pay2, (lappr_pay, word_pay))
            copy_ms(out2, out)
        torch.cuda.synchronize()
        first = out[0].clone()
        t = {k: [] for k in ("demap", "rate_adapt_expand", "count_rows", "copy_payload", "copy_output")}
        _lib.profile_enable(True)
        _lib.profile_select("demap,rate_adapt_expand,count_rows")
        for _ in range(args.rounds):
            _lib.profile_reset()
            once()
            torch.cuda.synchronize()
            for k in ("demap", "rate_adapt_expand", "count_rows"):
                ms, n = _lib.profile_query(k)
                assert n == 1, (k, n)
                t[k].append(ms)
            t["copy_payload"].append(copy_ms(pay2, (lappr_pay, word_pay)))
            t["copy_output"].append(copy_ms(out2, out))
        _lib.profile_enable(False)
        _lib.profile_select(None)
        same = torch.equal(out[0].view(torch.int64), first.view(torch.int64))
        read = ad.n * ld * 9 + (p + s) * ld
        written = V * ld * 9
        yard = [(u + w) / 2 for u, w in zip(t["copy_payload"], t["copy_output"])]
        med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
        print(json.dumps({
            "V": V, "B": B, "ld": ld, "p": p, "s": s, "n": ad.n, "rounds": args.rounds, "repeatable_bits": same,
            "bytes_read": read, "bytes_written": written,
            **{k: stats(v) for k, v in t.items()}, "copy_same_bytes": stats(yard),
            "expand_GB_per_s": round((read + written) / med(t["rate_adapt_expand"]) / 1e6, 1),
            "expand_over_copy": round(med(t["rate_adapt_expand"]) / med(yard), 3),
            "count_rows_GB_per_s_read": round(ad.n * ld * 9 / med(t["count_rows"]) / 1e6, 1)}), flush=True)
        del x, nh, word_pay, fill, lappr_pay, out, pay2, out2, first
        torch.cuda.empty_cache()


def effect(args):
    import qamr
    from qamr import codes
    from qamr.rate_adapt import RateAdaption, untainted_order
    from qamr.sim import Simulator
    from qamr.sim_rate_adapt import COLUMNS, run_point

    vid, cid = codes.dvbs2_like_half()
    dec = qamr.Decoder(vid, cid)
    order, u = untainted_order(vid, cid, 0)
    print(json.dumps({"code": "dvbs2_like_half", "untainted_u": u}), flush=True)
    V = order.size
    rows = [(3.25, 0, 0, 0, 1), (3.25, 0, V // 20, 0, 1), (3.25, 0, V // 10, 0, 1),
            (4.5, 0, 0, 0, 1), (4.5, V // 20, 0, 0, 1), (4.5, V // 10, 0, 0, 1),
            (4.0, V // 10, 0, 4, V // 40)]
    for i, (snr, p, s, rounds, step) in enumerate(rows):
        sim = Simulator(dec, 2, "softening", 50, 0.7, args.eff_batch, adapt=RateAdaption.from_order(order, p, s))
        r = run_point(sim, snr, args.frames, rounds, step, 0, i)
        print(json.dumps({"p": p, "s": s, "blind_rounds": rounds, "blind_step": step, "frames": args.frames,
                          "rate": sim.adapt.rate(sim.K), **dict(zip(COLUMNS, r))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=64800)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--effect", action="store_true", help="the FER rows instead of the launch times")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--eff-batch", type=int, default=1024)
    args = ap.parse_args()
    import torch
    from qamr import _lib

    _lib.require_gpu()
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; hip {torch.version.hip}", flush=True)
    (effect if args.effect else launches)(args)


if __name__ == "__main__":
    main()
