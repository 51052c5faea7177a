#!/usr/bin/env python3
"""Rate of the binary-channel code evaluation (qamr.sim_binary): frames/s of one
BinaryChannelSimulator.run_point on the N = 64 800 code, and the hipEvent time of the LLR launch
(`biawgn_llr`, the library's own event pair) beside qr_stream_copy moving the same number of bytes
(17 B per element: the word byte and the draw read, the LLR written; the copy reads and writes half
of that each).  One warm-up point, then `--points` timed ones; no threshold is attached.

    python scripts/binary_channel_rate.py [--snr 1.0] [--batch 4096] [--batches 2] [--maxiter 30] [--points 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qam-reconciliation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snr", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--points", type=int, default=3)
    ap.add_argument("--channel", default="biawgn")
    args = ap.parse_args()
    import torch
    import qamr
    from qamr import _lib, codes
    from qamr.pipeline import leading_dim
    from qamr.sim_binary import BinaryChannelSimulator

    _lib.require_gpu()
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; hip {torch.version.hip}", flush=True)
    vid, cid = codes.dvbs2_like_half()
    dec = qamr.Decoder(vid, cid)
    sim = BinaryChannelSimulator(dec, args.channel, args.maxiter, batch=args.batch)
    loops = args.batch * args.batches
    sim.run_point(args.snr, args.batch, 1 << 60, seed=99)       # warm-up: code objects, workspace
    torch.cuda.synchronize()
    name = "bsc_llr" if args.channel == "bsc" else "biawgn_llr"
    _lib.profile_enable(True)
    _lib.profile_select(name)
    _lib.profile_reset()
    rates, res = [], None
    for p in range(args.points):
        t0 = time.perf_counter()
        res = sim.run_point(args.snr, loops, 1 << 60, seed=p)
        torch.cuda.synchronize()
        rates.append(loops / (time.perf_counter() - t0))
    ms, n = _lib.profile_query(name)
    _lib.profile_enable(False)
    _lib.profile_select(None)
    ld = leading_dim(args.batch)
    elems = dec.vnum * ld
    half = elems * 17 // 2 // 16 * 16                           # bytes the copy reads (and writes)
    src = torch.zeros(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    L = _lib.load()
    copy_ms = []
    for _ in range(2 + args.points * args.batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(L.qr_stream_copy(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), half,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        b.record()
        b.synchronize()
        copy_ms.append(a.elapsed_time(b))
    copy_ms = sorted(copy_ms[2:])
    rates.sort()
    print(json.dumps({
        "channel": args.channel, "point": args.snr, "V": dec.vnum, "B": args.batch, "ld": ld, "maxiter": args.maxiter,
        "frames_per_point": loops, "result": list(res),
        "frames_per_s": {"median": round(rates[len(rates) // 2], 1), "min": round(rates[0], 1), "max": round(rates[-1], 1)},
        "llr_launch": {"launches": n, "ms_mean": round(ms / max(n, 1), 4), "bytes": elems * 17,
                       "TB_per_s": round(elems * 17 / (ms / max(n, 1)) / 1e9, 3)},
        "stream_copy_same_bytes": {"ms_median": round(copy_ms[len(copy_ms) // 2], 4), "ms_min": round(copy_ms[0], 4),
                                   "bytes": 2 * half, "TB_per_s": round(2 * half / copy_ms[len(copy_ms) // 2] / 1e9, 3)},
    }), flush=True)


if __name__ == "__main__":
    main()
