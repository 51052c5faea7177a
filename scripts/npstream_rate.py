#!/usr/bin/env python3
"""Rate of the simulations on numpy's stream (stream="numpy", qamr.npstream) beside torch's: frames/s
of one Simulator.run_snr on the N = 64 800 code at 4-PAM, the hipEvent time of the four launches of
the generator (`np_words`, `np_scan`, `np_chain`, `np_fill`: the library's own event pairs), and what
numpy's own draws of one frame cost on this host.  One warm-up run per mode, then `--points` timed
ones; no threshold is attached.  With --parent-lib the torch-mode rate is measured again in a child
process on that library (QAMR_LIB), in the same session.

    python scripts/npstream_rate.py [--snr 4.0] [--batch 4096] [--frames 8192] [--maxiter 50] [--points 3]
                                    [--parent-lib PATH/libqamr.so]
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qam-reconciliation_amd"))

NAMES = ("np_words", "np_scan", "np_chain", "np_fill")


def rate(sim, args, torch):
    rates = []
    for p in range(args.points):
        t0 = time.perf_counter()
        res = sim.run_snr(args.snr, args.frames, 1 << 60, seed=p)
        torch.cuda.synchronize()
        rates.append(args.frames / (time.perf_counter() - t0))
    rates.sort()
    return {"median": round(rates[len(rates) // 2], 1), "min": round(rates[0], 1), "max": round(rates[-1], 1)}, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snr", type=float, default=4.0)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--maxiter", type=int, default=50)
    ap.add_argument("--points", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--torch-only", action="store_true", help="the child of --parent-lib: torch mode alone")
    args = ap.parse_args()
    import numpy as np
    import torch
    import qamr
    from qamr import _lib, codes
    from qamr.sim import Simulator

    _lib.require_gpu()
    vid, cid = codes.dvbs2_like_half()
    dec = qamr.Decoder(vid, cid)
    out = {"lib": _lib.LIB_PATH, "V": dec.vnum, "bps": 2, "snr": args.snr, "B": args.batch, "frames": args.frames,
           "maxiter": args.maxiter}
    if not args.torch_only:
        print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; hip {torch.version.hip}", flush=True)
    sim = Simulator(dec, 2, "softening", args.maxiter, batch=args.batch)
    sim.run_snr(args.snr, args.batch, 1 << 60, seed=99)   # warm-up: code objects, workspaces
    torch.cuda.synchronize()
    out["torch_frames_per_s"], res = rate(sim, args, torch)
    out["torch_result"] = list(res)
    if args.torch_only:
        print(json.dumps(out), flush=True)
        return
    sim = Simulator(dec, 2, "softening", args.maxiter, batch=args.batch, stream="numpy")
    np.random.seed(99)
    sim.run_snr(args.snr, args.batch, 1 << 60)
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    _lib.profile_select(NAMES)
    _lib.profile_reset()
    np.random.seed(0)
    out["numpy_frames_per_s"], res = rate(sim, args, torch)
    out["numpy_result"] = list(res)
    batches = args.points * ((args.frames + args.batch - 1) // args.batch)
    launches = {}
    for name in NAMES:
        ms, n = _lib.profile_query(name)
        launches[name] = {"launches": n, "ms_per_batch": round(ms / batches, 3)}
    _lib.profile_enable(False)
    _lib.profile_select(None)
    out["launches"] = launches
    device_ms = sum(v["ms_per_batch"] for v in launches.values()) / args.batch
    # numpy's own draws of one frame on this host (sims/reconciliation.pyx:129-132)
    S, p = sim.S, np.asarray(sim.pa.probabilities, np.float64)
    np.random.seed(1)
    t0 = time.perf_counter()
    for _ in range(200):
        np.random.choice(p.size, size=S, p=p)
        np.random.randn(S)
    host_ms = (time.perf_counter() - t0) / 200 * 1e3
    out["host_draw_ms_per_frame"] = round(host_ms, 4)
    out["device_draw_ms_per_frame"] = round(device_ms, 5)
    out["ratio_numpy_over_torch"] = round(out["numpy_frames_per_s"]["median"] / out["torch_frames_per_s"]["median"], 4)
    out["ratio_host_over_device_draws"] = round(host_ms / device_ms, 1)
    print(json.dumps(out), flush=True)
    if args.parent_lib:
        argv = [sys.executable, os.path.abspath(__file__), "--torch-only", "--snr", str(args.snr), "--batch",
                str(args.batch), "--frames", str(args.frames), "--maxiter", str(args.maxiter), "--points", str(args.points)]
        del sim, dec
        torch.cuda.empty_cache()
        r = subprocess.run(argv, env=dict(os.environ, QAMR_LIB=os.path.abspath(args.parent_lib)), check=True,
                           capture_output=True, text=True)
        print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
