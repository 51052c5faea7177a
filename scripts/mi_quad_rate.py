#!/usr/bin/env python3
"""Wall time of the quad-integrated mutual-information evaluators' batches (qr_mi_quad_batch) on the sweeps
of the two CLIs built on them:

  compare_signs   the default sweep of qamr.sim_mutual_information_compare_signs (--snr 0 5 --nsnr 11):
                  (SNR points) x (sign configurations) base-scheme integrals in one batch, bps 2 (110
                  integrals) and bps 3 (1496)
  base_scheme     a 401-point sweep of qamr.sim_mutual_information_base_scheme (--snr 0 5): 401 base-scheme
                  integrals in one batch and 401 I(X;Y) integrals in another, bps 2 and bps 4

The NoiseMappers (tables, grid) are built before the clock starts; their construction time is printed
apart.  Every batch is warmed up once, then the batches are timed in turn, `--rounds` times over
(alternating, so a drift of the clock or the host hits all of them).  Printed per batch, one JSON line:
integrals, median / min / max wall ms of the call, rounds (= launches: one per round), work items
(interval evaluations: one wavefront each), the share of the wall time the host spends in the
integrator's bookkeeping, the warnings (ier != 0) and whether repeated calls return the same bits.

    python scripts/mi_quad_rate.py [--rounds 5] [--nsnr 401] [--only compare_signs,base_scheme]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qam-reconciliation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nsnr", type=int, default=401, help="points of the base_scheme sweep")
    ap.add_argument("--only", default="compare_signs,base_scheme")
    args = ap.parse_args()
    import numpy as np
    import torch
    import qamr
    from qamr import _lib
    from qamr.mutual_information import P_xhat, mutual_information_quad_batch, quad_batch_stats
    from qamr.sim_mutual_information_compare_signs import config_list

    _lib.require_gpu()
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; hip {torch.version.hip}", flush=True)

    def mappers(bps, EsN0dB, cfg=None):
        pa = qamr.PAMAlphabet(bps, 2)
        t0 = time.perf_counter()
        nms = [qamr.NoiseMapper(pa, pa.variance * (10 ** (-float(e) / 10)) / 2, cfg) for e in EsN0dB]
        for nm in nms:
            nm._device_grid()
        return nms, [P_xhat(nm) for nm in nms], time.perf_counter() - t0

    batches = []
    only = args.only.split(",")
    if "compare_signs" in only:
        for bps in (2, 3):
            cfgs = config_list(bps)
            snr = np.linspace(0, 5, 11)
            nms, pXs, setup = mappers(bps, snr, cfgs[0])
            nc = len(cfgs)
            batches.append({"sweep": "compare_signs", "bps": bps, "kind": "base", "setup_s": setup,
                            "nms": [nm for nm in nms for _ in range(nc)], "pXs": [p for p in pXs for _ in range(nc)],
                            "cfg": np.tile(cfgs, (len(snr), 1))})
    if "base_scheme" in only:
        for bps in (2, 4):
            nms, pXs, setup = mappers(bps, np.linspace(0, 5, args.nsnr))
            batches.append({"sweep": "base_scheme", "bps": bps, "kind": "base", "setup_s": setup, "nms": nms, "pXs": pXs,
                            "cfg": None})
            batches.append({"sweep": "base_scheme", "bps": bps, "kind": "X_Y", "setup_s": setup, "nms": nms, "pXs": None,
                            "cfg": None})

    def call(b):
        t0 = time.perf_counter()
        out = mutual_information_quad_batch(b["kind"], b["nms"], b["pXs"], b["cfg"])
        return out, time.perf_counter() - t0, quad_batch_stats()

    for b in batches:   # warm-up: code objects, clocks
        b["first"], _, b["stats"] = call(b)
        b["ms"], b["host"], b["same"] = [], [], True
    for _ in range(args.rounds):
        for b in batches:
            out, dt, st = call(b)
            b["ms"].append(dt * 1e3)
            b["host"].append(st["host_s"] / st["total_s"])
            b["same"] &= all(np.array_equal(np.asarray(u).view(np.int32 if u.dtype == np.int32 else np.int64),
                                            np.asarray(v).view(np.int32 if v.dtype == np.int32 else np.int64))
                             for u, v in zip(out, b["first"]))
    ok = True
    for b in batches:
        ms, host = sorted(b["ms"]), sorted(b["host"])
        I, _, neval, ier = b["first"]
        ok &= b["same"]
        print(json.dumps({
            "sweep": b["sweep"], "bps": b["bps"], "kind": b["kind"], "integrals": len(b["nms"]), "rounds_timed": args.rounds,
            "ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
            "rounds": b["stats"]["rounds"], "launches": b["stats"]["launches"], "work_items": b["stats"]["work_items"],
            "evaluations": int(np.asarray(neval, np.int64).sum()), "host_share_median": round(host[len(host) // 2], 4),
            "warned": int(np.count_nonzero(ier)), "minus_inf": int(np.isneginf(I).sum()), "repeatable_bits": bool(b["same"]),
            "mapper_setup_s": round(b["setup_s"], 2)}), flush=True)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
