#!/usr/bin/env python3
"""Latency of the decode of a few frames on the N = 64 800 code, and the A/B that sets the default
of knob ``few_max``.

The frames are 4-PAM 3.0 dB (SofteningPipeline.generate + demap), so every frame runs all 50
iterations.  Per B in 1, 2, 4, 8, 16, 32, 64, after a warm-up of each shape, the median of
``--calls`` calls (default 25) of

  decode_batch          Decoder.decode_batch, host arrays in and out, synchronous: the drop-in's own
                        shape (Decoder.decode is this call at B = 1);
  frames_device         Decoder.decode_frames_device on device tensors, timed with device events
                        (libraries that have it).

One library (whatever qamr loads: QAMR_LIB or the in-tree build), one JSON line per B:

    python scripts/few_frame_rate.py [--few-max 64] [--calls 25] [--oracle]

``--oracle`` also times one frame in the oracle (oracle/qamr_oracle.c, one CPU core).

The A/B against another build of the library (the commit before the few-frame schedule, built into
a scratch directory), each run a fresh child process, alternating, the other library twice so that
the spread between its own repeats is known:

    python scripts/few_frame_rate.py --ab path/to/libqamr_parent.so [--out few_rate.jsonl]

runs parent, new (few_max = 64: every listed B on the few-frame schedule), new with few_max = 0,
parent, new; prints the table and the default the rule gives: the largest listed B up to which, at
every listed B, the new library's decode_batch median beats the parent's by more than twice the
spread of the parent's two runs and by no less than 5 %; 0 if that fails at B = 1.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qam-reconciliation_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

BS = (1, 2, 4, 8, 16, 32, 64)
MI = 50


def measure(args):
    import numpy as np
    import torch
    import qamr
    from qamr import _lib, codes
    from qamr.pipeline import SofteningPipeline

    _lib.require_gpu()
    L = _lib.load()
    has_few = hasattr(L, "qr_decode_frames_device")
    few_max = None
    if has_few:
        _lib.tune_set("few_max", args.few_max)
        few_max = _lib.tune_get("few_max")
    vid, cid = codes.dvbs2_like_half()
    dec = qamr.Decoder(vid, cid)
    pipe = SofteningPipeline(dec, bps=2, snr_db=3.0, batch=64, max_iterations=MI)
    b = pipe.generate(torch.Generator(device="cuda").manual_seed(30))
    lappr = pipe.demap(b)
    torch.cuda.synchronize()
    Lh = lappr[:, :64].T.contiguous().cpu().numpy()
    Sh = b.synd[:, :64].T.contiguous().cpu().numpy()
    head = {"label": args.label, "device": torch.cuda.get_device_name(0), "lib": os.path.basename(_lib.LIB_PATH),
            "few_max": few_max, "calls": args.calls}
    for B in BS:
        l, s = np.ascontiguousarray(Lh[:B]), np.ascontiguousarray(Sh[:B])
        for _ in range(3):
            succ, its, _ = dec.decode_batch(l, s, MI)
        assert (its == MI).all(), "every frame must run all 50 iterations"
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            dec.decode_batch(l, s, MI)
            ms.append((time.perf_counter() - t0) * 1e3)
        row = dict(head, B=B, decode_batch_ms=round(statistics.median(ms), 4), decode_batch_min_ms=round(min(ms), 4))
        if has_few:
            ld, sd = torch.from_numpy(l).cuda(), torch.from_numpy(s).cuda()
            out = dec.decode_frames_device(ld, sd, MI)
            for _ in range(2):
                dec.decode_frames_device(ld, sd, MI, *out)
            torch.cuda.synchronize()
            ev = []
            for _ in range(args.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dec.decode_frames_device(ld, sd, MI, *out)
                e1.record()
                e1.synchronize()
                ev.append(e0.elapsed_time(e1))
            assert bool((out[2] == MI).all())
            row["frames_device_ms"] = round(statistics.median(ev), 4)
        print(json.dumps(row), flush=True)
    if args.oracle:
        import oracle as O

        orc = O.OracleCode(vid, cid)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            s1, i1, _ = orc.decode(Lh[0], Sh[0], MI)
            ts.append((time.perf_counter() - t0) * 1e3)
        assert i1 == MI
        print(json.dumps(dict(head, B=1, oracle_decode_ms=round(statistics.median(ts), 3))), flush=True)


def child(label, lib, few_max, calls, oracle=False):
    env = dict(os.environ)
    env.pop("QAMR_LIB", None)
    if lib:
        env["QAMR_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--label", label, "--few-max", str(few_max), "--calls", str(calls)]
    if oracle:
        cmd.append("--oracle")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    if r.returncode != 0:
        sys.exit(f"{label}: exit {r.returncode}\n{(r.stdout + r.stderr)[-2000:]}")
    rows = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    for x in rows:
        print(json.dumps(x), flush=True)
    return rows


def ab(args):
    runs = [("parent_1", args.ab, 0), ("new_1", None, 64), ("new_off", None, 0), ("parent_2", args.ab, 0),
            ("new_2", None, 64)]
    rows = []
    for label, lib, fm in runs:
        rows += child(label, lib, fm, args.calls, oracle=label == "new_1")
    get = lambda label, B, key="decode_batch_ms": next(  # noqa: E731
        r[key] for r in rows if r["label"] == label and r["B"] == B and key in r)
    table, default, open_ = [], 0, True
    for B in BS:
        p1, p2 = get("parent_1", B), get("parent_2", B)
        n1, n2 = get("new_1", B), get("new_2", B)
        parent, new, spread = (p1 + p2) / 2, (n1 + n2) / 2, abs(p1 - p2)
        gain = (parent - new) / parent
        win = parent - new > 2 * spread and gain >= 0.05
        open_ = open_ and win
        if open_:
            default = B
        table.append(dict(B=B, parent_1=p1, parent_2=p2, spread=round(spread, 4), new_1=n1, new_2=n2,
                          new_off=get("new_off", B), gain=round(gain, 4), win=win,
                          frames_device_ms=get("new_1", B, "frames_device_ms")))
    summary = {"label": "summary", "table": table, "few_max_default": default,
               "oracle_decode_ms": next(r["oracle_decode_ms"] for r in rows if "oracle_decode_ms" in r),
               "decode_ms_new": get("new_1", 1), "decode_ms_parent": get("parent_1", 1)}
    print(json.dumps(summary), flush=True)
    print("| B | parent 1 | parent 2 | spread | new 1 | new 2 | few_max=0 | gain | wins | frames_device |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for t in table:
        print(f"| {t['B']} | {t['parent_1']:.3f} | {t['parent_2']:.3f} | {t['spread']:.3f} | {t['new_1']:.3f} | "
              f"{t['new_2']:.3f} | {t['new_off']:.3f} | {100 * t['gain']:.1f} % | {'yes' if t['win'] else 'no'} | "
              f"{t['frames_device_ms']:.3f} |")
    print(f"few_max default by the rule: {default}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows + [summary]:
                f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", help="the other library (A/B driver mode)")
    ap.add_argument("--out", help="A/B mode: write every JSON line here")
    ap.add_argument("--label", default="run")
    ap.add_argument("--few-max", type=int, default=64)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    if args.calls < 20:
        sys.exit("--calls: at least 20")
    if args.ab:
        ab(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
