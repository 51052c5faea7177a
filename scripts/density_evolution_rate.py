#!/usr/bin/env python3
"""Cost and verdicts of the sampled density evolution (qamr.density_evolution; DESIGN.md "Density evolution").

Launch times (``--out-rate``): for M in 2^16, 2^20, 2^24 and the degree tables of ``codes.dvbs2_like_half()``
and of the regular (3, 6) ensemble, one evolution of ``--iterations`` iterations on a channel population of
64 softened 4-PAM frames at 4.0 dB and alpha = 0.7, timed per phase by the library's own hipEvent pairs
(qr_profile_*: de_var, de_check, de_post summed over the call's launches).  Beside it a device-to-device copy
of the two populations' bytes by a torch event pair.  Everything is warmed up twice, then the configurations
are timed in turn, ``--rounds`` times over (alternating, so a drift of the clock hits all of them).  One JSON
line per (tables, M): ms per iteration (median, min, max over the rounds), box-plus evaluations per second of
the check phase, and whether repeated evolutions wrote identical bits.

Verdicts (``--out-points``): the points of the FER table of profiles/lappr_info/README.md -- 4-PAM, search
demapper, alpha 0.7 and 1.0, 3.25 / 3.5 / 3.75 / 4.0 dB, the dvbs2_like_half tables, T = 50, M = 2^20, 64
frames, seed 0, exactly what ``python -m qamr.sim_density_evolution`` computes -- one JSON line per
(point, alpha) with errors[t] / M for every t, the first iteration with no error, and the wall time of the
point's evolution.  Markdown tables of both parts go to stdout.

    python scripts/density_evolution_rate.py [--rounds 5] [--iterations 10] [--sizes 16,20,24]
        [--out-rate profiles/density_evolution/density_evolution_rate.jsonl]
        [--out-points profiles/density_evolution/density_evolution_points.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qam-reconciliation_amd"))
OUT = os.path.join(ROOT, "profiles", "density_evolution")
SCOPES = ("de_var", "de_check", "de_post")


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def spread(v):
    return {"median": round(median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def channel_population(snr_db, alpha, frames, seed, symbols=32400):
    """64 softened 4-PAM frames of N = 64 800 bits as a signed population, as the CLI draws them."""
    import qamr
    import torch
    from qamr.density_evolution import signed_population
    from qamr.pipeline import alternating_config
    from qamr.sim import llr_source

    pa = qamr.PAMAlphabet(2, 2)
    two_var = pa.variance * (10 ** (-snr_db / 10))
    nm = qamr.NoiseMapper(pa, two_var / 2, alternating_config(pa.order), device=0)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    lappr, word = llr_source(nm, pa, symbols, frames, gen, "softening", "search", 1.0, two_var)
    return signed_population(lappr, word, frames, alpha)


def rates(args):
    import numpy as np
    import torch
    from qamr import _lib, codes
    from qamr.density_evolution import DETables, degree_tables, evolve_device

    u = channel_population(4.0, 0.7, 64, 0)
    reg = (np.full(6, 3, np.int32), np.full(6, 6, np.int32), np.full(2, 3, np.int32))
    ensembles = {"dvbs2_like_half": degree_tables(*codes.dvbs2_like_half()), "regular_3_6": reg}
    tables = {k: DETables(*v) for k, v in ensembles.items()}
    # box-plus evaluations of one check phase per sample: E[d_c - 2] over the edge perspective
    bp_per_sample = {k: float(np.mean(v[1].astype(np.float64) - 2.0)) for k, v in ensembles.items()}
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    T = args.iterations
    configs = [(k, M) for k in tables for M in sizes]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    buf = {M: (torch.zeros(2 * M, dtype=torch.float64, device="cuda"), torch.empty(2 * M, dtype=torch.float64, device="cuda"))
           for M in sizes}

    def copy_ms(M):
        ev[0].record()
        buf[M][1].copy_(buf[M][0])
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    first = {}
    for w in range(2):   # warm-up: code objects, the clocks
        for k, M in configs:
            r = evolve_device(u, tables[k], M, T, 0)
            copy_ms(M)
            first[(k, M)] = (r.errors.clone(), r.c2v.clone())
    torch.cuda.synchronize()
    t = {c: {s: [] for s in SCOPES + ("iteration", "call")} for c in configs}
    tc = {M: [] for M in sizes}
    same = {c: True for c in configs}
    _lib.profile_enable(True)
    _lib.profile_select(",".join(SCOPES))
    for _ in range(args.rounds):
        for k, M in configs:
            _lib.profile_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = evolve_device(u, tables[k], M, T, 0)
            torch.cuda.synchronize()
            t[(k, M)]["call"].append((time.perf_counter() - t0) * 1e3)
            q = {s: _lib.profile_query(s) for s in SCOPES}
            assert (q["de_var"][1], q["de_check"][1], q["de_post"][1]) == (T, T, T + 1), q
            for s in SCOPES:
                t[(k, M)][s].append(q[s][0] / T)
            t[(k, M)]["iteration"].append(sum(q[s][0] for s in SCOPES) / T)
            same[(k, M)] &= torch.equal(r.errors, first[(k, M)][0]) and \
                torch.equal(r.c2v.view(torch.int64), first[(k, M)][1].view(torch.int64))
        for M in sizes:
            tc[M].append(copy_ms(M))
    _lib.profile_enable(False)
    _lib.profile_select(None)
    lines = []
    for k, M in configs:
        c = t[(k, M)]
        bp = bp_per_sample[k] * M
        lines.append({"tables": k, "M": M, "T": T, "Mu": int(u.numel()), "rounds": args.rounds, "repeatable_bits": bool(same[(k, M)]),
                      "ms_per_iteration": spread(c["iteration"]), "de_var_ms": spread(c["de_var"]),
                      "de_check_ms": spread(c["de_check"]), "de_post_ms": spread(c["de_post"]),
                      "call_ms_host_clock": spread(c["call"]), "box_plus_per_iteration": bp,
                      "box_plus_per_s_check_phase": round(bp / median(c["de_check"]) * 1e3, 1),
                      "box_plus_per_s_iteration": round(bp / median(c["iteration"]) * 1e3, 1),
                      "copy_of_both_populations": dict(bytes=16 * M, ms=spread(tc[M]),
                                                       GB_per_s_read=round(16 * M / median(tc[M]) / 1e6, 1))})
    print("| tables | M | ms per iteration | `de_var` | `de_check` | `de_post` | box-plus/s (check phase) | copy of 16 M bytes |")
    print("|---|---|---|---|---|---|---|---|")
    f = lambda s: "%.4f (%.4f .. %.4f)" % (s["median"], s["min"], s["max"])   # noqa: E731
    for ln in lines:
        print("| %s | 2^%d | %s | %s | %s | %s | %.3g | %s |" % (
            ln["tables"], ln["M"].bit_length() - 1, f(ln["ms_per_iteration"]), f(ln["de_var_ms"]), f(ln["de_check_ms"]),
            f(ln["de_post_ms"]), ln["box_plus_per_s_check_phase"], f(ln["copy_of_both_populations"]["ms"])))
    return lines, all(same.values())


def points(args):
    import numpy as np
    import torch
    import qamr
    from qamr import codes
    from qamr import sim_density_evolution as cli
    from qamr.density_evolution import DETables, degree_tables
    from qamr.sim_lappr_information import point_seed

    a = cli.build_parser().parse_args(["-", "--snr", "3.25", "4.0", "--nsnr", "4", "--alphas", "0.7", "1.0", "--iterations", "50",
                                       "--population", str(1 << 20), "--frames", "64", "--seed", "0"])
    pa = qamr.PAMAlphabet(2, 2)
    vid, cid = codes.dvbs2_like_half()
    tables = DETables(*degree_tables(vid, cid))
    lines = []
    for rep in range(2):   # the first pass warms up; the second is reported
        lines = []
        for i, snr in enumerate(np.linspace(a.snr[0], a.snr[1], a.nsnr)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = cli.point(pa, tables, float(snr), 32400, a, point_seed(a.seed, i))
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            for alpha, r in zip(a.alphas, res):
                rate = r.error_rate()
                below = np.flatnonzero(rate < 1.0 / 64800.0)   # under one bit of an N = 64 800 frame
                lines.append({"EsN0dB": float(snr), "alpha": alpha, "T": a.iterations, "M": a.population, "frames": a.frames,
                              "final": float(rate[-1]), "best": float(rate.min()), "first_zero": r.first_zero(),
                              "first_below_one_bit_per_frame": int(below[0]) if below.size else None,
                              "point_ms_frames_demap_and_both_alphas": round(ms, 2), "error_rate": [float(v) for v in rate]})
    print("\n| Es/N0 | alpha | errors[0]/M | errors[50]/M | smallest errors[t]/M | first zero | first t under 1/64800 |")
    print("|---|---|---|---|---|---|---|")
    dash = lambda v: "—" if v is None else v   # noqa: E731
    for ln in lines:
        print("| %.2f dB | %.1f | %.4f | %.3g | %.3g | %s | %s |" % (
            ln["EsN0dB"], ln["alpha"], ln["error_rate"][0], ln["final"], ln["best"], dash(ln["first_zero"]),
            dash(ln["first_below_one_bit_per_frame"])))
    print("wall time of a point (frames, demap, two evolutions of 151 launches): %s ms" %
          ", ".join("%.1f" % ln["point_ms_frames_demap_and_both_alphas"] for ln in lines[::2]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--sizes", default="16,20,24", help="log2 of the population sizes")
    ap.add_argument("--out-rate", default=os.path.join(OUT, "density_evolution_rate.jsonl"))
    ap.add_argument("--out-points", default=os.path.join(OUT, "density_evolution_points.jsonl"))
    args = ap.parse_args()
    import torch
    from qamr import _lib

    _lib.require_gpu()
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; hip {torch.version.hip}", flush=True)
    lines, ok = rates(args)
    for path, rows in ((args.out_rate, lines), (args.out_points, points(args))):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            for ln in rows:
                fh.write(json.dumps(ln) + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
