"""Rate-adapted softening reconciliation vs SNR: one mother code, punctured and shortened, with
blind rounds (qamr.rate_adapt; this library's, the reference has no rate adaptation).

    PYTHONPATH=qam-reconciliation_amd python -m qamr.sim_rate_adapt code.csv \\
        [--out out.csv] [--bps 2] [--snr 0 5] [--nsnr 11] [--punctured P] [--shortened S] [--adapt-seed 0] \\
        [--blind-rounds 0] [--blind-step 1] [--frames 4096] [--batch 4096] [--maxiter 50] [--alpha 1.0] \\
        [--demapper search|simplified] [--schedule flooding|layered] [--seed 0] [--device 0]

Per SNR point a fixed number of frames (no early stop), on one rank.  Every batch goes through
blind_batch: round 0 decodes with the punctured bits undisclosed; a frame that failed has
``--blind-step`` more of them disclosed and is decoded again, up to ``--blind-rounds`` times.  One CSV
row per point: EsN0dB, fer (frames with a payload bit error after the last attempt), ber (over the
n payload bits), iters (iterations summed over a frame's attempts, averaged over the frames that
ended decoded), fer_round0 (frames whose first decode did not reach the syndrome), revealed_mean
(punctured bits disclosed per frame) and rate_mean = (K - s - revealed_mean) / n.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

COLUMNS = ("EsN0dB", "fer", "ber", "iters", "fer_round0", "revealed_mean", "rate_mean")


def build_parser():
    p = argparse.ArgumentParser(prog="sim_rate_adapt", description="Rate-adapted reconciliation vs SNR")
    p.add_argument("edgefile", help="CSV with a 'vid' and a 'cid' columns representing an edge per line")
    p.add_argument("--out", default="out.csv")
    p.add_argument("--bps", type=int, default=2)
    p.add_argument("--snr", type=float, nargs=2, default=[0, 5], metavar=("LO", "HI"))
    p.add_argument("--nsnr", type=int, default=11)
    p.add_argument("--punctured", type=int, default=0)
    p.add_argument("--shortened", type=int, default=0)
    p.add_argument("--adapt-seed", type=int, default=0)
    p.add_argument("--blind-rounds", type=int, default=0, help="further decodes of a frame that failed")
    p.add_argument("--blind-step", type=int, default=1, help="punctured bits disclosed per blind round")
    p.add_argument("--frames", type=int, default=4096, help="frames per SNR point")
    p.add_argument("--batch", type=int, default=4096, help="frames per batch")
    p.add_argument("--maxiter", type=int, default=50)
    p.add_argument("--alpha", type=float, default=1.0)
    p.add_argument("--demapper", choices=("search", "simplified"), default="search")
    p.add_argument("--schedule", choices=("flooding", "layered"), default="flooding")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=int, default=0)
    return p


def point_seed(seed: int, index: int, batch: int) -> int:
    """The generator seed of batch `batch` of SNR point `index`."""
    return (int(seed) * 1000003 + int(index)) * 4099 + int(batch)


def run_point(sim, snr_dB: float, frames: int, rounds: int, step: int, seed: int, index: int):
    """One SNR point of `frames` frames in batches of sim.batch: the CSV row."""
    import torch

    from .noisemapper import NoiseMapper
    from .rate_adapt import blind_batch

    two_var = sim.pa.variance * (10 ** (-snr_dB / 10))
    nm = NoiseMapper(sim.pa, two_var / 2, sim.cfg, device=sim.device.index)
    adapt = sim.adapt
    counters = torch.zeros(5, dtype=torch.int64, device=sim.device)
    fail0 = torch.zeros((), dtype=torch.int64, device=sim.device)
    revealed = torch.zeros((), dtype=torch.int64, device=sim.device)
    done, b = 0, 0
    while done < frames:
        B = min(sim.batch, frames - done)
        gen = torch.Generator(device=sim.device).manual_seed(point_seed(seed, index, b))
        r = blind_batch(sim, nm, B, gen, two_var, rounds, step)
        ferr = torch.empty(B, dtype=torch.int32, device=sim.device)
        its = torch.clamp(r["iterations_total"], max=2 ** 31 - 1).to(torch.int32)
        adapt.count_errors_device(B, r["final"].shape[1], r["final"], r["word"], r["success"], its, ferr, counters)
        fail0 += (r["success_round0"] == 0).sum()
        revealed += r["revealed"].to(torch.int64).sum()
        done += B
        b += 1
    be, fe, su, it, fr = [int(v) for v in counters.cpu().numpy()]
    rev_mean = int(revealed) / fr
    return (snr_dB, fe / fr, be / (fr * adapt.n), 0 if su == 0 else it / su, int(fail0) / fr, rev_mean,
            adapt.rate(sim.K, rev_mean))


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.nsnr < 1 or args.frames < 1 or args.batch < 1 or args.blind_rounds < 0 or args.blind_step < 1:
        raise SystemExit("--nsnr, --frames, --batch, --blind-step must be positive and --blind-rounds >= 0")

    from ._lib import require_gpu
    from .codes import load_edge_csv
    from .decoder import Decoder
    from .rate_adapt import RateAdaption
    from .sim import Simulator
    from .sim_reconciliation import adaption_from_args

    require_gpu()
    vid, cid = load_edge_csv(args.edgefile)
    adapt = adaption_from_args(vid, cid, args.punctured, args.shortened, args.adapt_seed)
    if adapt is None:   # nothing adapted: every variable is payload
        adapt = RateAdaption(int(np.max(vid)) + 1, [], [])
    dec = Decoder(vid, cid, device=args.device)
    sim = Simulator(dec, args.bps, "softening", args.maxiter, args.alpha, args.batch, device=args.device,
                    demapper=args.demapper, schedule=args.schedule, adapt=adapt)
    rows = []
    for i, snr in enumerate(np.linspace(args.snr[0], args.snr[1], args.nsnr)):
        rows.append(run_point(sim, float(snr), args.frames, args.blind_rounds, args.blind_step, args.seed, i))
        print("EsN0dB=%.3f fer=%.6g ber=%.6g iters=%.3f fer_round0=%.6g revealed_mean=%.6g rate_mean=%.6g" % rows[-1],
              flush=True)
    with open(args.out, "w") as fh:
        fh.write(",".join(COLUMNS) + "\n")
        for r in rows:
            fh.write(",".join(repr(float(v)) for v in r) + "\n")
    return rows


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
