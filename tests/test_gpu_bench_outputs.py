"""bench.py --dump-outputs on the hardware: a plain run (fresh child process) writes what its last
timed step returned, and the same arguments give the same arrays again (here: the same workload
rebuilt and stepped once in this process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.gpu
# failing and converging frames of the small code (48 of 200 frames sampled; 200 is no multiple of a
# tile), and the fused demap + decode of the large one at a batch that is sampled as a whole
@pytest.mark.parametrize("workload,snr,B", [("reg1008_4pam", 3.0, 200), ("reg1008_4pam", 6.0, 200),
                                            ("dvbs2_16pam", 14.5, 40)])
def test_dump_outputs_of_plain_run(gpu, tmp_path, workload, snr, B):
    steps = 3
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMR_BENCH_") and k != "WORLD_SIZE"}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", workload, "--snr", str(snr),
           "--batch", str(B), "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == steps and out["ms_per_step"] > 0 and out["full"] is False
    assert abs(out["value"] - B * 1e3 / out["ms_per_step"]) / out["value"] < 1e-2
    # a plain run carries none of the --full measurements
    assert out["roofline"] is None and out["cpu_baseline"] is None and out["kernels"] == {} and "secondary" not in out

    got = {p.name[:-4]: np.load(p) for p in tmp_path.iterdir()}
    fused = workload == "dvbs2_16pam"
    assert sorted(got) == sorted(["final_lappr", "final_lappr_frames", "iterations", "success"]
                                 + (["demap_lappr"] if fused else []))
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 1000 * 1000
    V = out["config"]["V"]
    assert got["final_lappr"].shape == (min(B, 48), V) and got["final_lappr"].dtype == np.float64
    assert got["success"].shape == got["iterations"].shape == (B,)
    assert abs(float(got["iterations"].mean()) - out["mean_iterations"]) < 1e-4
    fr = got["final_lappr_frames"].astype(np.int64)
    assert np.all(np.diff(fr) > 0) and fr[0] >= 0 and fr[-1] < B

    sys.path.insert(0, ROOT)
    import bench

    w = bench.Work(workload, snr, B, 50, 1.0, 0, 0, 0)
    w.step()
    w.sync()
    again = w.outputs()
    assert sorted(again) == sorted(got)
    for k in got:
        assert np.array_equal(got[k].view(np.int64 if got[k].dtype == np.float64 else np.int32),
                              again[k].view(np.int64 if again[k].dtype == np.float64 else np.int32)), k
    # the dumped rows are the decoder's final LAPPRs of the sampled frames
    ref = w.final[:, :B].cpu().numpy().T[fr]
    assert np.array_equal(np.ascontiguousarray(ref).view(np.int64), got["final_lappr"].view(np.int64))
