"""Loop closing's OptimizeSim3 on the GPU (lba_sim3_optimize, one workgroup of one wave per candidate pair):
milliseconds per call, host set-up, upload, the launch and download included, and the share of it that k_sim3 itself
takes (two HIP events around the launch, lba_sim3_profile), for 1, 16 and 64 pairs of 100 and of 300 correspondences
(4 cameras per rig, 0.7 px noise, 10 % gross outliers).  Median of 20 timed calls after 5 warm-ups.

    python scripts/bench_sim3.py [--pairs 1,16,64] [--rows 100,300]

A report, not a gate: the capability is new, and the reference's CPU time for the same call was never measured."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "amc-slam_amd")]
from amc_lba.sim3 import make_sim3_pairs  # noqa: E402
from amc_lba.track import Tracker, track_config  # noqa: E402

WARMUP, REPS = 5, 20


def arg(name, default):
    return [int(x) for x in sys.argv[sys.argv.index(name) + 1].split(",")] if name in sys.argv else default


t = Tracker(track_config())
t.sim3_kernel_ms(on=True)
for rows in arg("--rows", [100, 300]):
    for n in arg("--pairs", [1, 16, 64]):
        pairs, corr, cams, _ = make_sim3_pairs(n_pairs=n, n_corr=rows, n_cam=4, seed=9)
        call_ms, kernel_ms = [], []
        for k in range(WARMUP + REPS):
            p, c = pairs.copy(), corr.copy()
            t0 = time.perf_counter()
            out = t.sim3_optimize(p, c, cams, 4)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= WARMUP:
                call_ms.append(dt)
                kernel_ms.append(t.sim3_kernel_ms(on=True))
        med, ker = float(np.median(call_ms)), float(np.median(kernel_ms))
        print(json.dumps({"pairs": n, "rows_per_pair": rows, "call_ms": round(med, 3),
                          "call_ms_min_max": [round(min(call_ms), 3), round(max(call_ms), 3)],
                          "kernel_ms": round(ker, 3), "kernel_share": round(ker / med, 3),
                          "mean_lm_iterations": float(out[0]["iterations"].mean()), "mean_n_in": float(out[0]["n_in"].mean()),
                          "mean_n_bad": float(out[0]["n_bad"].mean()), "warmup": WARMUP, "reps": REPS}), flush=True)
t.close()
