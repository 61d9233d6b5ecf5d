"""Local mapping's CreateNewMapPoints triangulation on the GPU (lba_triangulate: one thread per row, one workgroup per
64 rows of a pair): milliseconds per call, host packing, upload, launch, download and scatter included, and the share of
it that the kernel takes (two HIP events around the launch, lba_triangulate_profile), for 1, 20 and 200 pairs of 300
rows (4 cameras per rig, the last one stereo, 0.5 px noise, 10 % gross outliers).  Median of 20 timed calls after 5
warm-ups.  A batch is eight generated pairs repeated.

    python scripts/bench_triangulate.py [--pairs 1,20,200] [--rows 300]

A report, not a gate: the capability is new, no earlier implementation exists to compare a time against, and no speed
target is set.  The reference's CPU time for the same loop was not run: Eigen cannot be built where this was measured."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "amc-slam_amd")]
from amc_lba.track import Tracker, track_config  # noqa: E402
from amc_lba.triangulate import make_tri_pairs, tri_params  # noqa: E402

WARMUP, REPS, BASE = 5, 20, 8


def arg(name, default):
    return [int(x) for x in sys.argv[sys.argv.index(name) + 1].split(",")] if name in sys.argv else default


def batch(n, n_rows):
    """n pairs: BASE generated ones (one current keyframe, BASE neighbours) repeated, every copy with rows of its own"""
    k = min(n, BASE)
    pairs, rows, kfs, cams, _ = make_tri_pairs(n_pairs=k, n_rows=n_rows, seed=9)
    rep = np.arange(n) % k
    P = pairs[rep].copy()
    P["row0"] = np.arange(n) * n_rows
    return P, np.concatenate([rows[r * n_rows:(r + 1) * n_rows] for r in rep]), kfs, cams


def timed(call, kernel_ms):
    call_ms, ker_ms, out = [], [], None
    for k in range(WARMUP + REPS):
        t0 = time.perf_counter()
        out = call()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= WARMUP:
            call_ms.append(dt)
            ker_ms.append(kernel_ms())
    return float(np.median(call_ms)), [round(min(call_ms), 3), round(max(call_ms), 3)], float(np.median(ker_ms)), out


NOTE = ("# lba_triangulate, median of 20 calls after 5 warm-ups.  No speed target: nothing earlier to compare with.  "
        "The reference's CPU time for this loop was not run (Eigen cannot be built here).")
print(NOTE, flush=True)
t = Tracker(track_config())
t.triangulate_kernel_ms(on=True)
prm = tri_params(1.2)
n_rows = arg("--rows", [300])[0]
for n in arg("--pairs", [1, 20, 200]):
    P, rows, kfs, cams = batch(n, n_rows)
    med, mm, ker, out = timed(lambda: t.triangulate(P.copy(), rows.copy(), kfs, cams, 4, prm),
                              lambda: t.triangulate_kernel_ms(on=True))
    print(json.dumps({"pairs": n, "rows_per_pair": n_rows, "call_ms": round(med, 3), "call_ms_min_max": mm,
                      "kernel_ms": round(ker, 4), "kernel_share": round(ker / med, 3),
                      "us_per_row": round(1e3 * med / (n * n_rows), 4), "new_points": int(out[0]["n_new"].sum()),
                      "stereo_points": int(out[0]["n_stereo"].sum()),
                      "status_counts": np.bincount(out[1]["status"], minlength=11).tolist(),
                      "warmup": WARMUP, "reps": REPS}), flush=True)
t.close()
