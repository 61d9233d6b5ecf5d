"""Loop closing's Sim3Solver RANSAC on the GPU (lba_sim3_ransac: one wave per hypothesis, then one per pair):
milliseconds per call, host set-up, upload, both launches and download included, and the share of it that the two
kernels take (two HIP events around them, lba_sim3_ransac_profile), for 1, 16 and 64 pairs of 100 and of 300
correspondences with 300 hypotheses each (4 cameras per rig, 4 mm noise, 30 % gross outliers), next to
lba_sim3_optimize's figures for the same candidates.  Median of 20 timed calls after 5 warm-ups.  A batch is eight
generated candidates repeated, every copy with triples of its own.

    python scripts/bench_sim3_ransac.py [--pairs 1,16,64] [--rows 100,300] [--hyp 300]

A report, not a gate: the capability is new, no earlier implementation exists to compare a time against, and the
reference's CPU time for the same loop cannot be measured where Eigen is absent."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "amc-slam_amd")]
from amc_lba.sim3_ransac import draw_triples, make_sim3_ransac_pairs  # noqa: E402
from amc_lba.track import Tracker, track_config  # noqa: E402

WARMUP, REPS, BASE = 5, 20, 8


def arg(name, default):
    return [int(x) for x in sys.argv[sys.argv.index(name) + 1].split(",")] if name in sys.argv else default


def batch(n, rows, n_hyp):
    """n candidates: BASE generated ones repeated; RANSAC and OptimizeSim3 inputs of the same candidates"""
    k = min(n, BASE)
    pairs, corr, _, cams, truth = make_sim3_ransac_pairs(n_pairs=k, n_corr=rows, n_hyp=0, seed=9)
    rep = np.arange(n) % k
    rng = np.random.default_rng(9)

    def rows_of(a):
        return np.concatenate([a[r * rows:(r + 1) * rows] for r in rep])
    P, S = pairs[rep].copy(), truth["sim3_pairs"][rep].copy()
    P["corr0"] = S["corr0"] = np.arange(n) * rows
    P["cam0"] = S["cam0"] = np.arange(n) * 8
    P["hyp0"], P["n_hyp"] = np.arange(n) * n_hyp, n_hyp
    samples = np.concatenate([draw_triples(rows, n_hyp, rng) for _ in range(n)])
    return P, rows_of(corr), samples, np.concatenate([cams[r * 8:(r + 1) * 8] for r in rep]), S, rows_of(truth["sim3_corr"])


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


t = Tracker(track_config())
t.sim3_ransac_kernel_ms(on=True)
t.sim3_kernel_ms(on=True)
n_hyp = arg("--hyp", [300])[0]
for rows in arg("--rows", [100, 300]):
    for n in arg("--pairs", [1, 16, 64]):
        P, corr, samples, cams, S, scorr = batch(n, rows, n_hyp)
        med, mm, ker, out = timed(lambda: t.sim3_ransac(P.copy(), corr.copy(), samples, cams, 4, per_hyp=False),
                                  lambda: t.sim3_ransac_kernel_ms(on=True))
        o_med, _, o_ker, _ = timed(lambda: t.sim3_optimize(S.copy(), scorr.copy(), cams, 4), lambda: t.sim3_kernel_ms(on=True))
        print(json.dumps({"pairs": n, "rows_per_pair": rows, "hypotheses_per_pair": n_hyp, "call_ms": round(med, 3),
                          "call_ms_min_max": mm, "kernel_ms": round(ker, 3), "kernel_share": round(ker / med, 3),
                          "converged": int(out[0]["converged"].sum()), "mean_best_hyp": float(out[0]["best_hyp"].mean()),
                          "mean_n_inliers": float(out[0]["n_inliers"].mean()),
                          "sim3_optimize_call_ms": round(o_med, 3), "sim3_optimize_kernel_ms": round(o_ker, 3),
                          "warmup": WARMUP, "reps": REPS}), flush=True)
t.close()
