"""Loop closing's OptimizeEssentialGraph on the GPU (lba_posegraph_optimize): milliseconds per call for the essential
graphs of synthetic laps of 200, 1000 and 4000 keyframes, each with its loop (amc_lba.posegraph.make_pose_graph,
fix_scale = 1, optimize(20) at the reference's lambda 1e-16), split by lba_posegraph_profile into host planning
(activity, lba_plan::make_plan, the gather lists and the factorisation's lists), upload, and device (first launch to
last readback, the host's accept / reject round trips included); the plan's panels, tiles, levels, chain and launches
per solve from the stats; the LM's iterations and trials.  Median of 5 timed calls after 2 warm-ups.

For context, on the same graph, one solve of the restatement's system (tests/posegraph_oracle.py) through scipy's
sparse LU, on this host's CPU: what a CPU sparse direct solve of one trial costs, not the reference's time for the call
(g2o with LinearSolverEigen was never built or timed here).

    python scripts/bench_posegraph.py [--sizes 200,1000,4000]

A report, not a gate: the capability is new and there is nothing to compare it with."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "amc-slam_amd"), os.path.join(ROOT, "tests")]
import posegraph_oracle as po  # noqa: E402
from amc_lba.posegraph import essential_graph, make_pose_graph  # noqa: E402
from amc_lba.track import Tracker, track_config  # noqa: E402

WARMUP, REPS = 2, 5
sizes = [int(x) for x in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [200, 1000, 4000]

t = Tracker(track_config())
for n in sizes:
    v, e, _ = essential_graph(make_pose_graph(n_kf=n, seed=5, radius=max(20.0, n / 8.0)))
    call_ms, parts = [], []
    for k in range(WARMUP + REPS):
        vv = v.copy()
        t0 = time.perf_counter()
        out, st = t.posegraph_optimize(vv, e, True, 20, 1e-16)
        dt = (time.perf_counter() - t0) * 1e3
        if k >= WARMUP:
            call_ms.append(dt)
            parts.append(t.posegraph_ms())
    plan, upload, device = (float(np.median([p[i] for p in parts])) for i in range(3))
    G = po.Graph(v, e, True)
    H, b, _ = G.build_system(G.states(), sparse=True)
    keep = np.ones(len(b), bool)
    keep[6::7] = False                      # (the sigma rows are 0 + lambda: singular for a general LU)
    Hk = H.tocsr()[keep][:, keep]
    t0 = time.perf_counter()
    po.solve_sparse(Hk, 1e-16, b[keep])
    scipy_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"vertices": len(v), "edges": len(e), "call_ms": round(float(np.median(call_ms)), 3),
                      "call_ms_min_max": [round(min(call_ms), 3), round(max(call_ms), 3)],
                      "host_plan_ms": round(plan, 3), "upload_ms": round(upload, 3), "device_ms": round(device, 3),
                      "iterations": st["iterations"], "trials": st["trials"], "solve_failures": st["solve_failures"],
                      "chi2": [st["chi2_initial"], st["chi2_final"]],
                      "device_ms_per_trial": round(device / max(1, st["trials"]), 3),
                      "panels": st["panels"], "tiles": st["tiles"], "fill_tiles": st["fill_tiles"], "levels": st["levels"],
                      "chain": st["chain"], "launches_per_solve": st["launches_per_solve"],
                      "scipy_sparse_solve_ms": round(scipy_ms, 3), "warmup": WARMUP, "reps": REPS}), flush=True)
t.close()
