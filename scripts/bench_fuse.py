"""ORBmatcher::Fuse's search on the GPU (lba_match_fuse) at the call sites' shapes: 1, 10 and 20 targets of 4 x 1500
features against 1500 shared points in mode KF (SearchInNeighbors' phase one), one target against 20 000 points (its
phase two with a long list), and 30 targets against 3000 points in mode SIM3 (SearchAndFuse).  Median of 20 timed calls
after 5 warm-ups, with the spread: the whole call and the kernel between events (lba_match_fuse_profile), so the host
part (checks, packing, the copies, the scatter) is the difference.  Alongside, with equality of every row asserted, the
same header's sequential fuse_search on ONE CPU thread (tests/native/fuse_harness.cpp, g++ -O2), median of 3: the only
baseline there is, the reference itself cannot be built here.

    python scripts/bench_fuse.py [--out profiles/fuse_bench.txt]

A report, not a gate: the capability is new and no speed target is set."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, d) for d in ("amc-slam_amd", "tests", "oracle")]
import test_fuse_host as th  # noqa: E402
from amc_lba.abi import FUSE_ROW_DTYPE, ptr  # noqa: E402
from amc_lba.fuse import (FUSE_KF, FUSE_OK, FUSE_SIM3, TH_KF, TH_LOW, TH_SIM3, fuse_raw, make_fuse_problem,  # noqa: E402
                          pack_searches, pack_targets)
from amc_lba.track import Tracker, track_config  # noqa: E402

WARMUP, REPS = 5, 20


def median_ms(call, reps=REPS, warmup=WARMUP):
    ms = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), [round(min(ms), 3), round(max(ms), 3)]


def main():
    lines = ["# lba_match_fuse, median of 20 calls after 5 warm-ups, [min, max] beside it; targets of 4 x 1500 features.  "
             "host_loop: one thread of fuse_search (g++ -O2), median of 3.  No speed target."]
    print(lines[0], flush=True)
    prob = make_fuse_problem(n_kf=31, n_cam=4, n_feat=1500, n_points=20000, seed=21)
    t = Tracker(track_config())
    H = th.load_harness()
    t.fuse_kernel_ms(True)
    all_points = prob.points(np.arange(20000))
    shapes = [("neighbours_1", list(range(1, 2)), 1500, FUSE_KF, TH_KF), ("neighbours_10", list(range(1, 11)), 1500, FUSE_KF, TH_KF),
              ("neighbours_20", list(range(1, 21)), 1500, FUSE_KF, TH_KF), ("long_list", [0], 20000, FUSE_KF, TH_KF),
              ("search_and_fuse_30", list(range(1, 31)), 3000, FUSE_SIM3, TH_SIM3)]
    for name, kfs, n_points, mode, thv in shapes:
        targets = [prob.targets[k] for k in kfs]
        pk = pack_targets(targets)
        points = all_points[:n_points]
        S = pack_searches(pk.T, [(i, 0, n_points, mode, thv) for i in range(len(kfs))])
        rows = np.zeros(n_points * 4 * len(kfs), FUSE_ROW_DTYPE)
        ker = []

        def gpu():
            assert fuse_raw(t, pk, S, points, rows, TH_LOW) == 0
            ker.append(t.fuse_kernel_ms(True))

        med, mm = median_ms(gpu)
        k_ms = float(np.median(ker[WARMUP:]))
        h_rows = np.zeros_like(rows)
        h_ok = np.zeros(len(kfs), np.int64)

        def host():
            for i in range(len(kfs)):
                h_ok[i] = H.fh_search(ptr(pk.T[i:i + 1]), ptr(pk.fcams), ptr(pk.gcams), ptr(pk.sf), ptr(pk.sigma),
                                      ptr(pk.cell_start), ptr(pk.cell_feat), ptr(pk.feats), ptr(S[i:i + 1]), ptr(points),
                                      TH_LOW, ptr(h_rows[int(S[i]["row0"]):]))

        hmed, hmm = median_ms(host, reps=3, warmup=1)
        assert h_rows.tobytes() == rows.tobytes() and (h_ok == S["n_ok"]).all(), "the device and the host loop differ"
        live = np.isin(rows["status"], (0, 1, 2))
        lines.append(json.dumps({
            "shape": name, "targets": len(kfs), "points": n_points, "mode": "KF" if mode == FUSE_KF else "SIM3",
            "jobs": int(len(rows)), "live_share": round(float(live.mean()), 4),
            "candidates_mean_max": [round(float(rows["n_cand"][live].mean()), 2), int(rows["n_cand"].max())],
            "accepted": int((rows["status"] == FUSE_OK).sum()), "call_ms": round(med, 3), "call_ms_min_max": mm,
            "k_fuse_ms": round(k_ms, 4), "kernel_share": round(k_ms / med, 3), "host_part_ms": round(med - k_ms, 3),
            "host_loop_one_thread_ms": round(hmed, 3), "host_loop_min_max": hmm, "warmup": WARMUP, "reps": REPS}))
        print(lines[-1], flush=True)
    t.close()
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fuse_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
