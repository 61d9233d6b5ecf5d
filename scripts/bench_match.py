"""ORBmatcher's projection searches on the GPU (lba_match_project: one wave per job, then one workgroup per
(search, camera)): milliseconds per call, host checks and packing, upload, two launches, download, scatter and
rotation pass included, and the two kernels' shares (HIP events around the launches, lba_match_profile), for 1, 16 and
64 searches of 4 cameras x 1500 features x 3000 points, in both modes.  Median of 20 timed calls after 5 warm-ups.  A
batch is eight generated frames repeated.  Also the distribution of `rounds` over the (search, camera) pairs.

    python scripts/bench_match.py [--searches 1,16,64] [--feat 1500] [--points 3000]

For context only, next to it: the time of the host-built SEQUENTIAL loop (lba_match_math.hpp: match_search_host through
tests/native/match_harness.cpp, g++ -O2) on ONE CPU thread for the same inputs.  That is this project's restatement,
not the reference's binary, which cannot be built where this was measured.  A report, not a gate: no target is set."""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "amc-slam_amd")]
from amc_lba.abi import ptr  # noqa: E402
from amc_lba.match import (MATCH_BEST, MATCH_RATIO, LbaMatchParams, make_match_search, match_kernel_ms,  # noqa: E402
                           match_params, match_project, pack_searches)
from amc_lba.track import Tracker, track_config  # noqa: E402

WARMUP, REPS, BASE = 5, 20, 8


def arg(name, default):
    return [int(x) for x in sys.argv[sys.argv.index(name) + 1].split(",")] if name in sys.argv else default


def harness():
    src = os.path.join(ROOT, "tests", "native", "match_harness.cpp")
    out = os.path.join(ROOT, "tests", "native", "_build", "libmatch_harness.so")
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", out])
    L = ctypes.CDLL(out)
    L.mh_search.argtypes = [ctypes.c_void_p] * 6 + [ctypes.POINTER(LbaMatchParams)]
    L.mh_search.restype = None
    return L


def median_ms(call, after=None):
    ms, extra, out = [], [], None
    for k in range(WARMUP + REPS):
        t0 = time.perf_counter()
        out = call()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= WARMUP:
            ms.append(dt)
            if after:
                extra.append(after())
    return float(np.median(ms)), [round(min(ms), 3), round(max(ms), 3)], extra, out


print("# lba_match_project, median of 20 calls after 5 warm-ups.  No speed target.  cpu_sequential_ms: this project's "
      "host-built sequential loop on one CPU thread (not the reference's binary).", flush=True)
H = harness()
t = Tracker(track_config())
match_kernel_ms(t, on=True)
n_feat, n_points = arg("--feat", [1500])[0], arg("--points", [3000])[0]
for mode, name in ((MATCH_RATIO, "ratio"), (MATCH_BEST, "best")):
    base = [make_match_search(mode=mode, n_cam=4, n_feat=n_feat, n_points=n_points, seed=40 + k) for k in range(BASE)]
    prm = match_params(mode, 4)
    for n in arg("--searches", [1, 16, 64]):
        searches = [base[k % BASE] for k in range(n)]
        S, cams, cs, cf, feats, jobs = pack_searches(searches)
        # in place on the same arrays every time: the inputs come back as passed, the outputs are overwritten
        med, mm, ker, out = median_ms(lambda: match_project(t, S, cams, cs, cf, feats, jobs, prm),
                                      lambda: match_kernel_ms(t, on=True))
        gather, resolve = (float(np.median([k[i] for k in ker])) for i in (0, 1))

        def cpu():
            f, j = feats.copy(), jobs.copy()
            for R in S.copy():
                one = np.array([R])
                f0, j0 = int(R["feat0"]), int(R["job0"])
                one["feat0"] = one["job0"] = one["cam0"] = one["cell0"] = one["cf0"] = 0
                H.mh_search(ptr(one), ptr(cams[R["cam0"]:]), ptr(cs[R["cell0"]:]), ptr(cf[R["cf0"]:]), ptr(f[f0:]),
                            ptr(j[j0:]), ctypes.byref(prm))
            return f, j

        out = tuple(a.copy() for a in out)      # the device's results, before the CPU loop below reuses nothing of them
        cpu_med, cpu_mm, _, (cf_, cj_) = median_ms(cpu)
        same = all((cj_[k] == out[3][k]).all() for k in ("feat", "status", "best_dist", "best_dist2")) and \
            (cf_["job"] == out[2]["job"]).all()
        rounds = out[1]["rounds"]
        print(json.dumps({"mode": name, "searches": n, "cameras": 4, "features_per_camera": n_feat, "points": n_points,
                          "jobs": int(len(jobs)), "call_ms": round(med, 3), "call_ms_min_max": mm,
                          "k_match_gather_ms": round(gather, 4), "k_match_resolve_ms": round(resolve, 4),
                          "kernel_share": round((gather + resolve) / med, 3), "host_and_copies_ms": round(med - gather - resolve, 3), "us_per_job": round(1e3 * med / max(1, len(jobs)), 4),
                          "cpu_sequential_ms": round(cpu_med, 3), "cpu_sequential_ms_min_max": cpu_mm,
                          "gpu_equals_cpu_sequential": bool(same), "n_matches": int(out[0]["n_matches"].sum()),
                          "status_counts": np.bincount(out[3]["status"], minlength=5).tolist(),
                          "rounds_min_median_max": [int(rounds.min()), float(np.median(rounds)), int(rounds.max())],
                          "rounds_histogram": np.bincount(rounds).tolist(), "warmup": WARMUP, "reps": REPS}), flush=True)
t.close()
