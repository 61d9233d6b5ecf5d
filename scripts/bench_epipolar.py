"""ORBmatcher::SearchForTriangulation on the GPU (lba_match_epipolar: one lane per keypoint of KF1, one wave per 64
entries of a common node): milliseconds per call, host checks, packing, upload, two launches, download and the host's
counting included, the two kernels' times (HIP events, lba_match_epipolar_profile), and next to it ONE THREAD of the
host running the same header's sequential function (epi_search_host through tests/native/epi_harness.cpp, g++ -O2) on
the same pairs.  Generated keyframes (amc_lba.epipolar.make_epi_pairs): 4 cameras, the current keyframe against 1 and
20 neighbours.  Median of 20 timed calls after 5 warm-ups.

    python scripts/bench_epipolar.py [--pairs 1,20] [--feat 1500] [--nodes 100]

A report, not a gate: the capability is new and no speed target is set.  The reference's own CPU time for this
function was not run: Eigen and DBoW2 cannot be built where this was measured; the one-thread figure is the product's
restatement of it, which does the same loops on the same data in fp64."""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "amc-slam_amd")]
from amc_lba.abi import EPI_ROW_DTYPE, ptr  # noqa: E402
from amc_lba.epipolar import epi_params, make_epi_pairs  # noqa: E402
from amc_lba.track import Tracker, track_config  # noqa: E402

WARMUP, REPS, N_CAM = 5, 20, 4


def arg(name, default):
    return [int(x) for x in sys.argv[sys.argv.index(name) + 1].split(",")] if name in sys.argv else default


def host_harness():
    src = os.path.join(ROOT, "tests", "native", "epi_harness.cpp")
    out = os.path.join(ROOT, "tests", "native", "_build", "libepi_harness.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", out])
    L = ctypes.CDLL(out)
    L.eh_search.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 6
    return L


def median_ms(call, reps=REPS, warmup=WARMUP):
    ms, out = [], None
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        out = call()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), [round(min(ms), 3), round(max(ms), 3)], out


print("# lba_match_epipolar, median of 20 calls after 5 warm-ups; host: one thread of epi_search_host (g++ -O2), median "
      "of 5.  No speed target.  The reference's own CPU time was not run (Eigen and DBoW2 cannot be built here).", flush=True)
t = Tracker(track_config())
t.match_epipolar_kernel_ms(True)
H = host_harness()
prm = epi_params()
n_feat, n_nodes = arg("--feat", [1500])[0], arg("--nodes", [100])[0]
for n in arg("--pairs", [1, 20]):
    pairs, kfs, ekfs, cams, feats, nid, nst, nf, _ = make_epi_pairs(n, N_CAM, n_feat, n_nodes, seed=9)
    out = np.zeros(int(pairs["out0"][-1]) + int(ekfs["n_feat"][0]), EPI_ROW_DTYPE)
    ker = []

    def gpu():
        r = t.match_epipolar(pairs, kfs, ekfs, cams, N_CAM, feats, nid, nst, nf, prm, out=out)
        ker.append(t.match_epipolar_kernel_ms(True))
        return r

    med, mm, res = median_ms(gpu)
    gpu_matches = res[0]["n_matches"].copy()
    rows = np.zeros(int(ekfs["n_feat"][0]), EPI_ROW_DTYPE)

    def host():
        total = []
        for P in pairs:
            c1, c2 = (np.ascontiguousarray(cams[kfs[k]["cam0"]:kfs[k]["cam0"] + N_CAM]) for k in (P["kf1"], P["kf2"]))
            total.append(H.eh_search(ptr(ekfs[P["kf1"]:P["kf1"] + 1]), ptr(ekfs[P["kf2"]:P["kf2"] + 1]), ptr(c1), ptr(c2), N_CAM,
                                     ptr(feats), ptr(nid), ptr(nst), ptr(nf), ctypes.byref(prm), ptr(rows)))
        return total

    hmed, hmm, htotal = median_ms(host, reps=5, warmup=1)
    k = np.median(np.array(ker[WARMUP:]), axis=0)
    print(json.dumps({"pairs": n, "keypoints_per_keyframe": N_CAM * n_feat, "nodes": n_nodes, "call_ms": round(med, 3),
                      "call_ms_min_max": mm, "k_epi_tables_ms": round(float(k[0]), 4), "k_epi_match_ms": round(float(k[1]), 4),
                      "kernel_share": round(float(k.sum()) / med, 3), "host_one_thread_ms": round(hmed, 3),
                      "host_ms_min_max": hmm, "host_over_call": round(hmed / med, 2),
                      "matches": int(gpu_matches.sum()), "host_matches": int(np.sum(htotal)),
                      "status_counts": np.bincount(out["status"], minlength=6).tolist(), "warmup": WARMUP, "reps": REPS}),
          flush=True)
t.close()
