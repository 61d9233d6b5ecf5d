"""ORBmatcher::SearchByBoW on the GPU (lba_match_bow: one wave per (pair, common vocabulary node), idx1 serially, the
node's candidates in parallel): milliseconds per call, host checks, the merge walk, packing, upload, launch, download
and the host's rotation pass included, the kernel's time (HIP events, lba_match_bow_profile), what is left for the
host and the copies, and next to it ONE THREAD of the host running the same header's sequential function
(bow_search_host through tests/native/bow_harness.cpp, g++ -O2) on the same pairs.  Generated keyframes
(amc_lba.bow.make_bow_pairs): 4 x 1500 keypoints in 100 nodes per keyframe, the current keyframe against 1, 11 and 33
others (DetectCommonRegionsFromBoW: up to 11 covisible keyframes of about 3 candidates).  Median of 20 timed calls
after 5 warm-ups.

    python scripts/bench_bow.py [--pairs 1,11,33] [--feat 6000] [--nodes 100] [--out profiles/bow_bench.txt]

A report, not a gate: the capability is new and no speed target is set.  The one-thread column is this project's loop,
not the reference's binary.  The match counts of the two must be equal: that is asserted."""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "amc-slam_amd")]
from amc_lba.abi import BOW_ROW_DTYPE, ptr  # noqa: E402
from amc_lba.bow import bow_params, make_bow_pairs  # noqa: E402
from amc_lba.track import Tracker, track_config  # noqa: E402

WARMUP, REPS = 5, 20


def arg(name, default, conv=lambda s: [int(x) for x in s.split(",")]):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def host_harness():
    src = os.path.join(ROOT, "tests", "native", "bow_harness.cpp")
    out = os.path.join(ROOT, "tests", "native", "_build", "libbow_harness.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", out])
    L = ctypes.CDLL(out)
    L.bh_search_batch.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 8
    L.bh_search_batch.restype = ctypes.c_long
    return L


def median_ms(call, reps=REPS, warmup=WARMUP):
    ms, out = [], None
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        out = call()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), [round(min(ms), 3), round(max(ms), 3)], out


lines = ["# lba_match_bow, median of 20 calls after 5 warm-ups; host: one thread of bow_search_host (g++ -O2), this project's "
         "loop, median of 5.  No speed target.  The reference's own CPU time was not run."]
print(lines[0], flush=True)
t = Tracker(track_config())
t.match_bow_kernel_ms(True)
H = host_harness()
prm = bow_params()
n_feat, n_nodes = arg("--feat", [6000])[0], arg("--nodes", [100])[0]
for n in arg("--pairs", [1, 11, 33]):
    pairs, ekfs, feats, nid, nst, nf, _ = make_bow_pairs(n, n_feat=n_feat, n_nodes=n_nodes, seed=9)
    out = np.zeros(int(pairs["out0"][-1]) + int(ekfs["n_feat"][0]), BOW_ROW_DTYPE)
    ker = []

    def gpu():
        r = t.match_bow(pairs, ekfs, feats, nid, nst, nf, prm, out=out)
        ker.append(t.match_bow_kernel_ms(True))
        return r

    med, mm, res = median_ms(gpu)
    gpu_matches = res[0]["n_matches"].copy()
    rows, host_n = np.zeros(len(out), BOW_ROW_DTYPE), np.zeros(n, np.int32)

    def host():
        return H.bh_search_batch(ptr(pairs), n, ptr(ekfs), ptr(feats), ptr(nid), ptr(nst), ptr(nf), ctypes.byref(prm), ptr(rows),
                                 ptr(host_n))

    hmed, hmm, htotal = median_ms(host, reps=5, warmup=1)
    assert (host_n == gpu_matches).all() and rows.tobytes() == out.tobytes(), "the device and the host loop differ"
    k = float(np.median(ker[WARMUP:]))
    node_len = np.diff(nst)[np.diff(nst) > 0]
    lines.append(json.dumps({"pairs": n, "keypoints_per_keyframe": n_feat, "nodes": n_nodes,
                             "node_list_median_max": [int(np.median(node_len)), int(node_len.max())], "call_ms": round(med, 3),
                             "call_ms_min_max": mm, "k_bow_match_ms": round(k, 4), "host_and_copies_ms": round(med - k, 3),
                             "kernel_share": round(k / med, 3), "host_one_thread_ms": round(hmed, 3), "host_ms_min_max": hmm,
                             "host_over_call": round(hmed / med, 2), "matches": int(gpu_matches.sum()),
                             "host_matches": int(htotal), "status_counts": np.bincount(out["status"], minlength=6).tolist(),
                             "warmup": WARMUP, "reps": REPS}))
    print(lines[-1], flush=True)
t.close()
path = arg("--out", os.path.join(ROOT, "profiles", "bow_bench.txt"), str)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
