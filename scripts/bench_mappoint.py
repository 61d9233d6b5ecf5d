"""MapPoint's refresh on the GPU (lba_mappoint_refresh) at the call sites' shapes: one keyframe's points (3000 points of
3 to 30 observations, both functions: ProcessNewKeyFrame, SearchInNeighbors), the LocalGPBA tail (20 000 points of
about 6, normal and depth only), a global-BA tail (200 000 of about 6, normal and depth only) and long tracks (500
points of 200 observations, both functions).  Median of 20 timed calls after 5 warm-ups, with the spread: the whole
call and the three kernels between events (lba_mappoint_refresh_profile), so the host part (checks, classes, packing,
the copies, the write-back) is the difference.  Alongside, with equality of every point asserted, mp_refresh_point of
the same header on ONE CPU thread (tests/native/mp_harness.cpp, g++ -O2), median of 3.  That CPU loop is this project's
code, not the reference's binary, which cannot be built here.

    python scripts/bench_mappoint.py [--out profiles/mappoint_bench.txt]

A report, not a gate: the capability is new and no speed target is set."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, d) for d in ("amc-slam_amd", "tests", "oracle")]
import mp_oracle as mo  # noqa: E402
import test_mp_host as th  # noqa: E402
from amc_lba.abi import MP_OBS_DTYPE, MP_POINT_DTYPE  # noqa: E402
from amc_lba.mappoint import refresh_raw, synthetic_keyframes  # noqa: E402
from amc_lba.track import Tracker, track_config  # noqa: E402

WARMUP, REPS = 5, 20
N_CAM = 4


def median_ms(call, reps=REPS, warmup=WARMUP):
    ms = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), [round(min(ms), 3), round(max(ms), 3)]


def tracks(K, n_points, lo, hi, n_feat, rng):
    """per point lo .. hi observations spread over the (keyframe, camera) slots of consecutive keyframes from a random
    start, in the map's order (keyframes ascending, cameras ascending)"""
    n_kf = len(K.kfs)
    n = rng.integers(lo, hi + 1, n_points)
    n_kfs = np.minimum(n_kf, n)
    start = (rng.random(n_points) * (n_kf - n_kfs + 1)).astype(np.int64)
    total = int(n.sum())
    first = np.concatenate([[0], np.cumsum(n)[:-1]])
    within = np.arange(total) - np.repeat(first, n)
    slot = np.repeat(start, n) * N_CAM + (within * np.repeat(n_kfs * N_CAM, n)) // np.repeat(n, n)   # ascending slots
    obs = np.zeros(total, MP_OBS_DTYPE)
    obs["kf"] = slot // N_CAM
    obs["feat"] = (slot % N_CAM) * n_feat + rng.integers(0, n_feat, total)
    return n, first, obs


def main():
    lines = ["# lba_mappoint_refresh, median of 20 calls after 5 warm-ups, [min, max] beside it.  kernels_ms: k_mp_geom, "
             "k_mp_desc_wave, k_mp_desc_block between events.  host_loop: one thread of mp_refresh_point from the same "
             "header (g++ -O2), median of 3: this project's code, not the reference's binary, which cannot be built "
             "here.  No speed target."]
    print(lines[0], flush=True)
    t = Tracker(track_config())
    H = th.load_harness()
    t.mappoint_refresh_kernel_ms(True)
    shapes = [("one_keyframes_points", 3000, 3, 30, 3, 30, 1000), ("local_gpba_tail", 20000, 3, 9, 1, 40, 1000),
              ("global_ba_tail", 200000, 3, 9, 1, 400, 500), ("long_tracks", 500, 200, 200, 3, 60, 500)]
    for name, n_points, lo, hi, ops, n_kf, n_feat in shapes:
        rng = np.random.default_rng([n_points, 0xBE])
        K = synthetic_keyframes(n_kf, N_CAM, n_feat, rng, spread=3.0)
        n, first, obs = tracks(K, n_points, lo, hi, n_feat, rng)
        P = np.zeros(n_points, MP_POINT_DTYPE)
        P["pos"], P["ops"] = rng.normal(0, 8.0, (n_points, 3)), ops
        P["n_obs"], P["obs0"], P["ref_kf"] = n, first, obs["kf"][first]
        kf_bad = (rng.random(n_kf) < 0.05).astype(np.int32)
        out = P.copy()
        ker = []

        def gpu():
            out[:] = P
            assert refresh_raw(t, out, obs, K, kf_bad) == 0
            ker.append(t.mappoint_refresh_kernel_ms(True))

        med, mm = median_ms(gpu)
        k_ms = np.median(np.array(ker[WARMUP:]), axis=0)
        host_out = [None]

        def host():
            host_out[0] = th.host_refresh(H, P, obs, K, kf_bad)

        hmed, hmm = median_ms(host, reps=3, warmup=1)
        assert mo.diff_fields(out, host_out[0]) == [], "the device and the host loop differ"
        lines.append(json.dumps({
            "shape": name, "points": n_points, "observations": int(len(obs)), "obs_per_point": [lo, hi], "ops": ops,
            "keyframes": n_kf, "features": int(len(K.feats)), "call_ms": round(med, 3), "call_ms_min_max": mm,
            "kernels_ms": [round(float(x), 4) for x in k_ms], "host_part_ms": round(med - float(k_ms.sum()), 3),
            "host_loop_one_thread_ms": round(hmed, 3), "host_loop_min_max": hmm, "warmup": WARMUP, "reps": REPS}))
        print(lines[-1], flush=True)
    t.close()
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mappoint_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
