"""MCRansac's velocity hypotheses on the GPU (lba_track_vel_ransac, one wave per hypothesis): milliseconds per call,
host set-up, upload, both launches and download included, for one frame of 300 observations with 23 hypotheses
and for batches of 64 and 256 such frames.  For orientation the same numbers of frames of about 300 edges through
lba_track (the step after it in Tracking::TrackLocalMap).  Median of the timed calls after a warm-up.

    python scripts/bench_vel_ransac.py [--frames 1,64,256]

(one batch size per process under rocprofv3 --kernel-trace --stats gives k_vel_hyp's and k_vel_select's own times)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "amc-slam_amd")]
from amc_lba.synth import make_window  # noqa: E402
from amc_lba.track import (TRACK_FRAME_DTYPE, TRACK_OBS_DTYPE, Tracker, make_track_frames, make_vel_frames,  # noqa: E402
                           track_config)

win = make_window(n_opt_kf=12, n_fixed=1, n_lm=650, obs_per_lm=6, n_cam=4, gp=True, seed=11, perturb=False)
base_f, base_o = make_track_frames(win, list(range(2, 12)), fix_prev=True, seed=3)


def track_batch(n):
    fr = np.zeros(n, TRACK_FRAME_DTYPE)
    obs, off = [], 0
    for i in range(n):
        j = i % len(base_f)
        fr[i] = base_f[j]
        o = base_o[base_f[j]["obs0"]: base_f[j]["obs0"] + base_f[j]["n_obs"]]
        fr[i]["obs0"] = off
        off += len(o)
        obs.append(o)
    return fr, np.concatenate(obs).astype(TRACK_OBS_DTYPE)


def median_ms(call, reps):
    call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


sizes = [int(x) for x in sys.argv[sys.argv.index("--frames") + 1].split(",")] if "--frames" in sys.argv else [1, 64, 256]
t = Tracker(track_config())
for n in sizes:
    fr, ob, sm, cams, _ = make_vel_frames(n_frames=n, n_obs=300, n_hyp=23, seed=9)
    reps = 20 if n == 1 else 10
    med, lo, hi = median_ms(lambda: t.vel_ransac(fr.copy(), ob.copy(), sm, cams), reps)
    out = t.vel_ransac(fr.copy(), ob.copy(), sm, cams)
    tf, to = track_batch(n)
    tmed, tlo, thi = median_ms(lambda: t.track(tf.copy(), to.copy(), win.cams), reps)
    print(json.dumps({"frames": n, "obs_per_frame": 300, "hyp_per_frame": 23,
                      "vel_ransac_ms": round(med, 3), "vel_ransac_ms_min_max": [round(lo, 3), round(hi, 3)],
                      "mean_inliers": float(out[0]["n_inliers"].mean()), "mean_lm_iterations": float(out[2][2].mean()),
                      "lba_track_ms": round(tmed, 3), "lba_track_ms_min_max": [round(tlo, 3), round(thi, 3)],
                      "lba_track_edges_per_frame": float(tf["n_obs"].mean()), "reps": reps}), flush=True)
