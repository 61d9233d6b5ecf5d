"""The Sim3 ORBmatcher::SearchByProjection on the GPU (lba_match_sim3_project): one keyframe of 4 x 1500 features against
1, 11 and 33 hypotheses of 3000 points each, at the three call sites' parameters (LoopClosing.cc:586, :608, :800).
Median of 20 timed calls after 5 warm-ups: the whole call, each kernel between events (lba_match_sim3_project_profile),
the host part (everything that is not a kernel: checks, packing, the copies, the readback, the scatter), the rounds and the
live share of the jobs.  Alongside, for context only, with equality of the results asserted:
  * the same header's sequential loop on ONE CPU thread (s3p_search_host through tests/native/s3p_harness.cpp, g++ -O2);
  * the way without this entry point: the projection on the host (the same header, one thread), the live jobs packed for
    lba_match_project with the keyframe's 6000 features copied once per hypothesis, and that call.

    python scripts/bench_sim3_project.py [--hyps 1,11,33] [--points 3000] [--out profiles/sim3_project_bench.txt]

The points of a hypothesis sit behind random features of the keyframe, a pixel off, so neighbours compete as map points
of covisible keyframes do ("crowd": 0).  A second block repeats the largest batch with 30 % of every hypothesis's points
on ONE feature ("crowd": 0.3): the resolve's worst case, a dependency chain of several hundred rounds in one camera.

A report, not a gate: the capability is new and no speed target is set.  The hypotheses are the first pose-settled ones
of a generated keyframe (tests/s3p_cases.py: pose_settled), so the device and the host loop must agree bit for bit."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, d) for d in ("amc-slam_amd", "tests", "oracle")]
import s3p_cases as sc  # noqa: E402
import test_s3p_host as th  # noqa: E402
from amc_lba.abi import MATCH_JOB_DTYPE, ptr  # noqa: E402
from amc_lba.match import MATCH_BEST, Search, match_params, match_searches  # noqa: E402
from amc_lba.sim3_project import (S3P_POSE_DTYPE, S3P_ROW_DTYPE, LbaS3pParams, make_s3p_problem, pack_hypotheses,  # noqa: E402
                                  s3p_params, sim3_project_raw)
from amc_lba.track import Tracker, track_config  # noqa: E402

WARMUP, REPS = 5, 20
SITES = ((8, 1.5, 1), (5, 1.0, 0), (3, 1.5, 0))      # th, ratioHamming, proj_form of :586, :608, :800
STRETCH = ("k_s3p_pose", "k_s3p_project", "k_s3p_compact_base", "readback_and_sizing", "k_s3p_gather", "k_s3p_resolve")


def arg(name, default, conv=lambda s: [int(x) for x in s.split(",")]):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def median_ms(call, reps=REPS, warmup=WARMUP):
    ms, out = [], None
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        out = call()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), [round(min(ms), 3), round(max(ms), 3)], out


def main():
    lines = ["# lba_match_sim3_project, median of 20 calls after 5 warm-ups; one keyframe of 4 x 1500 features.  host_loop: one "
             "thread of s3p_search_host (g++ -O2), this project's loop, median of 3.  parent_way: host projection + "
             "lba_match_project with the keyframe copied per hypothesis, median of 3.  No speed target; the reference's own "
             "CPU time was not run."]
    print(lines[0], flush=True)
    n_points = arg("--points", [3000])[0]
    counts = arg("--hyps", [1, 11, 33])
    t = Tracker(track_config())
    for crowd, cnts in ((0.0, counts), (0.3, counts[-1:])):
        block(t, lines, crowd, cnts, n_points)
    t.close()
    path = arg("--out", os.path.join(ROOT, "profiles", "sim3_project_bench.txt"), str)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def block(t, lines, crowd, counts, n_points):
    kfm, pool = make_s3p_problem(n_cam=4, n_feat=1500, n_hyp=max(counts) + 8, n_points=n_points, seed=11, crowd=crowd)
    pool = [h for h in pool if sc.pose_settled(kfm, h)]
    assert len(pool) >= max(counts), "not enough settled hypotheses: generate more"
    t.sim3_project_kernel_ms(True)
    H = th.load_harness()
    H.sh_project_all.argtypes = [ctypes.c_void_p] * 5 + [ctypes.POINTER(LbaS3pParams)] + [ctypes.c_void_p] * 2
    H.sh_project_all.restype = None
    n_cam, nf = kfm.n_cam, len(kfm.feats)
    for n in counts:
        hyps = pool[:n]
        S, points, taken = pack_hypotheses(kfm, hyps)
        rows = np.zeros(len(points) * n_cam, S3P_ROW_DTYPE)
        fp = np.zeros(n * nf, np.int32)
        poses = np.zeros(n * n_cam, S3P_POSE_DTYPE)
        for th_, ratio, form in SITES:
            prm = s3p_params(th_, ratio, form)
            ker = []

            def gpu():
                rc = sim3_project_raw(t, kfm, S, points, taken, rows, fp, poses, prm)
                assert rc == 0
                ker.append(t.sim3_project_kernel_ms(True))

            med, mm, _ = median_ms(gpu)
            k = np.median(np.array(ker[WARMUP:]), axis=0)
            kernels = float(k[[0, 1, 2, 4, 5]].sum())
            live = np.isin(rows["status"], (0, 1, 2))
            # ---- one thread of the same header's loop
            h_rows, h_fp, h_poses = np.zeros_like(rows), np.zeros_like(fp), np.zeros_like(poses)
            h_n = np.zeros(n, np.int64)

            def host():
                for i in range(n):
                    r0 = int(S[i]["row0"])
                    h_n[i] = H.sh_search(ptr(kfm.kf), ptr(kfm.kcams), ptr(kfm.gcams), ptr(kfm.sf), ptr(kfm.cell_start),
                                         ptr(kfm.cell_feat), ptr(kfm.feats), nf, ptr(S[i:i + 1]), ptr(points), None,
                                         ctypes.byref(prm), ptr(h_rows[r0:]), ptr(h_fp[i * nf:]), ptr(h_poses[i * n_cam:]))

            hmed, hmm, _ = median_ms(host, reps=3, warmup=1)
            h_poses["rounds"] = poses["rounds"]
            assert (h_n == S["n_matches"]).all() and h_rows.tobytes() == rows.tobytes() and h_fp.tobytes() == fp.tobytes()
            assert (h_poses["tcw"].view(np.uint32) == poses["tcw"].view(np.uint32)).all(), "the float Tcw differs"
            # ---- the way without this entry point
            mp = match_params(MATCH_BEST, n_cam, th_high=int(np.floor(np.float32(50) * np.float32(ratio))), stereo_cam=-1,
                              ur_truncate=0, check_orientation=0)
            p_rows, p_poses = np.zeros_like(rows), np.zeros_like(poses)

            def parent():
                searches, where = [], []
                for i in range(n):
                    r0, m = int(S[i]["row0"]), len(hyps[i].points) * n_cam
                    H.sh_project_all(ptr(kfm.kf), ptr(kfm.kcams), ptr(kfm.sf), ptr(S[i:i + 1]), ptr(points), ctypes.byref(prm),
                                     ptr(p_rows[r0:]), ptr(p_poses[i * n_cam:]))
                    r = p_rows[r0:r0 + m]
                    idx = np.flatnonzero(r["status"] == -1)
                    jobs = np.zeros(len(idx), MATCH_JOB_DTYPE)
                    for f in ("x", "y", "radius"):
                        jobs[f] = r[f][idx]
                    jobs["cam"], jobs["max_level"], jobs["min_level"] = idx % n_cam, r["level"][idx], r["level"][idx] - 1
                    jobs["point"], jobs["blocks"], jobs["desc"] = idx // n_cam, 1, hyps[i].points["desc"][idx // n_cam]
                    searches.append(Search(kfm.gcams, kfm.cell_start, kfm.cell_feat, kfm.feats, jobs))
                    where.append(r0 + idx)
                rec, out = match_searches(t, searches, mp)
                return rec, out, where

            pmed, pmm, (rec, out, where) = median_ms(parent, reps=3, warmup=1)
            assert (rec["n_matches"] == S["n_matches"]).all()
            for o, w in zip(out, where):
                assert (o.jobs["feat"] == rows["feat"][w]).all() and (o.jobs["status"] == rows["status"][w]).all()
            lines.append(json.dumps({
                "hypotheses": n, "points_each": n_points, "crowd": crowd, "th": th_, "ratio": ratio, "proj_form": form, "jobs": int(len(rows)),
                "live_share": round(float(live.mean()), 4), "call_ms": round(med, 3), "call_ms_min_max": mm,
                **{s: round(float(v), 4) for s, v in zip(STRETCH, k)}, "kernels_ms": round(kernels, 4),
                "host_part_ms": round(med - kernels, 3), "kernel_share": round(kernels / med, 3),
                "rounds_max_mean": [int(poses["rounds"].max()), round(float(poses["rounds"].mean()), 2)],
                "matches": int(S["n_matches"].sum()), "host_loop_one_thread_ms": round(hmed, 3), "host_loop_min_max": hmm,
                "parent_way_ms": round(pmed, 3), "parent_way_min_max": pmm, "warmup": WARMUP, "reps": REPS}))
            print(lines[-1], flush=True)


if __name__ == "__main__":
    main()
