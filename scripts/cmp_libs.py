"""Bitwise comparison between two builds of the engine (A/B of a change that must not move a result bit), each build in
its own child process, selected by AMC_LBA_LIB ("main": the tree's library):
    python scripts/cmp_libs.py <lib A> <lib B> [config]    LM runs of Problem.optimize on a window config
    python scripts/cmp_libs.py <lib A> <lib B> tracker     every entry point of the tracker handle (lba_track,
        lba_track_vel_ransac, lba_sim3_optimize, lba_sim3_ransac, lba_posegraph_optimize, lba_triangulate,
        lba_match_project), each case with early_stop 0 and 1, on the smallest shapes that reach every branch of their
        LM loops and of their host halves; every output array is hashed.  The four calls on the pinned arena run once
        more with their event bracket on ("timed"), so that path is compared too."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _h(*arrays):
    import numpy as np
    d = hashlib.sha256()
    for a in arrays:
        d.update(np.ascontiguousarray(a).tobytes())
    return d.hexdigest()[:16]


def child(cfg):
    sys.path.insert(0, os.path.join(ROOT, "amc-slam_amd"))
    from amc_lba import Problem
    from amc_lba.synth import make_config_window
    win = make_config_window(cfg)
    p = Problem(win, early_stop=0)
    n, st = p.optimize(10)
    kf, lm = p.state()
    print(json.dumps({"n": n, "trials": st.trials, "chi2": st.chi2_final, "kf_t": _h(kf["t"]), "kf_q": _h(kf["q"]),
                      "lm": _h(lm)}))


def child_tracker():
    sys.path.insert(0, os.path.join(ROOT, "amc-slam_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import match_cases as mc
    import posegraph_cases as pc
    from amc_lba.match import match_params, pack_searches
    from amc_lba.posegraph import posegraph_optimize
    from amc_lba.sim3 import make_sim3_pairs
    from amc_lba.sim3_ransac import make_sim3_ransac_pairs
    from amc_lba.synth import make_window
    from amc_lba.track import Tracker, make_track_frames, make_vel_frames, track_config
    from amc_lba.triangulate import make_tri_pairs
    out = {}

    def sim3(t, n_corr, fix_scale):
        p, c, cams, _ = make_sim3_pairs(n_pairs=3, n_corr=n_corr, n_cam=4, seed=71, fix_scale=fix_scale)
        return _h(*t.sim3_optimize(p, c, cams, 4))

    def sim3_ransac(t, n_corr):
        p, c, s, cams, _ = make_sim3_ransac_pairs(n_pairs=2, n_corr=n_corr, n_hyp=40, seed=61, min_inliers=6)
        p, c, hyp = t.sim3_ransac(p, c, s, cams, 4)
        return _h(p, c, *[hyp[k] for k in sorted(hyp)])

    def triangulate(t, n_pairs):
        p, r, kfs, cams, _ = make_tri_pairs(n_pairs=n_pairs, n_rows=70, shared_current=True)
        return _h(*t.triangulate(p, r, kfs, cams, 4))

    def match(t, mode):
        # two searches (1 and 2 cameras) in which some jobs match and some do not, in either mode
        # (tests/test_gpu_tracker_profile.py checks that on the CPU)
        S, cams, cs, cf, feats, jobs = pack_searches(mc.small_batch(mode, 2))
        return _h(*t.match_project(S, cams, cs, cf, feats, jobs, match_params(mode, 1)))
    win = make_window(n_opt_kf=4, n_lm=200, obs_per_lm=4, n_cam=4, gp=True, seed=3, perturb=False)
    for es in (0, 1):
        t = Tracker(track_config(early_stop=es))
        for fix_prev in (True, False):                       # d0 = 12 / 0
            f, o = make_track_frames(win, [2, 3], fix_prev=fix_prev)
            f, o = t.track(f, o, win.cams)
            out[f"track fix_prev={int(fix_prev)} es={es}"] = _h(f, o)
        for n_obs in (40, 130):                              # one / three 64-bit mask words
            f, o, s, cams, _ = make_vel_frames(n_frames=2, n_obs=n_obs, n_hyp=5, seed=51)
            f, o, hyp = t.vel_ransac(f, o, s, cams)
            out[f"vel_ransac n_obs={n_obs} es={es}"] = _h(f, o, *hyp)
        for n_corr in (30, 100):                             # one / two passes per lane
            for fix_scale in (False, True):
                out[f"sim3 n_corr={n_corr} fix_scale={int(fix_scale)} es={es}"] = sim3(t, n_corr, fix_scale)
        for n_corr in (20, 129):                             # one / three mask words per hypothesis
            out[f"sim3_ransac n_corr={n_corr} es={es}"] = sim3_ransac(t, n_corr)
        for n_pairs in (1, 3):                               # 70 rows: two chunks, 64 + 6; three pairs share the current KF
            out[f"triangulate n_pairs={n_pairs} es={es}"] = triangulate(t, n_pairs)
        for mode in mc.BOTH:
            out[f"match_project {mc.MODE_NAME[mode]} es={es}"] = match(t, mode)
        timed = {"sim3": lambda: sim3(t, 100, False), "sim3_ransac": lambda: sim3_ransac(t, 129),
                 "triangulate": lambda: triangulate(t, 3), "match": lambda: match(t, mc.MATCH_BEST)}
        for name, call in timed.items():                     # the same calls inside their event bracket
            getattr(t, name + "_kernel_ms")(True)
            out[f"{name} timed es={es}"] = call()
            getattr(t, name + "_kernel_ms")(False)
        for name in ("loop150", "hub"):
            for lam in (1e-16, 0.0):                         # the user's lambda / computeLambdaInit
                v, e, fix = pc.case(name)
                v, st = posegraph_optimize(t, v, e, fix, 20, lam)
                out[f"posegraph {name} lambda_init={lam:g} es={es}"] = _h(v) + " " + json.dumps(st, sort_keys=True)
        t.close()
    print(json.dumps(out))


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child_tracker() if sys.argv[2] == "tracker" else child(sys.argv[2])
        sys.exit(0)
    cfg = sys.argv[3] if len(sys.argv) > 3 else "cfg1_local_50kf"
    out = []
    for lib in sys.argv[1:3]:
        env = dict(os.environ, AMC_LBA_LIB=lib) if lib != "main" else dict(os.environ)
        r = subprocess.run([sys.executable, __file__, "--child", cfg], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(f"{lib}: child failed ({r.returncode})\n{r.stderr[-2000:]}")
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(lib, out[-1] if cfg != "tracker" else f"{len(out[-1])} cases")
    if cfg == "tracker":
        for k in out[0]:
            print(f"{k}: {'bitwise identical' if out[0][k] == out[1].get(k) else 'DIFFERENT'}   {out[0][k][:16]}")
    print("bitwise identical" if out[0] == out[1] else "DIFFERENT")
