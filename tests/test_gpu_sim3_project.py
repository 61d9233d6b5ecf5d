"""lba_match_sim3_project on the GPU: every named case (tests/s3p_cases.py) at the three call sites' parameters in both
projection forms IDENTICAL to the restatement (tests/s3p_oracle.py: `sequential`, with `by_jobs` for the rounds) in
status, feat, best_dist, level, the bits of x, y, radius and of the float Tcw, the per-feature point, n_matches and rounds;
the fp64 Tcw within M_POSE (a miss is a failure); and, without an oracle, bitwise: a 33-hypothesis batch on one keyframe
against each hypothesis alone, two runs, a fresh tracker against one that ran lba_match_project and lba_match_bow; the
device's echoed jobs through lba_match_project; the chain sim3_ransac -> sim3_project -> sim3_optimize -> sim3_project
on one handle; refused calls write nothing and leave a message.

Outputs are pre-filled with junk, so every row must be written; inputs come back byte for byte; nothing is written
behind the last row.  Every case and seed used here is settled (tests/test_s3p_cases.py checks that on the CPU)."""
import numpy as np
import pytest

import s3p_cases as sc
import s3p_oracle as so
from amc_lba.abi import LBA_E_ARG, LBA_E_LIMIT, MATCH_JOB_DTYPE
from amc_lba.bow import make_bow_pairs
from amc_lba.match import MATCH_BEST, MATCH_MAX_FEAT, Search, build_grid, match_params, match_searches, tracker_last_error
from amc_lba.sim3_project import (S3P_MAX_CAM, S3P_POSE_DTYPE, S3P_ROW_DTYPE, Hypothesis, Keyframe,
                                  pack_hypotheses, scw_from_pair, sim3_project_raw)
from amc_lba.sim3_ransac import make_sim3_ransac_pairs, seed_sim3_pairs
from amc_lba.track import Tracker, track_config

pytestmark = pytest.mark.gpu

JUNK = -77
EXTRA = 3
KF_ARRAYS = ("kf", "kcams", "gcams", "sf", "cell_start", "cell_feat", "feats")
LIVE = (0, 1, 2)
_ref = {}


@pytest.fixture(scope="module")
def tracker():
    t = Tracker(track_config())
    yield t
    t.close()


def reference(key, kfm, hyps, p):
    """the restatement of a problem, computed once and shared"""
    if (key, p) not in _ref:
        prm = sc.params(p)
        out = []
        for h in hyps:
            res = so.by_jobs(kfm, h, prm)[0]
            assert so.sequential(kfm, h, prm).same(res)
            out.append(res)
        _ref[(key, p)] = out
    return _ref[(key, p)]


def junk_outputs(kfm, hyps):
    n_rows = sum(len(h.points) for h in hyps) * kfm.n_cam
    rows = np.full(8 * (n_rows + EXTRA), JUNK, np.int32).view(S3P_ROW_DTYPE)
    fp = np.full(len(hyps) * len(kfm.feats) + EXTRA, JUNK, np.int32)
    poses = np.full(38 * (len(hyps) * kfm.n_cam + EXTRA), JUNK, np.int32).view(S3P_POSE_DTYPE)
    return rows, fp, poses


def device(tracker, kfm, hyps, prm, expect=0):
    """a list of s3p_oracle.Result (rounds filled), after the junk, input and overrun checks"""
    k = kfm.copy()
    S, points, taken = pack_hypotheses(k, hyps)
    S["n_matches"] = JUNK
    S0, points0, taken0 = S.copy(), points.copy(), taken.copy()
    rows, fp, poses = junk_outputs(k, hyps)
    rc = sim3_project_raw(tracker, k, S, points, taken, rows, fp, poses, prm)
    assert rc == expect, (rc, tracker_last_error(tracker))
    for a in KF_ARRAYS:
        assert getattr(k, a).tobytes() == getattr(kfm, a).tobytes(), a
    assert points.tobytes() == points0.tobytes() and taken.tobytes() == taken0.tobytes()
    for f in S.dtype.names:
        if f != "n_matches":
            assert S[f].tobytes() == S0[f].tobytes(), f
    n_rows, nf, n_cam = len(points) * k.n_cam, len(k.feats), k.n_cam
    assert (rows[n_rows:].view(np.int32) == JUNK).all() and (fp[len(hyps) * nf:] == JUNK).all()
    assert (poses[len(hyps) * n_cam:].view(np.int32) == JUNK).all()
    if expect != 0:
        assert (rows.view(np.int32) == JUNK).all() and (fp == JUNK).all() and (poses.view(np.int32) == JUNK).all()
        assert (S["n_matches"] == JUNK).all()
        return None
    out = []
    for i, h in enumerate(hyps):
        r = so.Result(len(h.points), n_cam, nf)
        r0 = int(S[i]["row0"])
        r.rows = rows[r0:r0 + len(h.points) * n_cam].reshape(len(h.points), n_cam)
        r.feat_point = fp[i * nf:(i + 1) * nf]
        r.poses = poses[i * n_cam:(i + 1) * n_cam]
        r.n_matches = int(S[i]["n_matches"])
        assert (r.rows["pad"] == 0).all() and (r.poses["pad"] == 0).all()
        out.append(r)
    return out


def identical(got, want, kfm, label):
    for i, (g, w) in enumerate(zip(got, want)):
        for f in ("status", "feat", "best_dist", "level"):
            assert (g.rows[f] == w.rows[f]).all(), (label, i, f, np.argwhere(g.rows[f] != w.rows[f])[:5])
        for f in ("x", "y", "radius"):
            assert (g.rows[f].view(np.uint32) == w.rows[f].view(np.uint32)).all(), (label, i, f)
        assert (g.poses["tcw"].view(np.uint32) == w.poses["tcw"].view(np.uint32)).all(), (label, i, "tcw")
        assert (g.feat_point == w.feat_point).all() and g.n_matches == w.n_matches, (label, i)
        assert (g.poses["rounds"] == w.poses["rounds"]).all(), (label, i, g.poses["rounds"], w.poses["rounds"])
        if kfm.kf[0]["has_prev"]:
            rel = so.pose_diff(g.poses["tcw_d"], w.poses["tcw_d"])
            assert rel.max() <= sc.M_POSE, (label, i, rel.max())      # a miss is a failure, not a margin to widen


def bitwise(a, b):
    return all(x.rows.tobytes() == y.rows.tobytes() and x.feat_point.tobytes() == y.feat_point.tobytes()
               and x.poses.tobytes() == y.poses.tobytes() and x.n_matches == y.n_matches for x, y in zip(a, b))


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_identical_to_restatement(tracker, name):
    kfm, hyps, _ = sc.case(name)
    for p in sc.PARAMS:
        identical(device(tracker, kfm, hyps, sc.params(p)), reference(name, kfm, hyps, p), kfm, (name, p))


@pytest.mark.parametrize("seed", sc.GPU_SEEDS)
def test_generated_hypotheses_identical_to_restatement(tracker, seed):
    kfm, hyps = sc.gpu_problem(seed)
    for p in (sc.PARAMS[0], sc.PARAMS[3], sc.PARAMS[4]):
        got = device(tracker, kfm, hyps, sc.params(p))
        identical(got, reference(("seed", seed), kfm, hyps, p), kfm, (seed, p))
        assert sum(g.n_matches for g in got) > 0 and max(int(g.poses["rounds"].max()) for g in got) > 1


def test_batch_of_33_equals_each_hypothesis_alone_two_runs(tracker):
    kfm, hyps = sc.batch_33()
    assert len(hyps) == 33
    hyps = list(hyps)
    hyps[5] = Hypothesis(hyps[5].q, hyps[5].t, hyps[5].s, hyps[5].points[:0])              # a search without points
    tk = (np.arange(len(kfm.feats)) % 7 == 0).astype(np.uint8)
    hyps[7] = Hypothesis(hyps[7].q, hyps[7].t, hyps[7].s, hyps[7].points, tk)              # one with a taken row
    prm = sc.params(sc.PARAMS[1])
    batch = device(tracker, kfm, hyps, prm)
    assert bitwise(device(tracker, kfm, hyps, prm), batch)
    for i, h in enumerate(hyps):
        assert bitwise(device(tracker, kfm, [h], prm), batch[i:i + 1]), i
    # a search's result does not depend on its position: the batch reversed
    rev = device(tracker, kfm, hyps[::-1], prm)
    assert bitwise(rev[::-1], batch)
    # ... and against the restatement, on a few of them
    few = [0, 7, 32]
    identical([batch[i] for i in few], reference("batch", kfm, [hyps[i] for i in few], sc.PARAMS[1]), kfm, "batch")


def _echo_search(kfm, h, res):
    """the device's echoed live jobs as lba_match_job records on the keyframe as one lba_match_project search"""
    p, c = np.nonzero(np.isin(res.rows["status"], LIVE))
    jobs = np.zeros(len(p), MATCH_JOB_DTYPE)
    for f in ("x", "y", "radius"):
        jobs[f] = res.rows[f][p, c]
    jobs["cam"], jobs["min_level"], jobs["max_level"] = c, res.rows["level"][p, c] - 1, res.rows["level"][p, c]
    jobs["point"], jobs["blocks"], jobs["desc"] = p, 1, h.points["desc"][p]
    feats = kfm.feats.copy()
    feats["taken"] = 0 if h.taken is None else h.taken
    return Search(kfm.gcams, kfm.cell_start, kfm.cell_feat, feats, jobs), p, c


def test_echoed_jobs_through_match_project_and_fresh_tracker(tracker):
    """the echoed jobs fed to lba_match_project (LBA_MATCH_BEST) give the same features; and a tracker that ran
    lba_match_project and lba_match_bow before gives what a fresh one gives"""
    kfm, hyps = sc.gpu_problem(sc.GPU_SEEDS[0])
    prm = sc.params(sc.PARAMS[0])
    other = Tracker(track_config())
    fresh = device(other, kfm, hyps, prm)
    other.close()
    mp = match_params(MATCH_BEST, kfm.n_cam, th_high=75, stereo_cam=-1, ur_truncate=0, check_orientation=0)
    for h, res in zip(hyps, fresh):
        s, p, c = _echo_search(kfm, h, res)
        S, out = match_searches(tracker, [s], mp)
        assert (out[0].jobs["status"] == res.rows["status"][p, c]).all()
        assert (out[0].jobs["feat"] == res.rows["feat"][p, c]).all()
        assert (out[0].jobs["best_dist"] == res.rows["best_dist"][p, c]).all()
        assert int(S[0]["n_matches"]) == res.n_matches
        assert (out[0].cams["rounds"] == res.poses["rounds"]).all()
    bp = make_bow_pairs(3, n_feat=120, n_nodes=8, seed=4)
    tracker.match_bow(*bp[:6])
    assert bitwise(device(tracker, kfm, hyps, prm), fresh)


def test_chain_ransac_project_optimize_project_on_one_handle(tracker):
    """sim3_ransac -> scw_from_pair -> sim3_project -> sim3_optimize -> scw_from_pair -> sim3_project"""
    kfm, hyps = sc.gpu_problem(sc.GPU_SEEDS[1])
    h = hyps[0]
    pairs, corr, samples, cams, truth = make_sim3_ransac_pairs(n_pairs=1, n_corr=60, n_hyp=100, seed=81, outlier_frac=0.2)
    rp, rcorr, _ = tracker.sim3_ransac(pairs, corr, samples, cams, 4)
    assert rp["converged"].all()

    def smw_for(pair):
        """the matched keyframe's pose for which gScm * gSmw is (nearly) this hypothesis's Sbw: Scm^-1 Sbw, scale dropped"""
        from amc_lba.sim3_project import quat_mul, quat_rot
        q1 = np.asarray(pair["q"], float) / np.linalg.norm(pair["q"])
        qi = np.array([-q1[0], -q1[1], -q1[2], q1[3]])
        return quat_mul(qi, h.q.astype(float)), quat_rot(qi, h.t.astype(float) / float(h.s) - np.asarray(pair["t"], float) / float(pair["s"]))

    prm = sc.params(sc.PARAMS[0])
    q_mw, t_mw = smw_for(rp[0])
    q, t, s = scw_from_pair(rp[0], q_mw, t_mw)
    first = device(tracker, kfm, [Hypothesis(q, t, s, h.points)], prm)[0]
    s3p, s3c = truth["sim3_pairs"].copy(), truth["sim3_corr"].copy()
    assert seed_sim3_pairs(rp, s3p).all()
    keep = np.flatnonzero(rcorr["inlier"] != 0)
    s3p["corr0"], s3p["n_corr"] = 0, len(keep)
    out, _ = tracker.sim3_optimize(s3p, s3c[keep], cams, 4)
    assert (out["n_in"] >= 10).all()
    q_mw, t_mw = smw_for(out[0])
    q, t, s = scw_from_pair(out[0], q_mw, t_mw)
    second = device(tracker, kfm, [Hypothesis(q, t, s, h.points)], sc.params(sc.PARAMS[3]))[0]
    print("chain: %d matches after the RANSAC (th 8, 1.5), %d after OptimizeSim3 (th 5, 1.0)" % (first.n_matches, second.n_matches))
    assert first.n_matches > 0 and second.n_matches > 0


def test_profile_reports_six_stretches(tracker):
    kfm, hyps = sc.gpu_problem(sc.GPU_SEEDS[0])
    tracker.sim3_project_kernel_ms(True)
    device(tracker, kfm, hyps, sc.params(sc.PARAMS[0]))
    ms = tracker.sim3_project_kernel_ms(False)
    assert len(ms) == 6 and all(m >= 0 for m in ms), ms


def _refuse(tracker, kfm, hyps, prm, code, word, edit=None):
    """the call refused: the code, the text, and nothing written"""
    k = kfm.copy()
    S, points, taken = pack_hypotheses(k, hyps)
    S["n_matches"] = JUNK
    rows, fp, poses = junk_outputs(k, hyps)
    args = dict(kfm=k, searches=S, points=points, taken=taken, rows=rows, feat_point=fp, poses=poses)
    if edit:
        edit(args)
    before = {n: (a.tobytes() if isinstance(a, np.ndarray) else None) for n, a in args.items()}
    rc = sim3_project_raw(tracker, args["kfm"], args["searches"], args["points"], args["taken"], args["rows"],
                          args["feat_point"], args["poses"], prm)
    assert rc == code, (rc, word)
    assert word in tracker_last_error(tracker), tracker_last_error(tracker)
    for n, a in args.items():
        if isinstance(a, np.ndarray):
            assert a.tobytes() == before[n], n


def test_refused_calls_write_nothing_and_the_next_call_succeeds(tracker):
    kfm, hyps, _ = sc.case("generated_4cam")
    ok = sc.params(sc.PARAMS[0])
    _refuse(tracker, kfm, hyps, sc.params((8, 5.125, 0)), LBA_E_ARG, "vpMatched[-1]")              # quirk (g)
    _refuse(tracker, kfm, hyps, sc.params((8, 1.5, 2)), LBA_E_ARG, "proj_form")
    _refuse(tracker, kfm, hyps, sc.params((-1, 1.5, 0)), LBA_E_ARG, "negative")
    _refuse(tracker, kfm, hyps, sc.params((8, float("nan"), 0)), LBA_E_ARG, "ratio_hamming")

    def set_(name, field, idx, value):
        def edit(a):
            arr = a[name] if name != "kfm" else None
            if arr is None:
                getattr(a["kfm"], field[0])[field[1]][idx] = value
            else:
                arr[field][idx] = value
        return edit

    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "points outside", set_("searches", "n_points", 1, 10 ** 6))
    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "rows outside", set_("searches", "row0", 1, 0))
    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "feat_point", set_("searches", "featpt0", 1, 1))
    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "poses", set_("searches", "pose0", 1, 10 ** 6))
    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "taken row", set_("searches", "taken0", 0, 0))
    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "scale", set_("searches", "s", 0, 0.0))
    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "n_cam < 1", set_("kfm", ("kf", "n_cam"), 0, 0))
    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "n_levels", set_("kfm", ("kf", "n_levels"), 0, 0))
    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "camera outside", set_("kfm", ("feats", "cam"), 3, 9))
    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "cell names", set_("kfm", ("feats", "cam"), 3, (int(kfm.feats["cam"][3]) + 1) % 4))

    def cells(a):
        a["kfm"].cell_start[5:] += 1
    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "cell_start past", cells)

    def dec(a):
        a["kfm"].cell_start[7] = a["kfm"].cell_start[-1] + 5
    _refuse(tracker, kfm, hyps, ok, LBA_E_ARG, "decreases", dec)
    # limits: n_cam > 64 (checked before the grid is read), 8193 features in one camera
    _refuse(tracker, kfm, hyps, ok, LBA_E_LIMIT, "n_cam > 64", set_("kfm", ("kf", "n_cam"), 0, S3P_MAX_CAM + 1))
    big, bh, _ = sc.case("lds_limit")
    feats = np.concatenate([big.feats, big.feats[:1]])
    cs, cf = build_grid(feats, big.gcams)
    over = Keyframe(big.kf, big.kcams, big.gcams, big.sf, cs, cf, feats)
    assert np.bincount(over.feats["cam"]).max() == MATCH_MAX_FEAT + 1
    _refuse(tracker, over, bh, ok, LBA_E_LIMIT, "8192")
    # the tracker is as usable as before
    identical(device(tracker, kfm, hyps, ok), reference("generated_4cam", kfm, hyps, sc.PARAMS[0]), kfm, "after refusals")


def test_empty_calls(tracker):
    kfm, hyps, _ = sc.case("generated_1cam")
    prm = sc.params(sc.PARAMS[0])
    assert device(tracker, kfm, [], prm) == []
    none = Hypothesis(hyps[0].q, hyps[0].t, hyps[0].s, hyps[0].points[:0])
    r = device(tracker, kfm, [none], prm)[0]
    assert r.n_matches == 0 and (r.feat_point == -1).all() and (r.poses["rounds"] == 0).all()
    # a keyframe without features
    bare = Keyframe(kfm.kf, kfm.kcams, kfm.gcams, kfm.sf, np.zeros_like(kfm.cell_start), kfm.cell_feat[:0], kfm.feats[:0])
    got = device(tracker, bare, hyps, prm)
    identical(got, reference("bare", bare, hyps, sc.PARAMS[0]), bare, "no features")
    assert all(g.n_matches == 0 for g in got) and any((g.rows["status"] == 1).any() for g in got)
