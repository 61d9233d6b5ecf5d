"""lba_sim3_ransac on the GPU: the named cases (tests/sim3_ransac_cases.py) against the fp64 restatement
(tests/sim3_ransac_oracle.py), and, without an oracle, bitwise: a 300-pair batch against each pair alone, repeated
calls, a tracker that ran its other entry points in between, a fresh tracker, inputs returned as passed, refused calls.

Against the restatement: every degenerate / non-finite flag identical; hyp_inliers within the number of unsettled rows
of that hypothesis (identical where there are none); best_hyp, converged identical and n_inliers the selected
hypothesis's count; every settled row's inlier flag identical; q (up to sign), t and s of every settled transform within
sim3_cases.TOL = 1e-6 relative to max(1, |.|_inf).  The margins measured are printed (pytest -s) and recorded in
profiles/sim3_ransac_margins.log."""
import numpy as np
import pytest

import sim3_cases
import sim3_ransac_cases as rc
from amc_lba.abi import LBA_E_ARG, LBA_E_LIMIT, ptr
from amc_lba.sim3_ransac import (S3R_MAX_CAM, S3R_PAIR_OUTPUTS, _bind, make_sim3_ransac_pairs, seed_sim3_pairs)
from amc_lba.track import Tracker, make_track_frames, make_vel_frames, track_config

pytestmark = pytest.mark.gpu

N_BATCH = 300      # pairs of the batch: with 8 hypotheses each, far more workgroups than an MI355X has CUs (256)
PAIR_INPUTS = [f for f in rc.S3R_PAIR_DTYPE.names if f not in S3R_PAIR_OUTPUTS]
CORR_INPUTS = [f for f in rc.S3R_CORR_DTYPE.names if f != "inlier"]


@pytest.fixture(scope="module")
def tracker():
    t = Tracker(track_config())
    yield t
    t.close()


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:2], b[:2])) and all(a[2][k].tobytes() == b[2][k].tobytes() for k in a[2])


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_matches_restatement(tracker, name):
    assert sim3_cases.TOL == 1e-6
    c, r64, _ = rc.case(name)
    got = rc.run_device(tracker, c)
    problems, fig = rc.device_gaps(c, r64, got)
    print(f"{name}: S12 of settled transforms within {fig['S12']:.2e}; count differences {fig['flags']} on {fig['unsettled']} unsettled flags")
    assert not problems, problems
    for f in PAIR_INPUTS:
        assert got[0][f].tobytes() == c.pairs[f].tobytes(), f
    for f in CORR_INPUTS:
        assert got[1][f].tobytes() == c.corr[f].tobytes(), f


def test_untouched_without_a_selection(tracker):
    for name in ("n_hyp_0", "identity_rotation"):
        c, _, _ = rc.case(name)
        pairs, corr = c.pairs.copy(), c.corr.copy()
        pairs["q"], pairs["t"], pairs["s"] = (0.1, 0.2, 0.3, 0.4), (5.0, 6.0, 7.0), 8.0
        pairs["best_hyp"], pairs["n_inliers"], pairs["converged"] = 7, 7, 7
        corr["inlier"] = 9
        p, r, _ = tracker.sim3_ransac(pairs.copy(), corr, c.samples.copy(), c.cams, c.n_cam)
        assert p[0]["best_hyp"] == -1 and p[0]["n_inliers"] == 0 and p[0]["converged"] == 0 and not r["inlier"].any()
        for f in ("q", "t", "s"):
            assert p[f].tobytes() == pairs[f].tobytes()


def _batch():
    """N_BATCH pairs: four generated candidates (20, 65 and 129 rows) tiled, each copy with triples of its own"""
    rng = np.random.default_rng(5)
    parts = [make_sim3_ransac_pairs(n_corr=n, n_hyp=0, seed=60 + k, min_inliers=6)[:4] for k, n in enumerate((20, 65, 129, 33))]
    pairs, corr, samples, cams = [], [], [], []
    r0 = h0 = 0
    for k in range(N_BATCH):
        p, c, _, m = parts[k % 4]
        p = p.copy()
        n = len(c)
        s = np.stack([rng.choice(n, 3, replace=False) for _ in range(8)]).astype(np.int32)
        p["corr0"], p["cam0"], p["hyp0"], p["n_hyp"] = r0, 8 * k, h0, 8
        pairs.append(p); corr.append(c); samples.append(s); cams.append(m)
        r0, h0 = r0 + n, h0 + 8
    return np.concatenate(pairs), np.concatenate(corr), np.concatenate(samples), np.concatenate(cams)


def test_batch_equals_each_pair_alone(tracker):
    pairs, corr, samples, cams = _batch()
    bp, bc, bh = tracker.sim3_ransac(pairs.copy(), corr.copy(), samples, cams, 4)
    assert (bp["best_hyp"] >= 0).all() and bp["converged"].any()
    for k in list(range(0, N_BATCH, 37)) + [N_BATCH - 1]:
        P = pairs[k]
        one = pairs[k:k + 1].copy()
        rows = slice(int(P["corr0"]), int(P["corr0"] + P["n_corr"]))
        hyps = slice(int(P["hyp0"]), int(P["hyp0"] + 8))
        one["corr0"], one["cam0"], one["hyp0"] = 0, 0, 0
        sp, sc_, sh = tracker.sim3_ransac(one, corr[rows].copy(), samples[hyps], cams[8 * k:8 * k + 8], 4)
        for f in S3R_PAIR_OUTPUTS:
            assert sp[0][f].tobytes() == bp[k][f].tobytes(), (k, f)
        assert sc_.tobytes() == bc[rows].tobytes(), k
        for key in sh:
            assert sh[key].tobytes() == bh[key][hyps].tobytes(), (k, key)


def test_repeated_call_other_calls_between_and_fresh_tracker(tracker):
    from amc_lba.posegraph import essential_graph, make_pose_graph
    from amc_lba.sim3 import make_sim3_pairs
    from amc_lba.synth import make_window
    c, _, _ = rc.case("n_hyp_300")
    first = rc.run_device(tracker, c)
    again = rc.run_device(tracker, c)
    win = make_window(n_opt_kf=4, n_lm=200, obs_per_lm=4, n_cam=4, gp=True, seed=3, perturb=False)
    tf, to = make_track_frames(win, [2, 3])
    tracker.track(tf, to, win.cams)
    fr, ob, sm, vcams, _ = make_vel_frames(n_frames=2, n_obs=40, n_hyp=5, seed=51)
    tracker.vel_ransac(fr, ob, sm, vcams)
    sp, sc_, scams, _ = make_sim3_pairs(n_pairs=2, n_corr=30, seed=4)
    tracker.sim3_optimize(sp, sc_, scams, 4)
    v, e, _ = essential_graph(make_pose_graph(n_kf=12, seed=3))
    tracker.posegraph_optimize(v.copy(), e, True, 3)
    after = rc.run_device(tracker, c)
    other = Tracker(track_config())
    fresh = rc.run_device(other, c)
    other.close()
    for res in (again, after, fresh):
        assert _same(res, first)


def test_chains_into_sim3_optimize(tracker):
    pairs, corr, samples, cams, truth = make_sim3_ransac_pairs(n_pairs=2, n_corr=60, n_hyp=100, seed=81, outlier_frac=0.2)
    rp, rcorr, _ = tracker.sim3_ransac(pairs, corr, samples, cams, 4)
    assert rp["converged"].all()
    s3p, s3c = truth["sim3_pairs"].copy(), truth["sim3_corr"].copy()
    s3p["q"], s3p["t"], s3p["s"] = (0, 0, 0, 1), 0, 1
    assert seed_sim3_pairs(rp, s3p).all()
    for f in ("q", "t", "s"):
        assert s3p[f].tobytes() == rp[f].tobytes()
    # the inlier rows only, as vpMatchedMP after the RANSAC
    keep = rcorr["inlier"] != 0
    rows, n0 = [], 0
    for p in range(2):
        sel = np.flatnonzero(keep[60 * p:60 * p + 60]) + 60 * p
        s3p["corr0"][p], s3p["n_corr"][p] = n0, len(sel)
        rows.append(s3c[sel])
        n0 += len(sel)
    out, _ = tracker.sim3_optimize(s3p, np.concatenate(rows), cams, 4)
    assert (out["n_in"] >= 10).all(), out["n_in"]


def _call(tracker, pairs, corr, samples, cams, n_cam=4, n_cam_rows=None, n_hyp=None, h=None):
    hyp = np.full((len(samples), 8), 7.0), np.full(len(samples), 7, np.int32), np.full(len(samples), 7, np.int32)
    rc_ = _bind().lba_sim3_ransac(tracker.h if h is None else h, ptr(pairs), len(pairs), ptr(corr), len(corr), ptr(samples),
                                  len(samples) if n_hyp is None else n_hyp, ptr(cams), len(cams) if n_cam_rows is None else n_cam_rows,
                                  n_cam, ptr(hyp[0]), ptr(hyp[1]), ptr(hyp[2]))
    return rc_, hyp


def _refused(tracker, pairs, corr, samples, cams, code=LBA_E_ARG, **kw):
    p, c = pairs.copy(), corr.copy()
    rc_, hyp = _call(tracker, p, c, np.ascontiguousarray(samples, np.int32), cams, **kw)
    assert rc_ == code
    assert p.tobytes() == pairs.tobytes() and c.tobytes() == corr.tobytes()      # nothing written
    assert (hyp[0] == 7).all() and (hyp[1] == 7).all() and (hyp[2] == 7).all()


def test_refused_calls_write_nothing_and_the_next_call_succeeds(tracker):
    pairs, corr, samples, cams, _ = make_sim3_ransac_pairs(n_pairs=2, n_corr=20, n_hyp=5, seed=91, min_inliers=5)
    corr["inlier"] = 5
    pairs["n_inliers"] = -3

    def mod(arr, k, field, value):
        out = arr.copy()
        if field is None:
            out[k] = value
        else:
            out[field][k] = value
        return out

    L = _bind()
    a = (ptr(pairs), 2, ptr(corr), len(corr), ptr(samples), len(samples), ptr(cams), len(cams), 4, None, None, None)
    assert L.lba_sim3_ransac(None, *a) == LBA_E_ARG
    for null in (0, 2, 4, 6):
        b = list(a)
        b[null] = None
        assert L.lba_sim3_ransac(tracker.h, *b) == LBA_E_ARG
    for neg in (1, 3, 5, 7):
        b = list(a)
        b[neg] = -1
        assert L.lba_sim3_ransac(tracker.h, *b) == LBA_E_ARG
    _refused(tracker, pairs, corr, samples, cams, n_cam=0)
    _refused(tracker, mod(pairs, 1, "corr0", -1), corr, samples, cams)
    _refused(tracker, mod(pairs, 1, "n_corr", -1), corr, samples, cams)
    _refused(tracker, mod(pairs, 1, "n_corr", 21), corr, samples, cams)         # past the end of corr
    _refused(tracker, mod(pairs, 1, "hyp0", -1), corr, samples, cams)
    _refused(tracker, mod(pairs, 1, "n_hyp", -1), corr, samples, cams)
    _refused(tracker, mod(pairs, 1, "n_hyp", 6), corr, samples, cams)           # past the end of samples
    _refused(tracker, pairs, corr, samples, cams, n_hyp=9)
    _refused(tracker, mod(pairs, 1, "cam0", -1), corr, samples, cams)
    _refused(tracker, mod(pairs, 1, "cam0", 9), corr, samples, cams)            # 9 + 8 > 16 camera rows
    _refused(tracker, pairs, corr, samples, cams, n_cam_rows=15)
    _refused(tracker, pairs, mod(corr, 39, "cam1", 4), samples, cams)
    _refused(tracker, pairs, mod(corr, 39, "cam2", -1), samples, cams)
    _refused(tracker, pairs, corr, mod(samples, 9, None, (0, 1, 20)), cams)     # outside [0, n_corr) of its pair
    _refused(tracker, pairs, corr, mod(samples, 9, None, (0, -1, 2)), cams)
    for rep in ((3, 3, 5), (3, 5, 3), (5, 3, 3)):
        _refused(tracker, pairs, corr, mod(samples, 9, None, rep), cams)         # a repeated index
    _refused(tracker, mod(pairs, 1, "min_inliers", -1), corr, samples, cams)
    _refused(tracker, pairs, mod(corr, 39, "max_err1", np.nan), samples, cams)
    _refused(tracker, pairs, mod(corr, 39, "max_err2", np.nan), samples, cams)
    # the limit of the header: more than 64 cameras per keyframe
    many = np.concatenate([cams] * 9)[:2 * (S3R_MAX_CAM + 1)]
    _refused(tracker, pairs[:1], corr, samples, many, n_cam=S3R_MAX_CAM + 1, code=LBA_E_LIMIT)
    ok = np.concatenate([cams[:4]] * 16 + [cams[4:8]] * 16)                      # exactly 64: accepted
    p1 = pairs[:1].copy()
    rc_, _ = _call(tracker, p1, corr.copy(), samples, ok, n_cam=S3R_MAX_CAM)
    assert rc_ == 0
    # the next valid call succeeds, and an infinite gate is a gate
    p, c, h = tracker.sim3_ransac(pairs.copy(), mod(corr, 39, "max_err1", np.inf), samples, cams, 4)
    assert (p["best_hyp"] >= 0).all() and (h["flags"] == 0).all()
    assert p1[0]["best_hyp"] == p[0]["best_hyp"] and p1[0]["n_inliers"] == p[0]["n_inliers"]


def test_empty_calls(tracker):
    pairs, corr, samples, cams, _ = make_sim3_ransac_pairs(n_pairs=2, n_corr=20, n_hyp=5, seed=92, min_inliers=5)
    L = _bind()
    assert L.lba_sim3_ransac(tracker.h, None, 0, None, 0, None, 0, ptr(cams), len(cams), 4, None, None, None) == 0
    empty = pairs.copy()
    empty["n_corr"][1], empty["n_hyp"][1] = 0, 0
    empty["best_hyp"], empty["n_inliers"], empty["converged"] = 5, 5, 5
    p, c = tracker.sim3_ransac(empty.copy(), corr.copy(), samples, cams, 4, per_hyp=False)
    assert p[1]["best_hyp"] == -1 and p[1]["n_inliers"] == 0 and p[1]["converged"] == 0
    assert c[20:].tobytes() == corr[20:].tobytes() and p[0]["best_hyp"] >= 0
