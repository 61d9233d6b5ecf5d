"""lba_track_vel_ransac (k_vel_hyp / k_vel_select, amc-slam_amd/csrc/lba_track_vel.hip) against the numpy
restatement of Tracking::MCRansac / Optimizer::OptimizeVel (tests/vel_oracle.py) on the cases of tests/vel_cases.py.

Per case: the inlier flags, n_inliers and best_hyp identical; hyp_inliers identical for the settled hypotheses;
vel and the settled hyp_vel within 1e-6 max(1, |v|_inf), the project's LM-run tolerance.  hyp_iterations is only
held to 1 <= it <= iterations: three edges fit six unknowns exactly, so the stop rules fire on rounding noise
(tests/vel_oracle.py).  tests/test_vel_cases.py shows on the CPU that every frame here is settled and at most
10 % of a case's hypotheses are not.  The parity test prints the margins it measures (pytest -s).

Without an oracle, bitwise: a 300-frame batch against each frame alone, a repeated call, a Tracker that also ran
lba_track in between, NULL per-hypothesis outputs.  mc_ransac against the caller's rule on both sides of minMatch.
Bad input: every LBA_E_ARG of the header, the seventeenth (cam, dt) pair, nothing written by a refused call, and
the next valid call succeeds.
"""
import ctypes

import numpy as np
import pytest

import vel_cases as vc
from amc_lba import LbaError
from amc_lba.abi import LBA_E_ARG, LBA_E_LIMIT, ptr
from amc_lba.track import (Tracker, _bind, make_track_frames, make_vel_frames, mc_ransac, track_config, vel_params)

pytestmark = pytest.mark.gpu

N_BATCH = 300      # frames of the batch: more workgroups per launch than an MI355X has CUs (256)


@pytest.fixture(scope="module")
def tracker():
    t = Tracker(track_config())
    yield t
    t.close()


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max(initial=0.0) / max(1.0, np.abs(b).max(initial=0.0)))


@pytest.mark.parametrize("name", vc.CASES)
def test_case_matches_oracle(tracker, name):
    fr, ob, sm, cams, prm = vc.case(name)
    r = vc.reference(name)[0]
    fr_g, ob_g, (hv, hi, hit) = tracker.vel_ransac(fr.copy(), ob.copy(), sm, cams, params=prm)
    F = fr_g[0]
    s = r["settled"]
    d_vel = _rel(F["vel"], r["vel"])
    d_hyp = max([_rel(hv[h], r["hyp_vel"][h]) for h in np.nonzero(s)[0]], default=0.0)
    print(f"{name}: best {F['best_hyp']} / {r['best_hyp']}  n_inliers {F['n_inliers']} / {r['n_inliers']}  "
          f"flags differing {int((ob_g['inlier'] != r['inlier']).sum())}  settled {int(s.sum())} of {len(s)}  "
          f"hyp_inliers differing (settled) {int((hi[s] != r['hyp_inliers'][s]).sum())}  vel {d_vel:.2e}  "
          f"hyp_vel (settled) {d_hyp:.2e}  iterations GPU {hit.tolist()} oracle {r['hyp_iterations'].tolist()}")
    assert r["frame_settled"]
    assert F["best_hyp"] == r["best_hyp"] and F["n_inliers"] == r["n_inliers"]
    np.testing.assert_array_equal(ob_g["inlier"], r["inlier"])
    np.testing.assert_array_equal(hi[s], r["hyp_inliers"][s])
    assert d_vel <= vc.TOL and d_hyp <= vc.TOL
    it = prm.iterations if prm is not None else 40
    assert ((min(1, it) <= hit) & (hit <= it)).all()
    if r["best_hyp"] < 0:
        assert F["vel"].tobytes() == fr[0]["vel"].tobytes()            # untouched
    else:
        assert F["vel"].tobytes() == hv[F["best_hyp"]].tobytes() and F["n_inliers"] == hi[F["best_hyp"]]
    # everything that is not an output is as it went in
    for f in ("q", "t", "obs0", "n_obs", "hyp0", "n_hyp"):
        assert fr_g[f].tobytes() == fr[f].tobytes(), f
    for f in ("cam", "dt", "z", "w", "Xw"):
        assert ob_g[f].tobytes() == ob[f].tobytes(), f


def _batch(n_frames, seed=50):
    return make_vel_frames(n_frames=n_frames, n_obs=40, n_hyp=5, seed=seed)[:4]


def test_batch_equals_each_frame_alone(tracker):
    fr, ob, sm, cams = _batch(N_BATCH)
    fr_b, ob_b, hyp_b = tracker.vel_ransac(fr.copy(), ob.copy(), sm, cams)
    assert (fr_b["best_hyp"] >= 0).all()
    for f in range(N_BATCH):
        one = fr[f:f + 1].copy()
        one["obs0"], one["hyp0"] = 0, 0
        rows, hyps = slice(f * 40, (f + 1) * 40), slice(f * 5, (f + 1) * 5)
        fr_1, ob_1, hyp_1 = tracker.vel_ransac(one, ob[rows].copy(), sm[hyps], cams)
        for k in ("vel", "best_hyp", "n_inliers"):
            assert fr_1[0][k].tobytes() == fr_b[f][k].tobytes(), (f, k)
        assert ob_1.tobytes() == ob_b[rows].tobytes(), f
        for a, b in zip(hyp_1, hyp_b):
            assert a.tobytes() == b[hyps].tobytes(), f


def test_repeated_call_and_reuse_after_lba_track(tracker):
    from amc_lba.synth import make_window
    fr, ob, sm, cams = _batch(8, seed=51)
    first = tracker.vel_ransac(fr.copy(), ob.copy(), sm, cams)
    again = tracker.vel_ransac(fr.copy(), ob.copy(), sm, cams)
    win = make_window(n_opt_kf=4, n_lm=200, obs_per_lm=4, n_cam=4, gp=True, seed=3, perturb=False)
    tf, to = make_track_frames(win, [2, 3])
    tracker.track(tf, to, win.cams)
    after = tracker.vel_ransac(fr.copy(), ob.copy(), sm, cams)
    fresh = Tracker(track_config()).vel_ransac(fr.copy(), ob.copy(), sm, cams)
    for other in (again, after, fresh):
        assert other[0].tobytes() == first[0].tobytes() and other[1].tobytes() == first[1].tobytes()
        for a, b in zip(other[2], first[2]):
            assert a.tobytes() == b.tobytes()


def test_null_per_hypothesis_outputs(tracker):
    fr, ob, sm, cams = _batch(8, seed=52)
    fr_a, ob_a, _ = tracker.vel_ransac(fr.copy(), ob.copy(), sm, cams)
    fr_n, ob_n, none = tracker.vel_ransac(fr.copy(), ob.copy(), sm, cams, per_hyp=False)
    assert none is None and fr_n.tobytes() == fr_a.tobytes() and ob_n.tobytes() == ob_a.tobytes()


def test_unused_rows_and_hypotheses_are_left_alone(tracker):
    """Ranges in any order with unused rows and triples between them: nothing outside the ranges is written."""
    fr, ob, sm, cams = _batch(2, seed=53)
    pad_o, pad_h = np.zeros(3, ob.dtype), np.full((2, 3), -7, np.int32)
    pad_o["inlier"] = 99
    ob2 = np.concatenate([pad_o, ob[40:], pad_o, ob[:40], pad_o])
    sm2 = np.concatenate([pad_h, sm[5:], pad_h, sm[:5]])
    fr2 = fr.copy()
    fr2["obs0"], fr2["hyp0"] = [46, 3], [9, 2]
    fr_a, ob_a, hyp_a = tracker.vel_ransac(fr.copy(), ob.copy(), sm, cams)
    fr_g, ob_g, hyp_g = tracker.vel_ransac(fr2.copy(), ob2.copy(), sm2, cams)
    assert (ob_g["inlier"][[0, 1, 2, 43, 44, 45, 86, 87, 88]] == 99).all()
    assert ob_g[3:43].tobytes() == ob_a[40:].tobytes() and ob_g[46:86].tobytes() == ob_a[:40].tobytes()
    for k in ("vel", "best_hyp", "n_inliers"):
        assert fr_g[k].tobytes() == fr_a[k].tobytes()
    for a, g in zip(hyp_a, hyp_g):
        assert (g[[0, 1, 7, 8]] == 0).all() and g[2:7].tobytes() == a[5:].tobytes() and g[9:].tobytes() == a[:5].tobytes()


def test_mc_ransac_applies_the_callers_rule(tracker):
    fr, ob, sm, cams = _batch(6, seed=54)
    fr_g, ob_g, _ = tracker.vel_ransac(fr.copy(), ob.copy(), sm, cams)
    n = fr_g["n_inliers"]
    min_match = int(np.sort(n)[3])                       # frames on both sides, and one exactly at minMatch
    assert (n < min_match).any() and (n == min_match).any()
    before = np.random.default_rng(0).random(len(ob)) < 0.2
    ret, out, _, _ = mc_ransac(tracker, fr.copy(), ob.copy(), sm, cams, min_match=min_match, outlier=before)
    for f in range(len(fr)):
        rows = slice(f * 40, (f + 1) * 40)
        if n[f] < min_match:
            assert ret[f] == 0 and (out[rows] == before[rows]).all()
        else:
            assert ret[f] == n[f] and (out[rows] == (before[rows] | (ob_g["inlier"][rows] == 0))).all()


# ------------------------------------------------------------------ bad input
def _raw(handle, fr, ob, sm, cams, prm=None, n_frames=None, n_obs=None, n_hyp=None, n_cam=None):
    """The C entry point on the caller's arrays; returns (rc, hyp_vel, hyp_inliers, hyp_iterations)."""
    hv, hi, hit = np.full((len(sm), 6), -5.0), np.full(len(sm), -5, np.int32), np.full(len(sm), -5, np.int32)
    rc = _bind().lba_track_vel_ransac(
        handle, ptr(fr), len(fr) if n_frames is None else n_frames, ptr(ob), len(ob) if n_obs is None else n_obs,
        ptr(sm), len(sm) if n_hyp is None else n_hyp, ctypes.byref(prm) if prm is not None else None, ptr(cams),
        len(cams) if n_cam is None else n_cam, ptr(hv), ptr(hi), ptr(hit))
    return rc, hv, hi, hit


def _mutations():
    def cam_high(fr, ob, sm, kw): ob["cam"][5] = 4
    def cam_negative(fr, ob, sm, kw): ob["cam"][5] = -1
    def triple_high(fr, ob, sm, kw): sm[2, 1] = 40
    def triple_negative(fr, ob, sm, kw): sm[2, 1] = -1
    def triple_of_next_frame(fr, ob, sm, kw): sm[7, 0] = 45          # inside the array, outside its frame
    def triple_repeated(fr, ob, sm, kw): sm[3, 2] = sm[3, 0]
    def iterations_negative(fr, ob, sm, kw): kw["prm"] = vel_params(iterations=-1)
    def obs_range_past_end(fr, ob, sm, kw): fr["n_obs"][1] = 41
    def obs_range_negative(fr, ob, sm, kw): fr["obs0"][0] = -1
    def hyp_range_past_end(fr, ob, sm, kw): fr["n_hyp"][1] = 6
    def hyp_range_negative(fr, ob, sm, kw): fr["hyp0"][0] = -1
    def n_obs_short(fr, ob, sm, kw): kw["n_obs"] = 79
    def n_hyp_short(fr, ob, sm, kw): kw["n_hyp"] = 9
    def dt_not_finite(fr, ob, sm, kw): ob["dt"][7] = np.nan
    return [cam_high, cam_negative, triple_high, triple_negative, triple_of_next_frame, triple_repeated,
            iterations_negative, obs_range_past_end, obs_range_negative, hyp_range_past_end, hyp_range_negative,
            n_obs_short, n_hyp_short, dt_not_finite]


@pytest.mark.parametrize("mutate", _mutations(), ids=lambda m: m.__name__)
def test_bad_input_is_refused_and_writes_nothing(tracker, mutate):
    fr, ob, sm, cams = _batch(2, seed=55)
    sm = np.ascontiguousarray(sm, np.int32)
    ob["inlier"] = 77
    fr["best_hyp"], fr["n_inliers"] = 88, 99
    kw = {}
    mutate(fr, ob, sm, kw)
    fr0, ob0 = fr.copy(), ob.copy()
    rc, hv, hi, hit = _raw(tracker.h, fr, ob, sm, cams, **kw)
    assert rc == LBA_E_ARG
    assert fr.tobytes() == fr0.tobytes() and ob.tobytes() == ob0.tobytes()
    assert (hv == -5).all() and (hi == -5).all() and (hit == -5).all()
    good = _batch(2, seed=55)
    fr_g, _, _ = tracker.vel_ransac(*good)                 # the next valid call succeeds
    assert (fr_g["best_hyp"] >= 0).all()


def test_null_tracker_is_refused():
    fr, ob, sm, cams = _batch(1, seed=55)
    assert _raw(None, fr, ob, np.ascontiguousarray(sm, np.int32), cams)[0] == LBA_E_ARG


def test_seventeenth_cam_dt_pair_is_the_limit(tracker):
    fr, ob, sm, cams = _batch(1, seed=56)
    ob["dt"][:12] = 0.2 + 0.001 * np.arange(12)          # 4 pairs of the generator + 12 = 16
    assert len(set(zip(ob["cam"].tolist(), ob["dt"].tolist()))) == 16
    fr_g, _, _ = tracker.vel_ransac(fr.copy(), ob.copy(), sm, cams)
    assert fr_g[0]["best_hyp"] >= 0
    ob["dt"][12] = 0.3
    assert len(set(zip(ob["cam"].tolist(), ob["dt"].tolist()))) == 17
    ob["inlier"] = 77
    fr0, ob0 = fr.copy(), ob.copy()
    rc, hv, hi, hit = _raw(tracker.h, fr, ob, np.ascontiguousarray(sm, np.int32), cams)
    assert rc == LBA_E_LIMIT
    assert fr.tobytes() == fr0.tobytes() and ob.tobytes() == ob0.tobytes() and (hi == -5).all() and (hv == -5).all()
    with pytest.raises(LbaError):
        tracker.vel_ransac(fr.copy(), ob.copy(), sm, cams)
    fr_g, _, _ = tracker.vel_ransac(*_batch(1, seed=56))
    assert fr_g[0]["best_hyp"] >= 0


def test_empty_batch(tracker):
    fr, ob, sm, cams = _batch(1, seed=57)
    rc, hv, hi, hit = _raw(tracker.h, fr[:0].copy(), ob, np.ascontiguousarray(sm, np.int32), cams, n_frames=0)
    assert rc == 0 and (hi == -5).all() and (ob["inlier"] == 0).all()
