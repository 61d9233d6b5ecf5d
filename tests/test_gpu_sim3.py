"""lba_sim3_optimize (k_sim3, amc-slam_amd/csrc/lba_sim3.hip) against the numpy restatement of
Optimizer::OptimizeSim3 (tests/sim3_oracle.py, analytic Jacobian) on the cases of tests/sim3_cases.py.

Per case: every outlier flag, n_bad and n_in identical (tests/test_sim3_cases.py shows on the CPU that the analytic
run's integers are those of the reference-faithful numeric-Jacobian run and survive a 1e-6 disturbance of H and b);
q (up to sign), t and s within 1e-6 max(1, |.|_inf), the project's LM-run tolerance; `iterations` is only held to
1 <= it <= 5 + nMore: near the minimum the gain ratio's sign is rounding.  The parity test prints
the margins it measures (pytest -s).

Without an oracle, bitwise: the early return leaves S12 as passed, every input field is as passed, a 300-pair batch
against each pair alone, a repeated call, a tracker that ran lba_track and lba_track_vel_ransac in between, a fresh
tracker, correspondence and camera ranges out of order.  Bad input: every LBA_E_ARG of the header and the LDS limit,
nothing written by a refused call, and the next valid call succeeds.
"""
import numpy as np
import pytest

import sim3_cases as sc
import sim3_oracle as so
from amc_lba import LbaError
from amc_lba.abi import LBA_E_ARG, LBA_E_LIMIT, ptr
from amc_lba.sim3 import SIM3_PAIR_OUTPUTS, _bind, make_sim3_pairs
from amc_lba.track import Tracker, make_track_frames, make_vel_frames, track_config

pytestmark = pytest.mark.gpu

N_BATCH = 300      # pairs of the batch: more workgroups per launch than an MI355X has CUs (256)
PAIR_INPUTS = ("th2", "fix_scale", "corr0", "n_corr", "cam0", "pad")
CORR_INPUTS = ("cam1", "cam2", "pad", "X1c", "X2c", "z1", "z2", "w1", "w2")


@pytest.fixture(scope="module")
def tracker():
    t = Tracker(track_config())
    yield t
    t.close()


def _state(p):
    return dict(q=np.array(p["q"]), t=np.array(p["t"]), s=float(p["s"]))


@pytest.mark.parametrize("name", sc.CASES)
def test_case_matches_restatement(tracker, name):
    pairs, corr, cams, n_cam = sc.case(name)
    r = sc.reference(name)
    pg, cg = tracker.sim3_optimize(pairs.copy(), corr.copy(), cams.copy(), n_cam)
    P = pg[0]
    gq, gt, gs = so.state_gap(_state(P), r)
    n_more = 10 if r["n_bad"] > 0 else 5
    print(f"{name}: n_bad {P['n_bad']} / {r['n_bad']}  n_in {P['n_in']} / {r['n_in']}  "
          f"flags differing {int((cg['outlier'] != r['outlier']).sum())}  q {gq:.2e}  t {gt:.2e}  s {gs:.2e}  "
          f"iterations GPU {P['iterations']} restatement {r['iterations']}")
    np.testing.assert_array_equal(cg["outlier"], r["outlier"])
    assert P["n_bad"] == r["n_bad"] and P["n_in"] == r["n_in"]
    assert max(gq, gt, gs) <= sc.TOL
    if len(corr) == 0:
        assert P["iterations"] == 0
    else:
        assert 1 <= P["iterations"] <= (5 if r["ret0"] else 5 + n_more)
    if r["ret0"]:
        for f in ("q", "t", "s"):
            assert P[f].tobytes() == pairs[0][f].tobytes(), f           # the early return: S12 bitwise the input
    if pairs["fix_scale"][0]:
        assert P["s"] == pairs["s"][0]                                  # bitwise
    # everything that is not an output is as it went in
    for f in PAIR_INPUTS:
        assert pg[f].tobytes() == pairs[f].tobytes(), f
    for f in CORR_INPUTS:
        assert cg[f].tobytes() == corr[f].tobytes(), f
    assert set(PAIR_INPUTS) | set(SIM3_PAIR_OUTPUTS) == set(pairs.dtype.names)


def test_return0_leaves_s12_bitwise(tracker):
    pairs, corr, cams, n_cam = sc.case("return0_12_3")
    corr["outlier"] = 7                                                 # (an output: every row is written)
    pg, cg = tracker.sim3_optimize(pairs.copy(), corr.copy(), cams, n_cam)
    assert pg[0]["n_in"] == 0 and pg[0]["n_bad"] == 3 and 1 <= pg[0]["iterations"] <= 5
    for f in ("q", "t", "s"):
        assert pg[f].tobytes() == pairs[f].tobytes(), f
    assert sorted(cg["outlier"].tolist()) == [0] * 9 + [1] * 3
    assert (cg["outlier"].astype(bool) == sc.truth("return0_12_3")["gross"]).all()


def _batch(n_pairs, seed=70):
    return make_sim3_pairs(n_pairs=n_pairs, n_corr=40, n_cam=4, seed=seed)[:3]


def _alone(tracker, pairs, corr, cams, k, n_cam=4):
    """Pair k of a batch as a call of its own."""
    one = pairs[k:k + 1].copy()
    rows = slice(int(one["corr0"][0]), int(one["corr0"][0] + one["n_corr"][0]))
    cam = slice(int(one["cam0"][0]), int(one["cam0"][0]) + 2 * n_cam)
    one["corr0"], one["cam0"] = 0, 0
    return tracker.sim3_optimize(one, corr[rows].copy(), cams[cam].copy(), n_cam), rows


def test_batch_equals_each_pair_alone(tracker):
    pairs, corr, cams = _batch(N_BATCH)
    pb, cb = tracker.sim3_optimize(pairs.copy(), corr.copy(), cams, 4)
    assert (pb["n_in"] > 0).any() and (pb["iterations"] >= 1).all()
    for k in range(N_BATCH):
        (p1, c1), rows = _alone(tracker, pairs, corr, cams, k)
        for f in SIM3_PAIR_OUTPUTS:
            assert p1[0][f].tobytes() == pb[k][f].tobytes(), (k, f)
        assert c1.tobytes() == cb[rows].tobytes(), k


def test_repeated_call_and_reuse_after_other_tracker_calls(tracker):
    from amc_lba.synth import make_window
    pairs, corr, cams = _batch(8, seed=71)
    first = tracker.sim3_optimize(pairs.copy(), corr.copy(), cams, 4)
    again = tracker.sim3_optimize(pairs.copy(), corr.copy(), cams, 4)
    win = make_window(n_opt_kf=4, n_lm=200, obs_per_lm=4, n_cam=4, gp=True, seed=3, perturb=False)
    tf, to = make_track_frames(win, [2, 3])
    tracker.track(tf, to, win.cams)
    fr, ob, sm, vcams, _ = make_vel_frames(n_frames=2, n_obs=40, n_hyp=5, seed=51)
    tracker.vel_ransac(fr, ob, sm, vcams)
    after = tracker.sim3_optimize(pairs.copy(), corr.copy(), cams, 4)
    other = Tracker(track_config())
    fresh = other.sim3_optimize(pairs.copy(), corr.copy(), cams, 4)
    other.close()
    for res in (again, after, fresh):
        assert res[0].tobytes() == first[0].tobytes() and res[1].tobytes() == first[1].tobytes()


def test_ranges_out_of_order(tracker):
    """Two pairs whose corr0 and cam0 ranges lie in the arrays in the other order, with unused rows and cameras
    between them: each pair as alone, nothing outside the ranges written."""
    a = sc.case("clean_40")
    b = sc.case("outliers_10pct")
    pad_c = np.zeros(3, a[1].dtype)
    pad_c["outlier"] = 99
    pad_m = np.zeros(2, a[2].dtype)
    corr = np.concatenate([pad_c, b[1], pad_c, a[1], pad_c])
    cams = np.concatenate([pad_m, b[2], pad_m, a[2]])
    pairs = np.concatenate([a[0], b[0]])
    pairs["corr0"] = [3 + len(b[1]) + 3, 3]
    pairs["cam0"] = [2 + 8 + 2, 2]
    pg, cg = tracker.sim3_optimize(pairs.copy(), corr.copy(), cams, 4)
    for k, single in enumerate((a, b)):
        p1, c1 = tracker.sim3_optimize(single[0].copy(), single[1].copy(), single[2], 4)
        for f in SIM3_PAIR_OUTPUTS:
            assert p1[0][f].tobytes() == pg[k][f].tobytes(), (k, f)
        rows = slice(int(pairs["corr0"][k]), int(pairs["corr0"][k] + pairs["n_corr"][k]))
        assert c1.tobytes() == cg[rows].tobytes(), k
    used = np.zeros(len(corr), bool)
    used[3:3 + len(b[1])] = True
    used[pairs["corr0"][0]:pairs["corr0"][0] + len(a[1])] = True
    assert cg[~used].tobytes() == corr[~used].tobytes()


def test_empty_calls(tracker):
    pairs, corr, cams = _batch(2, seed=72)
    L = _bind()
    assert L.lba_sim3_optimize(tracker.h, None, 0, None, 0, ptr(cams), len(cams), 4) == 0
    assert L.lba_sim3_optimize(tracker.h, ptr(pairs), 0, ptr(corr), len(corr), ptr(cams), len(cams), 4) == 0
    empty = pairs.copy()
    empty["n_corr"][1] = 0
    empty["n_in"], empty["n_bad"], empty["iterations"] = 5, 5, 5
    pg, cg = tracker.sim3_optimize(empty.copy(), corr.copy(), cams, 4)
    assert pg[1]["n_in"] == 0 and pg[1]["n_bad"] == 0 and pg[1]["iterations"] == 0
    for f in ("q", "t", "s"):
        assert pg[1][f].tobytes() == pairs[1][f].tobytes()
    assert cg[40:].tobytes() == corr[40:].tobytes() and pg[0]["iterations"] >= 1


def _refused(tracker, pairs, corr, cams, n_cam=4, n_cam_rows=None, code=LBA_E_ARG, h=None):
    p, c = pairs.copy(), corr.copy()
    rc = _bind().lba_sim3_optimize(tracker.h if h is None else h, ptr(p), len(p), ptr(c), len(c), ptr(cams),
                                   len(cams) if n_cam_rows is None else n_cam_rows, n_cam)
    assert rc == code
    assert p.tobytes() == pairs.tobytes() and c.tobytes() == corr.tobytes()      # nothing written


def test_refused_calls_write_nothing(tracker):
    pairs, corr, cams = _batch(2, seed=73)
    corr["outlier"] = 5
    pairs["n_in"] = -3

    def mod(arr, k, field, value):
        out = arr.copy()
        out[field][k] = value
        return out

    L = _bind()
    assert L.lba_sim3_optimize(None, ptr(pairs), 2, ptr(corr), len(corr), ptr(cams), len(cams), 4) == LBA_E_ARG
    assert L.lba_sim3_optimize(tracker.h, None, 2, ptr(corr), len(corr), ptr(cams), len(cams), 4) == LBA_E_ARG
    assert L.lba_sim3_optimize(tracker.h, ptr(pairs), 2, None, len(corr), ptr(cams), len(cams), 4) == LBA_E_ARG
    assert L.lba_sim3_optimize(tracker.h, ptr(pairs), 2, ptr(corr), len(corr), None, len(cams), 4) == LBA_E_ARG
    assert L.lba_sim3_optimize(tracker.h, ptr(pairs), -1, ptr(corr), len(corr), ptr(cams), len(cams), 4) == LBA_E_ARG
    assert L.lba_sim3_optimize(tracker.h, ptr(pairs), 2, ptr(corr), -1, ptr(cams), len(cams), 4) == LBA_E_ARG
    _refused(tracker, pairs, corr, cams, n_cam=0)
    _refused(tracker, mod(pairs, 1, "corr0", -1), corr, cams)
    _refused(tracker, mod(pairs, 1, "n_corr", -1), corr, cams)
    _refused(tracker, mod(pairs, 1, "n_corr", 41), corr, cams)                   # past the end of corr
    _refused(tracker, mod(pairs, 1, "cam0", -1), corr, cams)
    _refused(tracker, mod(pairs, 1, "cam0", 9), corr, cams)                      # 9 + 8 > 16 camera rows
    _refused(tracker, pairs, corr, cams, n_cam_rows=15)
    _refused(tracker, pairs, mod(corr, 79, "cam1", 4), cams)
    _refused(tracker, pairs, mod(corr, 79, "cam2", -1), cams)
    for bad in (0.0, -1.0, np.nan, np.inf):
        _refused(tracker, mod(pairs, 1, "th2", bad), corr, cams)
    for bad in (0.0, -1.0, np.nan, np.inf):
        _refused(tracker, mod(pairs, 1, "s", bad), corr, cams)
    # the compiled limit: more rows than a workgroup's LDS holds
    big_p, big_c, big_m = make_sim3_pairs(n_pairs=1, n_corr=8, n_cam=4, seed=74)[:3]
    big_c = np.concatenate([big_c] * 100)
    big_p["n_corr"] = len(big_c)
    _refused(tracker, big_p, big_c, big_m, code=LBA_E_LIMIT)
    with pytest.raises(LbaError):
        tracker.sim3_optimize(mod(pairs, 0, "s", -1.0), corr.copy(), cams, 4)
    # and the next valid call succeeds, as before
    pg, cg = tracker.sim3_optimize(pairs.copy(), corr.copy(), cams, 4)
    other = Tracker(track_config())
    pf, cf = other.sim3_optimize(pairs.copy(), corr.copy(), cams, 4)
    other.close()
    assert pg.tobytes() == pf.tobytes() and cg.tobytes() == cf.tobytes() and (pg["iterations"] >= 1).all()
