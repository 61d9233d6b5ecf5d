"""lba_mappoint_refresh on the GPU: every named case (tests/mp_cases.py) and generated batches of about 2000 points
IDENTICAL to the restatement (tests/mp_oracle.py) with no tolerance: status, n, best_obs, best_median and the desc words,
the float32 bits of normal, min_distance and max_distance, a NaN matching a NaN.  Without an oracle, bitwise: a
2000-point batch with both size classes against each point alone, a fresh tracker against one that ran lba_match_fuse
and lba_match_epipolar before.  The chain on one handle: match_fuse -> fuse_walk on a ToyMap -> refresh -> points_to_s3p
-> match_fuse.  Refused calls write nothing and leave a message.

The out fields are pre-filled with junk, so every one must be written; what the reference does not write comes back
byte for byte; inputs are untouched."""
import ctypes

import numpy as np
import pytest

import mp_cases as mc
import mp_oracle as mo
from amc_lba.abi import LBA_E_ARG, LBA_E_LIMIT, MP_POINT_DTYPE, ptr
from amc_lba.mappoint import (MP_DESC, MP_NORMAL, MP_OK, LbaMpParams, _bind, keyframes_from_targets, obs_from_map,
                              pack_points, points_to_s3p, refresh)
from amc_lba.match import MATCH_MAX_FEAT, tracker_last_error
from amc_lba.track import Tracker, track_config

pytestmark = pytest.mark.gpu

JUNK = -77
ARRAYS = ("kfs", "ekfs", "cams", "feats")
_ref = {}


@pytest.fixture(scope="module")
def tracker():
    t = Tracker(track_config())
    yield t
    t.close()


def call(tracker, P, obs, K, kf_bad=None, over=None):
    """the C call with any argument replaced by name (`over`)"""
    bad = None if kf_bad is None else np.ascontiguousarray(kf_bad, np.int32)
    prm = LbaMpParams(float(K.scale_top))
    a = dict(points=ptr(P), n_points=len(P), obs=ptr(obs), n_obs=len(obs), kfs=ptr(K.kfs), ekfs=ptr(K.ekfs),
             n_kf=len(K.kfs), cams=ptr(K.cams), n_cam_rows=len(K.cams), n_cam=K.n_cam, feats=ptr(K.feats),
             n_feats=len(K.feats), kf_bad=None if bad is None else ptr(bad), prm=ctypes.byref(prm))
    over = over or {}
    assert set(over) <= set(a)
    a.update(over)
    return _bind().lba_mappoint_refresh(tracker.h, *a.values())


def device(tracker, P, obs, K, kf_bad=None, expect=0, over=None):
    """the refreshed points after the junk, untouched-input and refusal checks"""
    P = np.ascontiguousarray(P, MP_POINT_DTYPE).copy()
    for f in ("n", "best_obs", "best_median", "status"):
        P[f] = JUNK
    P0, obs0 = P.copy(), obs.copy()
    K0 = {a: getattr(K, a).copy() for a in ARRAYS}
    bad0 = None if kf_bad is None else np.array(kf_bad).copy()
    rc = call(tracker, P, obs, K, kf_bad, over)
    assert rc == expect, (rc, tracker_last_error(tracker))
    assert obs.tobytes() == obs0.tobytes() and all(getattr(K, a).tobytes() == K0[a].tobytes() for a in ARRAYS)
    assert kf_bad is None or np.array(kf_bad).tobytes() == bad0.tobytes()
    for f in ("pos", "ref_kf", "obs0", "n_obs", "bad", "ops", "pad"):
        assert P[f].tobytes() == P0[f].tobytes(), f
    if expect != 0:
        assert P.tobytes() == P0.tobytes()
        assert tracker_last_error(tracker).startswith("lba_mappoint_refresh: ")
        return None
    n = (over or {}).get("n_points", len(P))
    assert P[n:].tobytes() == P0[n:].tobytes()
    assert not (P[:n]["status"] == JUNK).any() and not (P[:n]["n"] == JUNK).any()
    assert not (P[:n]["best_obs"] == JUNK).any() and not (P[:n]["best_median"] == JUNK).any()
    return P


def identical(got, want, label):
    for i in range(len(want)):
        d = mo.diff_fields(got[i], want[i])
        assert d == [], (label, i, d, got[i], want[i])


def gen_reference(seed):
    if seed not in _ref:
        p = mc.gpu_problem(seed)
        _ref[seed] = (p, mo.refresh_batch(p.points, p.obs, p.K, p.kf_bad))
    return _ref[seed]


@pytest.mark.parametrize("name", mc.NAMES)
def test_case_identical_to_restatement(tracker, name):
    c = mc.case(name)
    got = device(tracker, c.points, c.obs, c.K, c.kf_bad, expect=c.refused)
    if not c.refused:
        identical(got, mc.reference(name), name)
        if c.check is not None:
            c.check(got)


@pytest.mark.parametrize("seed", mc.GPU_SEEDS)
def test_generated_batch_identical_to_restatement(tracker, seed):
    p, want = gen_reference(seed)
    assert (p.points["n_obs"] > 64).sum() >= 6 and len(p.points) > 1900
    identical(device(tracker, p.points, p.obs, p.K, p.kf_bad), want, ("gen", seed))


def test_untouched_outputs_come_back_byte_for_byte(tracker):
    p, want = gen_reference(0)
    got = device(tracker, p.points, p.obs, p.K, p.kf_bad)
    P = p.points
    quiet = got["status"] != MP_OK
    no_geom = quiet | ((P["ops"] & MP_NORMAL) == 0)
    no_desc = quiet | ((P["ops"] & MP_DESC) == 0) | (got["best_obs"] < 0)
    assert quiet.sum() > 0 and (no_geom & ~quiet).sum() > 0 and (no_desc & ~quiet).sum() > 0
    for f in ("normal", "min_distance", "max_distance"):
        assert got[f][no_geom].tobytes() == P[f][no_geom].tobytes(), f
    assert got["desc"][no_desc].tobytes() == P["desc"][no_desc].tobytes()
    assert (got["n"][no_geom] == 0).all() and (got["best_median"][no_desc] == -1).all()


def test_batch_equals_each_point_alone_and_a_second_run(tracker):
    p, _ = gen_reference(1)
    batch = device(tracker, p.points, p.obs, p.K, p.kf_bad)
    again = device(tracker, p.points, p.obs, p.K, p.kf_bad)
    assert batch.tobytes() == again.tobytes()
    classes = set()
    for i in range(len(p.points)):
        alone = p.points[i:i + 1].copy()
        alone["n"] = alone["best_obs"] = alone["best_median"] = alone["status"] = JUNK
        assert call(tracker, alone, p.obs, p.K, p.kf_bad) == 0
        assert alone.tobytes() == batch[i:i + 1].tobytes(), i
        classes.add(int(p.points[i]["n_obs"]) > 64)
    assert classes == {False, True}


def test_fresh_tracker_equals_one_that_ran_other_calls_before(tracker):
    import fuse_cases as fc
    from amc_lba.epipolar import make_epi_pairs
    from amc_lba.fuse import FUSE_KF, TH_KF, fuse
    prob = fc.gpu_problem(fc.GPU_SEEDS[0])
    fuse(tracker, prob.targets[:3], prob.points(np.arange(60)), [(k, 0, 60, FUSE_KF, TH_KF) for k in range(3)])
    pairs, kfs, ekfs, cams, feats, nid, nst, nf, _ = make_epi_pairs(1, 4, 150, 30, seed=9)
    tracker.match_epipolar(pairs, kfs, ekfs, cams, 4, feats, nid, nst, nf)
    p, _ = gen_reference(2)
    used = device(tracker, p.points, p.obs, p.K, p.kf_bad)
    fresh = Tracker(track_config())
    try:
        new = device(fresh, p.points, p.obs, p.K, p.kf_bad)
    finally:
        fresh.close()
    assert used.tobytes() == new.tobytes()


def test_profile_reports_the_three_kernels(tracker):
    p, _ = gen_reference(0)
    assert len(tracker.mappoint_refresh_kernel_ms(True)) == 3
    device(tracker, p.points, p.obs, p.K, p.kf_bad)
    ms = tracker.mappoint_refresh_kernel_ms(False)
    assert all(m > 0.0 for m in ms), ms


def test_null_kf_bad_means_none_is_bad(tracker):
    p, _ = gen_reference(0)
    P = p.points[:300]
    a = device(tracker, P, p.obs, p.K, None)
    b = device(tracker, P, p.obs, p.K, np.zeros(len(p.K.kfs), np.int32))
    assert a.tobytes() == b.tobytes()
    identical(a, mo.refresh_batch(P, p.obs, p.K, None), "kf_bad NULL")


# ---------------------------------------------------------------- the chain on one handle
def test_search_in_neighbors_chain_on_one_handle(tracker):
    """match_fuse -> fuse_walk on a ToyMap (both phases of SearchInNeighbors), refresh of the current keyframe's points
    from the map's observations, its descriptors against distinctive_descriptor, then the refreshed points through
    points_to_s3p into a second match_fuse, whose rows equal the restatement's rows on the restatement's points"""
    import fuse_oracle as fo
    import test_fuse_walk as tw
    from amc_lba.fuse import FUSE_KF, TH_KF, distinctive_descriptor, fuse, make_fuse_problem

    def rows_fn(targets, points, mode, th):
        return fuse(tracker, targets, points, [(i, 0, len(points), mode, th) for i in range(len(targets))])[1]

    prob = make_fuse_problem(n_kf=7, n_cam=4, n_feat=100, n_points=220, seed=2, duplicates=0.1)
    tally = tw.Tally()
    m, ms = tw.search_in_neighbors(prob, 0, list(range(1, 7)), tally, rows_fn=rows_fn)
    assert tw.same(m, ms)
    ids = sorted(m.points_of(0))
    assert len(ids) > 50
    K = keyframes_from_targets(prob.targets)
    P, obs = pack_points([obs_from_map(m.pts[i].obs) for i in ids], prob.pos[ids], [min(m.pts[i].obs) for i in ids])
    got = device(tracker, P, obs, K)
    want = mo.refresh_batch(P, obs, K)
    identical(got, want, "chain refresh")
    assert (got["n_obs"] > 4).sum() > 10
    for i, r in zip(ids, got):
        ds = [m.kfs[kf][2][f] for kf in sorted(m.pts[i].obs) for f in m.pts[i].obs[kf] if f != -1]
        assert r["desc"].tolist() == np.asarray(ds[distinctive_descriptor(ds)]).tolist(), i
    S3 = points_to_s3p(got)
    targets = prob.targets[1:4]
    _, rows = fuse(tracker, targets, S3, [(k, 0, len(S3), FUSE_KF, TH_KF) for k in range(3)])
    S3w = points_to_s3p(want)
    live = 0
    for k in range(3):
        w = fo.sequential(targets[k], S3w, FUSE_KF, TH_KF)[0]
        assert fo.same_rows(rows[k], w), k
        live += int((w["status"] <= 2).sum())
    assert live > 50


# ---------------------------------------------------------------- refusals
def test_refusals_write_nothing_and_leave_a_message(tracker):
    c = mc.case("shuffled_shared")
    P0, obs0, K = c.points, c.obs, c.K
    arg, lim = LBA_E_ARG, LBA_E_LIMIT

    def with_P(field, k, value):
        P = P0.copy()
        P[field][k] = value
        return dict(use_P=P)

    def with_obs(field, k, value):
        o = obs0.copy()
        o[field][k] = value
        return dict(use_obs=o)

    def with_K(array, field, k, value):
        import copy
        K2 = copy.copy(K)
        a = getattr(K, array).copy()
        a[field][k] = value
        setattr(K2, array, a)
        return dict(use_K=K2)

    def refuse(code, use_P=P0, use_obs=obs0, use_K=K, **over):
        device(tracker, use_P, use_obs, use_K, None, expect=code, over=over)

    live = int(np.flatnonzero(P0["n_obs"] > 0)[0])
    for name in ("points", "obs", "kfs", "ekfs", "cams", "feats", "prm"):        # null arrays, null params
        refuse(arg, **{name: None})
    for name in ("n_points", "n_obs", "n_kf", "n_cam_rows", "n_feats"):          # negative counts
        refuse(arg, **{name: -1})
    refuse(arg, n_cam=0)
    refuse(lim, n_cam=65)
    refuse(arg, n_obs=len(obs0) - 1)                                             # a point's range outside obs
    refuse(arg, **with_P("obs0", live, len(obs0)))
    refuse(arg, **with_P("obs0", live, -1))
    refuse(arg, **with_P("n_obs", live, -1))
    refuse(arg, **with_P("ref_kf", 0, len(K.kfs)))
    refuse(arg, **with_P("ref_kf", 0, -2))
    refuse(arg, **with_P("ops", 1, 0))
    refuse(arg, **with_P("ops", 1, 4))
    refuse(arg, **with_obs("kf", 3, len(K.kfs)))
    refuse(arg, **with_obs("kf", 3, -1))
    refuse(arg, **with_obs("feat", 3, int(K.ekfs["n_feat"][obs0["kf"][3]])))
    refuse(arg, **with_obs("feat", 3, -1))
    refuse(arg, **with_K("feats", "cam", 5, K.n_cam))
    refuse(arg, **with_K("feats", "cam", 5, -1))
    refuse(arg, **with_K("kfs", "cam0", 2, len(K.cams) - 1))
    refuse(arg, **with_K("ekfs", "feat0", 2, len(K.feats)))
    refuse(arg, **with_K("ekfs", "n_feat", 2, -1))
    refuse(arg, n_cam_rows=len(K.cams) - 1)
    refuse(arg, n_feats=len(K.feats) - 1)
    prm = LbaMpParams(float("nan"))
    refuse(arg, prm=ctypes.byref(prm))
    # more than LBA_MATCH_MAX_FEAT features in one camera of a keyframe
    import copy
    big = copy.copy(K)
    big.feats = np.zeros(MATCH_MAX_FEAT + 1, K.feats.dtype)
    big.ekfs = K.ekfs.copy()
    big.ekfs["feat0"], big.ekfs["n_feat"] = 0, 1
    big.ekfs["n_feat"][0] = MATCH_MAX_FEAT + 1
    o = obs0.copy()
    o["feat"] = 0
    refuse(lim, use_obs=o, use_K=big)
    # (an arena above 2 GB needs gigabytes of observations on the host: not exercised, as for the sibling calls)
    # the tracker is as usable as before
    identical(device(tracker, P0, obs0, K), mc.reference("shuffled_shared"), "after refusals")


def test_valid_edge_shapes(tracker):
    c = mc.case("n3")
    got = device(tracker, c.points[:0], c.obs, c.K)                              # n_points == 0
    assert len(got) == 0
    device(tracker, c.points, c.obs, c.K, over=dict(n_points=0))                 # (device() checks: nothing written)
    P = np.concatenate([mc.case("bad_point").points, mc.case("empty_list").points])
    P["obs0"] = 0
    got = device(tracker, P, c.obs, c.K)                                         # nothing to launch
    assert got["status"].tolist() == [1, 2]
    assert refresh(tracker, c.points.copy(), c.obs, c.K)["best_obs"].tolist() == [1]
