"""MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:611-700, :498-578) for a
batch of map points through the C ABI (lba_mappoint_refresh on an lba_tracker): the refresh local mapping runs point by
point after ProcessNewKeyFrame, after SearchInNeighbors' fuses and at the end of the bundle adjustments.  See
include/amc_lba.h for the contract and the quirks that are kept.

`refresh` is the call on numpy structured arrays (`refresh_raw` returns the status code instead of raising).  The
keyframe side is lba_match_epipolar's arrays; `keyframes_from_targets` makes them from amc_lba.fuse Targets.
`obs_from_map` flattens a map's observation dict into the ordered list, `pack_points` lays several lists out,
`points_to_s3p` turns refreshed points into the matchers' lba_s3p_point entries.  `make_mp_problem` is a seeded problem
over the scenes of amc_lba.fuse or amc_lba.epipolar."""
import ctypes

import numpy as np

from . import LbaError
from .abi import EPI_FEAT_DTYPE, EPI_KF_DTYPE, MP_OBS_DTYPE, MP_POINT_DTYPE, TRI_CAM_DTYPE, TRI_KF_DTYPE, ptr
from .match import _bind as _bind_match, tracker_last_error
from .sim3_project import S3P_POINT_DTYPE
from .track import Tracker, kernel_ms

MP_OK, MP_BAD, MP_EMPTY = 0, 1, 2
MP_STATUS_NAMES = ("OK", "BAD", "EMPTY")
MP_NORMAL, MP_DESC = 1, 2
MP_MAX_OBS = 1024
F = np.float32


class LbaMpParams(ctypes.Structure):
    _fields_ = [("scale_top", ctypes.c_float)]


def _bind():
    L = _bind_match()
    if not getattr(L, "_mp_bound", False):
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.lba_mappoint_refresh.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, vp, i32, vp,
                                           ctypes.POINTER(LbaMpParams)]
        L._mp_bound = True
    return L


class Keyframes:
    """lba_match_epipolar's keyframe side as this call reads it: kfs [n_kf] TRI_KF_DTYPE (cam0), ekfs [n_kf]
    EPI_KF_DTYPE (feat0, n_feat), cams TRI_CAM_DTYPE (Ow), feats EPI_FEAT_DTYPE (cam, scale, desc); n_cam; scale_top =
    mvScaleFactors[nLevels - 1]"""

    def __init__(self, kfs, ekfs, cams, n_cam, feats, scale_top):
        self.kfs = np.ascontiguousarray(kfs, TRI_KF_DTYPE)
        self.ekfs = np.ascontiguousarray(ekfs, EPI_KF_DTYPE)
        self.cams = np.ascontiguousarray(cams, TRI_CAM_DTYPE)
        self.feats = np.ascontiguousarray(feats, EPI_FEAT_DTYPE)
        self.n_cam, self.scale_top = int(n_cam), F(scale_top)

    def centre(self, kf, cam):
        """GetCameraCenter(cam) of keyframe kf, narrowed to float32 as the call narrows it"""
        return self.cams["Ow"][int(self.kfs["cam0"][kf]) + int(cam)].astype(F)

    def feature(self, kf, feat):
        return self.feats[int(self.ekfs["feat0"][kf]) + int(feat)]


def refresh_raw(tracker, points, obs, K, kf_bad=None, scale_top=None, params=True):
    """The call itself on the caller's arrays (points is written); returns the status code.  params=False passes NULL."""
    prm = LbaMpParams(float(K.scale_top if scale_top is None else scale_top)) if params else None
    bad = None if kf_bad is None else np.ascontiguousarray(kf_bad, np.int32)
    return _bind().lba_mappoint_refresh(
        tracker.h, ptr(points), len(points), ptr(obs), len(obs), ptr(K.kfs), ptr(K.ekfs), len(K.kfs), ptr(K.cams),
        len(K.cams), K.n_cam, ptr(K.feats), len(K.feats), None if bad is None else ptr(bad),
        ctypes.byref(prm) if prm is not None else None)


def refresh(tracker, points, obs, kfs, ekfs=None, cams=None, n_cam=None, feats=None, kf_bad=None, scale_top=None):
    """Every point of `points` (MP_POINT_DTYPE, modified in place when it has the right dtype and layout, copied
    otherwise) on its range of `obs` (MP_OBS_DTYPE).  `kfs` is a Keyframes, or lba_match_epipolar's four arrays are
    given one by one with n_cam and scale_top.  Returns the points."""
    K = kfs if isinstance(kfs, Keyframes) else Keyframes(kfs, ekfs, cams, n_cam, feats, scale_top)
    points = np.ascontiguousarray(points, MP_POINT_DTYPE)
    obs = np.ascontiguousarray(obs, MP_OBS_DTYPE)
    rc = refresh_raw(tracker, points, obs, K, kf_bad, scale_top)
    if rc != 0:
        raise LbaError(rc, "lba_mappoint_refresh failed: " + tracker_last_error(tracker))
    return points


def refresh_kernel_ms(tracker, on=True):
    """track.kernel_ms for lba_mappoint_refresh's launches (k_mp_geom, k_mp_desc_wave, k_mp_desc_block)"""
    return kernel_ms(tracker, "lba_mappoint_refresh_profile", on, 3)


Tracker.mappoint_refresh = refresh
Tracker.mappoint_refresh_kernel_ms = refresh_kernel_ms


# ---------------------------------------------------------------- packers
def obs_from_map(observations, order=None, index=None):
    """A point's mObservations as the ordered list: `observations` {keyframe: [keypoint index per camera, -1: none]};
    `order`: the keyframes in the map's iteration order (default: sorted keys); `index`: keyframe -> its row of the
    keyframe arrays (default: the key itself).  Keyframes in the given order, cameras ascending.  MP_OBS_DTYPE."""
    order = sorted(observations) if order is None else [k for k in order if k in observations]
    rows = [((k if index is None else index[k]), i) for k in order for i in observations[k] if i != -1]
    out = np.zeros(len(rows), MP_OBS_DTYPE)
    if rows:
        out["kf"], out["feat"] = np.array(rows, np.int64).T
    return out


def pack_points(lists, pos, ref_kf, ops=3, bad=0, normal=None, min_distance=None, max_distance=None, desc=None):
    """Points one behind the other: `lists` per point its MP_OBS_DTYPE list; the other arguments per point or one for
    all.  Returns (points MP_POINT_DTYPE, obs MP_OBS_DTYPE)."""
    n = len(lists)
    P = np.zeros(n, MP_POINT_DTYPE)
    P["pos"] = np.asarray(pos, F).reshape(n, 3)
    P["ref_kf"], P["ops"], P["bad"] = ref_kf, ops, bad
    P["n_obs"] = [len(lst) for lst in lists]
    P["obs0"] = np.concatenate([[0], np.cumsum(P["n_obs"])[:-1]]) if n else 0
    for name, v in (("normal", normal), ("min_distance", min_distance), ("max_distance", max_distance), ("desc", desc)):
        if v is not None:
            P[name] = v
    obs = np.concatenate([np.asarray(lst, MP_OBS_DTYPE) for lst in lists]) if n else np.zeros(0, MP_OBS_DTYPE)
    return P, obs.astype(MP_OBS_DTYPE)


def points_to_s3p(points, skip=None):
    """lba_s3p_point entries of refreshed points: min_dist = 0.8f * min_distance and max_dist = 1.2f * max_distance
    (GetMinDistanceInvariance / GetMaxDistanceInvariance), the raw max_distance, normal, desc; skip = bad unless given"""
    S = np.zeros(len(points), S3P_POINT_DTYPE)
    S["pos"], S["normal"], S["desc"] = points["pos"], points["normal"], points["desc"]
    S["min_dist"] = F(0.8) * points["min_distance"].astype(F)
    S["max_dist"] = F(1.2) * points["max_distance"].astype(F)
    S["max_distance"] = points["max_distance"]
    S["skip"] = points["bad"] != 0 if skip is None else skip
    return S


def keyframes_from_targets(targets):
    """The keyframe arrays of amc_lba.fuse Targets (all with the same number of cameras and the same pyramid): the
    centres are the targets' float `ow` widened, a feature's scale is sf[octave]"""
    n_cam = targets[0].n_cam
    kfs, ekfs = np.zeros(len(targets), TRI_KF_DTYPE), np.zeros(len(targets), EPI_KF_DTYPE)
    cams = np.zeros(len(targets) * n_cam, TRI_CAM_DTYPE)
    feats, at = [], 0
    for k, t in enumerate(targets):
        assert t.n_cam == n_cam
        kfs[k]["cam0"] = k * n_cam
        cams["Ow"][k * n_cam:(k + 1) * n_cam] = t.fcams["ow"].astype(np.float64)
        f = np.zeros(len(t.feats), EPI_FEAT_DTYPE)
        for name in ("x", "y", "angle", "u_right", "cam", "desc"):
            f[name] = t.feats[name]
        f["scale"] = t.sf[t.feats["octave"]]
        f["sigma2"] = f["scale"] * f["scale"]
        ekfs[k]["feat0"], ekfs[k]["n_feat"] = at, len(f)
        at += len(f)
        feats.append(f)
    return Keyframes(kfs, ekfs, cams, n_cam, np.concatenate(feats) if feats else np.zeros(0, EPI_FEAT_DTYPE),
                     targets[0].sf[-1])


def synthetic_keyframes(n_kf, n_cam, n_feat, rng, n_levels=8, scale=1.2, spread=2.0):
    """Keyframe arrays without a scene: centres `spread` around the origin (float values), `n_feat` keypoints per
    camera in camera-major order with random octaves and descriptors"""
    from .match import scale_factors
    sf = scale_factors(n_levels, scale)
    kfs, ekfs = np.zeros(n_kf, TRI_KF_DTYPE), np.zeros(n_kf, EPI_KF_DTYPE)
    cams = np.zeros(n_kf * n_cam, TRI_CAM_DTYPE)
    kfs["cam0"] = np.arange(n_kf) * n_cam
    cams["Ow"] = rng.normal(0, spread, (n_kf * n_cam, 3)).astype(F).astype(np.float64)
    feats = np.zeros(n_kf * n_cam * n_feat, EPI_FEAT_DTYPE)
    feats["cam"] = np.tile(np.repeat(np.arange(n_cam), n_feat), n_kf)
    feats["scale"] = sf[rng.integers(0, n_levels, len(feats))]
    feats["desc"] = rng.integers(0, 2 ** 32, size=(len(feats), 8), dtype=np.uint64).astype(np.uint32)
    feats["u_right"] = -1.0
    ekfs["feat0"], ekfs["n_feat"] = np.arange(n_kf) * n_cam * n_feat, n_cam * n_feat
    return Keyframes(kfs, ekfs, cams, n_cam, feats, sf[-1])


# ---------------------------------------------------------------- a seeded problem
class MpProblem:
    """K: Keyframes; points / obs: the packed batch; kf_bad [n_kf] int32"""

    def __init__(self, K, points, obs, kf_bad):
        self.K, self.points, self.obs, self.kf_bad = K, points, obs, np.asarray(kf_bad, np.int32)


def _junk_fields(P, rng):
    """what a point holds before its refresh: anything"""
    n = len(P)
    P["normal"] = rng.normal(0, 1, (n, 3))
    P["min_distance"], P["max_distance"] = rng.uniform(0.1, 2.0, n), rng.uniform(5.0, 50.0, n)
    P["desc"] = rng.integers(0, 2 ** 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)


def make_mp_problem(seed=0, scene="fuse", n_kf=8, n_cam=4, n_feat=80, n_points=200, long_tracks=0, long_obs=(65, 200),
                    bad_kf=0.15, bad_point=0.03, no_ref=0.04, ops=(3, 3, 3, 1, 2)):
    """A seeded batch.  scene "fuse": the keyframes, map points and observations of amc_lba.fuse.make_fuse_problem (a
    point holds one feature per (keyframe, camera), several cameras of one keyframe near a seam; points nobody observes
    come out EMPTY); scene "epipolar": the keyframes of amc_lba.epipolar.make_epi_pairs, a point per keypoint of the
    current keyframe, observed there and by its partners.  A share `bad_kf` of the keyframes is bad, `bad_point` of the
    points; the reference keyframe is an observing keyframe, or -1 with probability `no_ref`; `ops` is drawn from the
    given tuple; the five in / out fields start as junk.  `long_tracks` further points observe 65 .. 200 random keypoints
    (one per (keyframe, camera) while there are enough, then further rounds), so both size classes occur."""
    rng = np.random.default_rng([seed, 0x3A9])
    if scene == "fuse":
        from .fuse import make_fuse_problem
        prob = make_fuse_problem(n_kf=n_kf, n_cam=n_cam, n_feat=n_feat, n_points=n_points, seed=seed)
        K = keyframes_from_targets(prob.targets)
        by_id = [dict() for _ in range(prob.n_ids)]
        for pid, kf, f in prob.obs:
            idx = by_id[int(pid)].setdefault(int(kf), [-1] * n_cam)
            idx[int(prob.targets[kf].feats["cam"][f])] = int(f)
        lists = [obs_from_map(o) for o in by_id]
        pos = prob.pos
    elif scene == "epipolar":
        from .epipolar import make_epi_pairs
        n_pairs = n_kf - 1
        _, kfs, ekfs, cams, feats, _, _, _, truth = make_epi_pairs(n_pairs, n_cam, n_feat, 20, seed=seed)
        K = Keyframes(kfs, ekfs, cams, n_cam, feats, truth["kf"][0]["scale_factors"][-1])
        lists = []
        for i in range(n_cam * n_feat):
            rows = [(0, i)] + [(p + 1, int(truth["partner"][p][i])) for p in range(n_pairs) if truth["partner"][p][i] >= 0]
            lst = np.zeros(len(rows), MP_OBS_DTYPE)
            lst["kf"], lst["feat"] = np.array(rows, np.int64).T
            lists.append(lst)
        pos = truth["X"].astype(F)
    else:
        raise ValueError(scene)
    pos = [np.asarray(p, F) for p in pos]
    n_kf_all, per_kf = len(K.kfs), K.ekfs["n_feat"]
    for _ in range(long_tracks):
        n = int(rng.integers(long_obs[0], long_obs[1] + 1))
        rows = []
        while len(rows) < n:                       # rounds over the (keyframe, camera) slots in the map's order
            for k in range(n_kf_all):
                fk = K.feats[int(K.ekfs["feat0"][k]):int(K.ekfs["feat0"][k]) + int(per_kf[k])]
                for c in range(n_cam):
                    cand = np.flatnonzero(fk["cam"] == c)
                    if len(cand) and len(rows) < n and rng.random() < 0.8:
                        rows.append((k, int(rng.choice(cand))))
        lst = np.zeros(n, MP_OBS_DTYPE)
        lst["kf"], lst["feat"] = np.array(rows, np.int64).T
        lists.append(lst)
        pos.append(rng.normal(0, 6.0, 3).astype(F))
    n = len(lists)
    ref = np.full(n, -1, np.int64)
    for p, lst in enumerate(lists):
        if len(lst) and rng.random() >= no_ref:
            ref[p] = lst["kf"][int(rng.integers(0, len(lst)))]
    P, obs = pack_points(lists, np.stack(pos) if n else np.zeros((0, 3), F), ref,
                         ops=rng.choice(np.asarray(ops), n), bad=rng.random(n) < bad_point)
    _junk_fields(P, rng)
    P["n"] = P["best_obs"] = P["best_median"] = P["status"] = -99
    return MpProblem(K, P, obs, rng.random(n_kf_all) < bad_kf)
