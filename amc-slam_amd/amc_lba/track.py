"""Tracking-side pose optimisation (Optimizer::PoseGPOptimizationFromeLastFrame, src/Optimizer.cc:369-686)
through the C ABI (lba_tracker_*, lba_track): a batch of frames, one GPU workgroup each, one launch.
The step before it in Tracking::TrackLocalMap, MCRansac's velocity hypotheses (src/Tracking.cc:1939-2002, one
Optimizer::OptimizeVel each), is `Tracker.vel_ransac` / `mc_ransac` (lba_track_vel_ransac: one wave per hypothesis).

`make_track_frames` cuts synthetic tracking problems out of a local-BA window: frame k's
observations (the asynchronous cameras' GP edges between k-1 and k, the reference camera's mono /
stereo edges) against fixed map points, the previous frame fixed or free.
"""
import ctypes

import numpy as np

from . import LbaError, lib
from .abi import CAM_DTYPE, KF_DTYPE, MONO, MONO_GP, STEREO, LbaConfig, make_config, ptr

TRACK_OBS_DTYPE = np.dtype([
    ("kind", "<i4"), ("cam", "<i4"), ("outlier", "<i4"), ("close", "<i4"),
    ("t", "<f8"), ("z", "<f8", (3,)), ("w", "<f8"), ("Xw", "<f8", (3,)),
], align=True)
TRACK_FRAME_DTYPE = np.dtype([
    ("prev", KF_DTYPE), ("cur", KF_DTYPE), ("obs0", "<i4"), ("n_obs", "<i4"), ("n_good", "<i4"),
    ("iterations", "<i4"),
], align=True)
assert TRACK_OBS_DTYPE.itemsize == 80
assert TRACK_FRAME_DTYPE.itemsize == 272
VEL_SET = 3
VEL_OBS_DTYPE = np.dtype([
    ("cam", "<i4"), ("inlier", "<i4"), ("dt", "<f8"), ("z", "<f8", (2,)), ("w", "<f8"), ("Xw", "<f8", (3,)),
], align=True)
VEL_FRAME_DTYPE = np.dtype([
    ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("vel", "<f8", (6,)), ("obs0", "<i4"), ("n_obs", "<i4"),
    ("hyp0", "<i4"), ("n_hyp", "<i4"), ("best_hyp", "<i4"), ("n_inliers", "<i4"),
], align=True)
assert VEL_OBS_DTYPE.itemsize == 64
assert VEL_FRAME_DTYPE.itemsize == 128


class LbaVelParams(ctypes.Structure):
    """lba_vel_params; the defaults are OptimizeVel's (threshold 2.0, rk->setDelta(5.991), optimize(40))."""
    _fields_ = [("threshold", ctypes.c_double), ("huber_delta", ctypes.c_double), ("iterations", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


def vel_params(threshold=2.0, huber_delta=5.991, iterations=40):
    return LbaVelParams(threshold, huber_delta, iterations, 0)


def _bind():
    L = lib()
    if not getattr(L, "_track_bound", False):
        vp = ctypes.c_void_p
        L.lba_tracker_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(LbaConfig)]
        L.lba_tracker_destroy.argtypes = [vp]
        L.lba_tracker_destroy.restype = None
        L.lba_track.argtypes = [vp, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, ctypes.c_int32]
        L.lba_track_vel_ransac.argtypes = [vp, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, ctypes.c_int32,
                                           ctypes.POINTER(LbaVelParams), vp, ctypes.c_int32, vp, vp, vp]
        L._track_bound = True
    return L


def kernel_ms(tracker, profile, on, n=1):
    """Measurement: switch the event bracket of one entry point (`profile`: its lba_*_profile function) on or off;
    returns the `n` kernel times of its last bracketed call in milliseconds (-1 before the first), a float for n = 1."""
    fn = getattr(_bind(), profile)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_double)]
    ms = (ctypes.c_double * n)(*[-1.0] * n)
    rc = fn(tracker.h, int(bool(on)), ms)
    if rc != 0:
        raise LbaError(rc, profile + " failed")
    return ms[0] if n == 1 else tuple(ms)


def track_config(**over):
    """The reference's tracking optimiser: Huber deltas as LocalGPBA, no user lambda
    (computeLambdaInit, src/Optimizer.cc:379-381), g2o stop rules."""
    kw = dict(lambda_init=0.0)
    kw.update(over)
    return make_config(**kw)


class Tracker:
    def __init__(self, cfg=None, device=0, **over):
        L = _bind()
        self.cfg = cfg if cfg is not None else track_config(device=device, **over)
        self.h = ctypes.c_void_p()
        rc = L.lba_tracker_create(ctypes.byref(self.h), ctypes.byref(self.cfg))
        if rc != 0:
            raise LbaError(rc, "lba_tracker_create failed")

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            _bind().lba_tracker_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        self.close()

    def track(self, frames, obs, cams):
        """Optimises the frames in place (cur, n_good, iterations) and the observations' outlier flags."""
        frames = np.ascontiguousarray(frames, TRACK_FRAME_DTYPE)
        obs = np.ascontiguousarray(obs, TRACK_OBS_DTYPE)
        cams = np.ascontiguousarray(cams, CAM_DTYPE)
        rc = _bind().lba_track(self.h, ptr(frames), len(frames), ptr(obs), len(obs), ptr(cams), len(cams))
        if rc != 0:
            raise LbaError(rc, "lba_track failed")
        return frames, obs

    def vel_ransac(self, frames, obs, samples, cams, params=None, per_hyp=True):
        """MCRansac's hypotheses for a batch of frames (lba_track_vel_ransac): `samples` [n_hyp, 3] frame-local
        observation indices, `params` an LbaVelParams (vel_params(...)) or None for OptimizeVel's defaults.
        Writes the frames (vel, best_hyp, n_inliers) and the observations' inlier flags in place and returns
        (frames, obs, (hyp_vel [n_hyp, 6], hyp_inliers, hyp_iterations)); per_hyp=False passes NULL for the
        per-hypothesis arrays and returns None in their place."""
        frames = np.ascontiguousarray(frames, VEL_FRAME_DTYPE)
        obs = np.ascontiguousarray(obs, VEL_OBS_DTYPE)
        samples = np.ascontiguousarray(samples, np.int32).reshape(-1, VEL_SET)
        cams = np.ascontiguousarray(cams, CAM_DTYPE)
        n_hyp = len(samples)
        hyp = (np.zeros((n_hyp, 6)), np.zeros(n_hyp, np.int32), np.zeros(n_hyp, np.int32)) if per_hyp else None
        rc = _bind().lba_track_vel_ransac(self.h, ptr(frames), len(frames), ptr(obs), len(obs), ptr(samples), n_hyp,
                                          ctypes.byref(params) if params is not None else None, ptr(cams), len(cams),
                                          *([ptr(a) for a in hyp] if per_hyp else [None] * 3))
        if rc != 0:
            raise LbaError(rc, "lba_track_vel_ransac failed")
        return frames, obs, hyp

    def triangulate(self, pairs, rows, kfs, cams, n_cam, params=None):
        """LocalMapping::CreateNewMapPoints' triangulation for a batch of (keyframe, neighbour) pairs
        (lba_triangulate; amc_lba.triangulate has the dtypes, the row construction and the generator)."""
        from .triangulate import triangulate
        return triangulate(self, pairs, rows, kfs, cams, n_cam, params)

    def match_epipolar(self, pairs, kfs, ekfs, cams, n_cam, feats, node_id, node_start, node_feat, params=None, out=None):
        """ORBmatcher::SearchForTriangulation for a batch of (keyframe, neighbour) pairs, the matcher in front of
        `triangulate` (lba_match_epipolar; amc_lba.epipolar has the dtypes, the caller's side and the generator)."""
        from .epipolar import match_epipolar
        return match_epipolar(self, pairs, kfs, ekfs, cams, n_cam, feats, node_id, node_start, node_feat, params, out)

    def match_epipolar_kernel_ms(self, on=True):
        """kernel_ms for lba_match_epipolar's two launches: (k_epi_tables, k_epi_match)"""
        return kernel_ms(self, "lba_match_epipolar_profile", on, 2)

    def match_bow(self, pairs, ekfs, feats, node_id, node_start, node_feat, params=None, out=None):
        """ORBmatcher::SearchByBoW for a batch of pairs, the matcher in front of `sim3_ransac` in loop closing and of
        the pose optimisation in TrackReferenceKeyFrame (lba_match_bow; amc_lba.bow has the dtypes, the caller's side
        and the generator).  The keyframe arrays are `match_epipolar`'s."""
        from .bow import match_bow
        return match_bow(self, pairs, ekfs, feats, node_id, node_start, node_feat, params, out)

    def match_bow_kernel_ms(self, on=True):
        """kernel_ms for lba_match_bow's launch (k_bow_match)"""
        return kernel_ms(self, "lba_match_bow_profile", on)


def mc_ransac(tracker, frames, obs, samples, cams, min_match=30, outlier=None, params=None):
    """Tracking::MCRansac for a batch of frames with the caller's triples: the hypotheses on the GPU, then the
    caller's rule (src/Tracking.cc:1987-2001) per frame: fewer than `min_match` inliers for the best hypothesis
    returns 0 and leaves the frame's mvbOutlier alone, otherwise its non-inliers become outliers and the count
    is returned.  `outlier`: mvbOutlier per observation on entry (None: all false).
    Returns (counts [n_frames], outlier [n_obs] bool, frames, obs)."""
    frames, obs, _ = tracker.vel_ransac(frames, obs, samples, cams, params=params, per_hyp=False)
    out = np.zeros(len(obs), bool) if outlier is None else np.array(outlier, bool)
    ret = np.zeros(len(frames), np.int32)
    for f, F in enumerate(frames):
        if F["n_inliers"] < min_match:
            continue
        rows = slice(int(F["obs0"]), int(F["obs0"] + F["n_obs"]))
        out[rows] |= obs["inlier"][rows] == 0
        ret[f] = F["n_inliers"]
    return ret, out, frames, obs


def _se3_exp(xi):
    """exp of a twist [translation; rotation] as (R, t)."""
    from .synth import _expso3
    xi = np.asarray(xi, float)
    w = xi[3:]
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-9:
        V = np.eye(3) + 0.5 * K
    else:
        V = np.eye(3) + (1 - np.cos(th)) / th**2 * K + (th - np.sin(th)) / th**3 * (K @ K)
    return _expso3(w), V @ xi[:3]


def make_vel_frames(n_frames=1, n_obs=200, n_cam=4, n_hyp=23, noise=0.7, outlier_frac=0.1, seed=0, vel_true=None,
                    start_sigma=0.05, dts=None, n_octaves=8):
    """Synthetic MCRansac inputs: per frame a last-frame pose T (float values, like GetPoseW()), a true body
    velocity, camera c observed `dts[c]` seconds after the last frame (default 0.08 .. 0.11 s), `n_obs` map points
    seen from the pose T exp(v dt) of their camera with `noise` pixels of Gaussian error, a share `outlier_frac`
    of gross outliers (20 .. 100 px off), octave weights 1 / 1.2^(2k), the start velocity `start_sigma` off the
    truth (float values, like GetVelocity()), and `n_hyp` seeded triples of distinct observations.
    Returns (frames, obs, samples [n_frames * n_hyp, 3], cams, truth) with truth = {"vel": [n_frames, 6],
    "gross": bool [n_frames * n_obs]}."""
    from .synth import _f32, _rotz, quat_to_rot, rot_to_quat
    rng = np.random.default_rng(seed)
    Rbc0 = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    yaws = [np.pi / 2, np.pi, -np.pi / 2]
    cam_yaw = [yaws[c % 3] for c in range(n_cam - 1)] + [0.0]
    cams = np.zeros(n_cam, CAM_DTYPE)
    Rbc, tbc = np.zeros((n_cam, 3, 3)), np.zeros((n_cam, 3))
    for c in range(n_cam):
        q = _f32(rot_to_quat(_rotz(cam_yaw[c]) @ Rbc0))
        Rbc[c] = quat_to_rot(q)
        tbc[c] = _f32([0.5 * np.cos(cam_yaw[c]), 0.5 * np.sin(cam_yaw[c]), 0.2])
        cams[c]["q"], cams[c]["t"] = q, tbc[c]
        cams[c]["fx"], cams[c]["fy"], cams[c]["cx"], cams[c]["cy"] = 500.0, 500.0, 480.0, 300.0
        cams[c]["rbc_ini"] = q
        cams[c]["rbc_info"] = (0.2 * np.eye(3)).ravel()
    dts = np.linspace(0.08, 0.11, n_cam) if dts is None else np.broadcast_to(np.asarray(dts, float), (n_cam,))
    frames = np.zeros(n_frames, VEL_FRAME_DTYPE)
    obs = np.zeros(n_frames * n_obs, VEL_OBS_DTYPE)
    samples = np.zeros((n_frames * n_hyp, VEL_SET), np.int32)
    truth = {"vel": np.zeros((n_frames, 6)), "gross": np.zeros(n_frames * n_obs, bool)}
    for f in range(n_frames):
        q = _f32(rot_to_quat(_rotz(rng.uniform(-np.pi, np.pi))))
        R, t = quat_to_rot(q / np.linalg.norm(q)), _f32(rng.uniform(-20, 20, 3))
        v = (np.array([4.0, 0.0, 0.0, 0.0, 0.0, 0.15]) + rng.normal(0, [0.3, 0.1, 0.05, 0.01, 0.01, 0.05])
             if vel_true is None else np.asarray(vel_true, float))
        truth["vel"][f] = v
        F = frames[f]
        F["q"], F["t"] = q, t
        F["vel"] = _f32(v + rng.normal(0, start_sigma, 6)) if start_sigma is not None else 0.0
        F["obs0"], F["n_obs"], F["hyp0"], F["n_hyp"] = f * n_obs, n_obs, f * n_hyp, n_hyp
        o = obs[f * n_obs:(f + 1) * n_obs]
        cam = rng.integers(0, n_cam, n_obs)
        o["cam"], o["dt"] = cam, dts[cam]
        o["w"] = 1.0 / 1.2 ** (2 * rng.integers(0, n_octaves, n_obs))
        gross = rng.random(n_obs) < outlier_frac
        truth["gross"][f * n_obs:(f + 1) * n_obs] = gross
        for c in range(n_cam):
            rows = np.nonzero(cam == c)[0]
            Rm, tm = _se3_exp(v * dts[c])
            Rwc, twc = R @ Rm @ Rbc[c], R @ (Rm @ tbc[c] + tm) + t       # T exp(v dt) Tbc
            uv = np.stack([rng.uniform(20, 940, rows.size), rng.uniform(20, 580, rows.size)], axis=1)
            depth = rng.uniform(4.0, 30.0, rows.size)
            Xc = np.stack([(uv[:, 0] - 480.0) / 500.0 * depth, (uv[:, 1] - 300.0) / 500.0 * depth, depth], axis=1)
            Xw = _f32(Xc @ Rwc.T + twc)
            Xc = (Xw - twc) @ Rwc                                          # the float point, re-projected
            z = np.stack([500.0 * Xc[:, 0] / Xc[:, 2] + 480.0, 500.0 * Xc[:, 1] / Xc[:, 2] + 300.0], axis=1)
            z += rng.normal(0, noise, z.shape)
            ang, far = rng.uniform(0, 2 * np.pi, rows.size), rng.uniform(20, 100, rows.size)
            z += np.where(gross[rows, None], np.stack([far * np.cos(ang), far * np.sin(ang)], axis=1), 0.0)
            o["Xw"][rows], o["z"][rows] = Xw, _f32(z)
        if n_hyp:
            samples[f * n_hyp:(f + 1) * n_hyp] = [rng.choice(n_obs, VEL_SET, replace=False) for _ in range(n_hyp)]
    return frames, obs, samples, cams, truth


def make_track_frames(win, ks, fix_prev=True, outlier_init=0.05, close_frac=0.2, seed=0, point_noise=0.02,
                      sigma_t=0.03, sigma_r=0.3, sigma_v=0.05):
    """One tracking problem per KF index k in `ks` of an unperturbed window `win`
    (make_window(..., perturb=False)), k >= 1: prev = KF k-1 at its true state, cur = KF k with its
    pose / velocity perturbed (the motion-model prediction the tracker starts from), the observations
    of KF k with their points fixed at the true positions plus `point_noise` (m), rounded to float like
    GetWorldPos()."""
    from .synth import _expso3, quat_to_rot, rot_to_quat
    rng = np.random.default_rng(seed)
    o = win.obs
    frames = np.zeros(len(ks), TRACK_FRAME_DTYPE)
    rows = []
    for f, k in enumerate(ks):
        sel = np.nonzero(o["kf_b"] == k)[0]
        frames[f]["prev"] = win.kfs[k - 1]
        frames[f]["prev"]["fixed"] = int(fix_prev)
        frames[f]["cur"] = win.kfs[k]
        frames[f]["cur"]["fixed"] = 0
        R = quat_to_rot(win.kfs[k]["q"]) @ _expso3(rng.normal(0, np.deg2rad(sigma_r), 3))
        frames[f]["cur"]["q"] = rot_to_quat(R).astype(np.float32)
        frames[f]["cur"]["t"] = (win.kfs[k]["t"] + rng.normal(0, sigma_t, 3)).astype(np.float32)
        frames[f]["cur"]["vel"] = (win.kfs[k]["vel"] + rng.normal(0, sigma_v, 6)).astype(np.float32)
        frames[f]["obs0"] = len(rows)
        frames[f]["n_obs"] = sel.size
        for i in sel:
            rows.append(i)
    rows = np.array(rows, np.int64)
    obs = np.zeros(rows.size, TRACK_OBS_DTYPE)
    src = o[rows]
    kind = src["kind"].copy()
    kind[kind == 1] = MONO_GP   # (no stereo GP edge in the tracking graph)
    obs["kind"] = kind
    obs["cam"] = src["cam"]
    obs["t"] = src["t"]
    obs["z"] = src["z"]
    obs["w"] = src["w"]
    X = win.truth_lm[src["lm"]] + rng.normal(0, point_noise, (rows.size, 3))
    obs["Xw"] = X.astype(np.float32).astype(np.float64)
    obs["outlier"] = rng.random(rows.size) < outlier_init
    obs["close"] = rng.random(rows.size) < close_frac
    return frames, obs
