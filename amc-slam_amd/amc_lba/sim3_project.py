"""The Sim3 ORBmatcher::SearchByProjection (src/ORBmatcher.cc:423-548 and :550-685) through the C ABI
(lba_match_sim3_project on an lba_tracker): ONE keyframe with its grid, a batch of hypotheses (searches), each with its
own Sbw and its own list of points.  The pose chain, the projection with its gates, PredictScale, the gather and the
greedy resolve all run on the device; see include/amc_lba.h for the contract and the quirks that are kept.

`sim3_project` is the call on packed arrays; `Keyframe` holds the shared side and `Hypothesis` one search.  The caller's
side of LoopClosing.cc on plain arrays: `points_from_keyframes` (the spMapPoints dedup of :554-572 / :778-794),
`matched_kf` (the second overload's vpMatchedKF) and `scw_from_pair` (gScw = gScm * gSmw, :576-579).
`make_s3p_problem` makes a seeded keyframe and hypotheses whose points reproject into it.
"""
import ctypes

import numpy as np

from . import LbaError
from .abi import MATCH_CAM_DTYPE, MATCH_FEAT_DTYPE, ptr
from .match import (build_grid, flip_bits, match_cams, scale_factors, tracker_last_error,
                    _bind as _bind_match)
from .track import Tracker, kernel_ms

(S3P_OK, S3P_NO_CAND, S3P_TOO_FAR, S3P_SKIPPED, S3P_BEHIND, S3P_OUT_OF_IMAGE, S3P_DIST, S3P_ANGLE,
 S3P_NO_PREV) = range(9)
S3P_STATUS_NAMES = ("OK", "NO_CAND", "TOO_FAR", "SKIPPED", "BEHIND", "OUT_OF_IMAGE", "DIST", "ANGLE", "NO_PREV")
S3P_MAX_CAM = 64
TH_LOW = 50
CALL_SITES = ((8, 1.5), (5, 1.0), (3, 1.5))        # (th, ratioHamming) of LoopClosing.cc:586, :608, :800
F = np.float32

S3P_KF_DTYPE = np.dtype([
    ("stamp", "<f8"), ("stamp_prev", "<f8"), ("q", "<f4", (4,)), ("t", "<f4", (3,)), ("q_prev", "<f4", (4,)),
    ("t_prev", "<f4", (3,)), ("v", "<f4", (6,)), ("v_prev", "<f4", (6,)), ("log_scale_factor", "<f4"),
    ("has_prev", "<i4"), ("n_levels", "<i4"), ("n_cam", "<i4"),
], align=True)
S3P_CAM_DTYPE = np.dtype([
    ("stamp", "<f8"), ("q_bc", "<f4", (4,)), ("t_bc", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
    ("cy", "<f4"), ("min_x", "<f4"), ("max_x", "<f4"), ("min_y", "<f4"), ("max_y", "<f4"), ("ow", "<f4", (3,)),
    ("pad", "<i4", (2,)),
], align=True)
S3P_POINT_DTYPE = np.dtype([
    ("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_dist", "<f4"), ("max_dist", "<f4"), ("max_distance", "<f4"),
    ("skip", "<i4"), ("desc", "<u4", (8,)), ("pad", "<i4", (2,)),
], align=True)
S3P_SEARCH_DTYPE = np.dtype([
    ("q", "<f4", (4,)), ("t", "<f4", (3,)), ("s", "<f4"), ("point0", "<i4"), ("n_points", "<i4"), ("taken0", "<i4"),
    ("row0", "<i4"), ("featpt0", "<i4"), ("pose0", "<i4"), ("n_matches", "<i4"), ("pad", "<i4"),
], align=True)
S3P_ROW_DTYPE = np.dtype([
    ("status", "<i4"), ("feat", "<i4"), ("best_dist", "<i4"), ("level", "<i4"), ("x", "<f4"), ("y", "<f4"),
    ("radius", "<f4"), ("pad", "<i4"),
], align=True)
S3P_POSE_DTYPE = np.dtype([
    ("tcw_d", "<f8", (12,)), ("tcw", "<f4", (12,)), ("rounds", "<i4"), ("pad", "<i4"),
], align=True)
assert S3P_KF_DTYPE.itemsize == 136 and S3P_CAM_DTYPE.itemsize == 88 and S3P_POINT_DTYPE.itemsize == 80
assert S3P_SEARCH_DTYPE.itemsize == 64 and S3P_ROW_DTYPE.itemsize == 32 and S3P_POSE_DTYPE.itemsize == 152


class LbaS3pParams(ctypes.Structure):
    """lba_s3p_params"""
    _fields_ = [("th", ctypes.c_int32), ("th_low", ctypes.c_int32), ("ratio_hamming", ctypes.c_float),
                ("proj_form", ctypes.c_int32)]


def s3p_params(th=8, ratio_hamming=1.5, proj_form=1, th_low=TH_LOW):
    return LbaS3pParams(int(th), int(th_low), float(ratio_hamming), int(proj_form))


def _bind():
    L = _bind_match()
    if not getattr(L, "_s3p_bound", False):
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.lba_match_sim3_project.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32,
                                             vp, i32, vp, i32, vp, i32, ctypes.POINTER(LbaS3pParams)]
        L._s3p_bound = True
    return L


class Keyframe:
    """The shared side: kf [1] S3P_KF_DTYPE, kcams [n_cam] S3P_CAM_DTYPE, gcams [n_cam] MATCH_CAM_DTYPE, sf [n_levels],
    cell_start, cell_feat (amc_lba.match.build_grid), feats MATCH_FEAT_DTYPE."""

    def __init__(self, kf, kcams, gcams, sf, cell_start, cell_feat, feats):
        self.kf = np.ascontiguousarray(kf, S3P_KF_DTYPE).reshape(1)
        self.kcams = np.ascontiguousarray(kcams, S3P_CAM_DTYPE)
        self.gcams = np.ascontiguousarray(gcams, MATCH_CAM_DTYPE)
        self.sf = np.ascontiguousarray(sf, F)
        self.cell_start = np.ascontiguousarray(cell_start, np.int32)
        self.cell_feat = np.ascontiguousarray(cell_feat, np.int32)
        self.feats = np.ascontiguousarray(feats, MATCH_FEAT_DTYPE)

    @property
    def n_cam(self):
        return int(self.kf["n_cam"][0])

    def copy(self):
        return Keyframe(*(a.copy() for a in (self.kf, self.kcams, self.gcams, self.sf, self.cell_start, self.cell_feat,
                                             self.feats)))


class Hypothesis:
    """One search: Sbw (q [4] as x, y, z, w, t [3], s), its points (S3P_POINT_DTYPE), optionally its taken row
    (n_feats bytes: vpMatched[idx] != NULL on entry)."""

    def __init__(self, q, t, s, points, taken=None):
        self.q, self.t, self.s = np.asarray(q, F), np.asarray(t, F), F(s)
        self.points = np.ascontiguousarray(points, S3P_POINT_DTYPE)
        self.taken = None if taken is None else np.ascontiguousarray(taken, np.uint8)


class S3pResult:
    """Per hypothesis: rows [n_points, n_cam] S3P_ROW_DTYPE, feat_point [n_feats], poses [n_cam] S3P_POSE_DTYPE,
    n_matches."""

    def __init__(self, rows, feat_point, poses, n_matches):
        self.rows, self.feat_point, self.poses, self.n_matches = rows, feat_point, poses, int(n_matches)


def pack_hypotheses(kfm, hyps):
    """(searches, points, taken): the hypotheses one behind the other, every output range its own"""
    n_cam, nf = kfm.n_cam, len(kfm.feats)
    S = np.zeros(len(hyps), S3P_SEARCH_DTYPE)
    at_p = at_r = at_t = 0
    for k, h in enumerate(hyps):
        S[k]["q"], S[k]["t"], S[k]["s"] = h.q, h.t, h.s
        S[k]["point0"], S[k]["n_points"], S[k]["row0"] = at_p, len(h.points), at_r
        S[k]["featpt0"], S[k]["pose0"] = k * nf, k * n_cam
        S[k]["taken0"] = -1 if h.taken is None else at_t
        at_p += len(h.points)
        at_r += len(h.points) * n_cam
        at_t += 0 if h.taken is None else nf
    points = np.concatenate([h.points for h in hyps]) if hyps else np.zeros(0, S3P_POINT_DTYPE)
    tk = [h.taken for h in hyps if h.taken is not None]
    taken = np.concatenate(tk) if tk else np.zeros(0, np.uint8)
    return S, points, taken


def sim3_project_raw(tracker, kfm, searches, points, taken, rows, feat_point, poses, params):
    """The call itself on the caller's arrays (modified in place); returns the status code."""
    return _bind().lba_match_sim3_project(
        tracker.h, ptr(kfm.kf), ptr(kfm.kcams), ptr(kfm.gcams), ptr(kfm.sf), ptr(kfm.cell_start), len(kfm.cell_start),
        ptr(kfm.cell_feat), len(kfm.cell_feat), ptr(kfm.feats), len(kfm.feats), ptr(searches), len(searches),
        ptr(points), len(points), ptr(taken), len(taken), ptr(rows), len(rows), ptr(feat_point), len(feat_point),
        ptr(poses), len(poses), ctypes.byref(params))


def sim3_project(tracker, kfm, hyps, params):
    """Every hypothesis of `hyps` against the keyframe `kfm`: a list of S3pResult."""
    S, points, taken = pack_hypotheses(kfm, hyps)
    n_cam, nf = kfm.n_cam, len(kfm.feats)
    rows = np.zeros(len(points) * n_cam, S3P_ROW_DTYPE)
    feat_point = np.zeros(len(hyps) * nf, np.int32)
    poses = np.zeros(len(hyps) * n_cam, S3P_POSE_DTYPE)
    rc = sim3_project_raw(tracker, kfm, S, points, taken, rows, feat_point, poses, params)
    if rc != 0:
        raise LbaError(rc, "lba_match_sim3_project failed: " + tracker_last_error(tracker))
    out = []
    for k, h in enumerate(hyps):
        r0 = int(S[k]["row0"])
        out.append(S3pResult(rows[r0:r0 + len(h.points) * n_cam].reshape(len(h.points), n_cam),
                             feat_point[k * nf:(k + 1) * nf], poses[k * n_cam:(k + 1) * n_cam], S[k]["n_matches"]))
    return out


def sim3_project_kernel_ms(tracker, on=True):
    """track.kernel_ms for the call's six stretches: (k_s3p_pose, k_s3p_project, k_s3p_compact + k_s3p_base, the
    readback and the host's sizing, k_s3p_gather, k_s3p_resolve)"""
    return kernel_ms(tracker, "lba_match_sim3_project_profile", on, 6)


Tracker.sim3_project = sim3_project
Tracker.sim3_project_kernel_ms = sim3_project_kernel_ms


# ---------------------------------------------------------------- the caller's side of LoopClosing.cc on plain arrays
def points_from_keyframes(kf_points, bad):
    """:554-572 / :778-794: `kf_points` is a list, per keyframe of vpCovKFi in order, of its GetMapPointMatches() as
    point ids (-1: NULL); `bad[id]`: isBad().  Returns (vpMapPoints as ids, vpKeyFrames as indices into the list): every
    point once, at its first keyframe."""
    seen, pts, kfs = set(), [], []
    for k, ids in enumerate(kf_points):
        for i in ids:
            i = int(i)
            if i < 0 or bad[i] or i in seen:
                continue
            seen.add(i)
            pts.append(i)
            kfs.append(k)
    return np.array(pts, np.int64), np.array(kfs, np.int64)


def matched_kf(feat_point, point_kf):
    """:675-676: vpMatchedKF[idx] = vpPointsKFs[iMP] of the point the feature holds at the end, -1 where it holds none"""
    feat_point, point_kf = np.asarray(feat_point), np.asarray(point_kf)
    out = np.full(len(feat_point), -1, np.int64)
    has = feat_point >= 0
    out[has] = point_kf[feat_point[has]]
    return out


def quat_mul(a, b):
    """Hamilton product of (x, y, z, w) quaternions, float64"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def quat_rot(q, p):
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R @ np.asarray(p, float)


def scw_from_pair(pair, q_mw, t_mw):
    """:576-579: gScw = gScm * gSmw with gScm an lba_sim3_pair's (q, t, s) and gSmw = (Rmw, tmw, 1) the matched keyframe's
    pose; g2o's product (r1 r2, s1 (r1 t2) + t1, s1 s2) in float64, then Converter::toSophus's cast to float.  Returns
    (q, t, s) as float32, the Sbw of a search."""
    q1 = np.asarray(pair["q"], float)
    q1 = q1 / np.linalg.norm(q1)
    t1, s1 = np.asarray(pair["t"], float), float(pair["s"])
    q2 = np.asarray(q_mw, float)
    q2 = q2 / np.linalg.norm(q2)
    q = quat_mul(q1, q2)
    t = s1 * quat_rot(q1, np.asarray(t_mw, float)) + t1
    return (q / np.linalg.norm(q)).astype(F), t.astype(F), F(s1)


# ---------------------------------------------------------------- a seeded problem
def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])


def _so3_exp(w):
    th = np.linalg.norm(w)
    W = _hat(w)
    if th < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W


def _se3_exp(xi):
    """(rho, w) -> (R, t), Sophus's order"""
    rho, w = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    th = np.linalg.norm(w)
    W = _hat(w)
    V = np.eye(3) + 0.5 * W if th < 1e-12 else \
        np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W
    return _so3_exp(w), V @ rho


def _se3_log(R, t):
    c = np.clip((np.trace(R) - 1) / 2, -1, 1)
    th = np.arccos(c)
    w = np.zeros(3) if th < 1e-12 else th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    W = _hat(w)
    V = np.eye(3) + 0.5 * W if th < 1e-12 else \
        np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W
    return np.concatenate([np.linalg.solve(V, t), w])


def mat_to_quat(R):
    """(x, y, z, w) of a rotation matrix, w >= 0"""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        r = np.sqrt(max(0.0, 1 + R[i, i] - R[j, j] - R[k, k]))
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = r / 2, (R[j, i] + R[i, j]) / (2 * r), (R[k, i] + R[i, k]) / (2 * r), (R[k, j] - R[j, k]) / (2 * r)
    return q / np.linalg.norm(q)


S3P_K = (320.0, 320.0, 320.0, 240.0)


def make_s3p_problem(n_cam=4, n_feat=300, n_hyp=3, n_points=400, seed=0, n_levels=8, scale=1.2, dt=0.1, vel_noise=0.02,
                     hyp_noise=0.002, bits=(0, 90), async_cams=True, crowd=0.3):
    """A seeded keyframe and `n_hyp` hypotheses.  The keyframe has `n_cam` cameras (640 x 480, yaws 360 / n_cam apart,
    their stamps spread over the interval before the keyframe's when `async_cams`; the last camera is at the keyframe's
    own stamp), a previous keyframe `dt` before it and velocities close to the constant twist between the two (for
    which QueryPose is exp(tau w) exactly), so the per-camera poses are known up to `vel_noise`.  Every hypothesis is
    the true Tbw with a small perturbation and a scale near 1; its points are placed behind a random subset of the
    features, with the feature's descriptor up to `bits` bits off, a normal near the viewing ray and mfMaxDistance
    half a level away from the rounding edge of PredictScale.  Points of one hypothesis compete: several project within
    a pixel or two of the same feature, and a share `crowd` of them all sit on ONE feature (the resolve's worst case: a
    chain of about that many rounds).  Returns (Keyframe, [Hypothesis])."""
    rng = np.random.default_rng([seed, 0x733370])
    sf = scale_factors(n_levels, scale)
    fx, fy, cx, cy = S3P_K
    W, H = 640.0, 480.0
    # the body poses (Tbw) and the twist between them
    R_kf = _so3_exp(rng.normal(0, 0.3, 3))
    t_kf = rng.normal(0, 1.0, 3)
    w_true = np.concatenate([rng.normal(0, 0.5, 3), rng.normal(0, 0.2, 3)])          # body twist per second
    dR, dt_ = _se3_exp(w_true * dt)                                                    # Twb_prev^-1 Twb_kf
    R_wb, t_wb = R_kf.T, -R_kf.T @ t_kf
    R_wbp, t_wbp = R_wb @ dR.T, t_wb - R_wb @ dR.T @ dt_                               # Twb_prev = Twb_kf * d^-1
    R_prev, t_prev = R_wbp.T, -R_wbp.T @ t_wbp
    kf = np.zeros(1, S3P_KF_DTYPE)
    kf["stamp"], kf["stamp_prev"] = 100.0 + dt, 100.0
    kf["q"], kf["t"], kf["q_prev"], kf["t_prev"] = mat_to_quat(R_kf), t_kf, mat_to_quat(R_prev), t_prev
    kf["v"], kf["v_prev"] = w_true + rng.normal(0, vel_noise, 6), w_true + rng.normal(0, vel_noise, 6)
    kf["log_scale_factor"], kf["has_prev"], kf["n_levels"], kf["n_cam"] = np.log(scale), 1, n_levels, n_cam
    kcams = np.zeros(n_cam, S3P_CAM_DTYPE)
    Rcw, tcw = [], []
    for c in range(n_cam):
        a = 2 * np.pi * c / n_cam
        R_bc = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        t_bc = np.array([0.05 * np.cos(a), 0.0, 0.05 * np.sin(a)])
        tau = dt if (c == n_cam - 1 or not async_cams) else dt * (c + 1) / n_cam
        kcams[c]["stamp"] = 100.0 + tau
        kcams[c]["q_bc"], kcams[c]["t_bc"] = mat_to_quat(R_bc), t_bc
        kcams[c]["fx"], kcams[c]["fy"], kcams[c]["cx"], kcams[c]["cy"] = fx, fy, cx, cy
        kcams[c]["min_x"], kcams[c]["max_x"], kcams[c]["min_y"], kcams[c]["max_y"] = 0.0, W, 0.0, H
        eR, et = _se3_exp(w_true * tau)                                                # Twb_c = Twb_prev exp(tau w)
        R_wbc, t_wbc = R_wbp @ eR, t_wbp + R_wbp @ et
        R_wc, t_wc = R_wbc @ R_bc, t_wbc + R_wbc @ t_bc
        Rcw.append(R_wc.T)
        tcw.append(-R_wc.T @ t_wc)
        # GetCameraCenter(c) of the map pose: near the true centre (quirk (a): not the corrected one)
        kcams[c]["ow"] = t_wc + rng.normal(0, 0.002, 3)
    gcams = match_cams(n_cam, 0.0, 0.0, W, H)
    feats = np.zeros(n_cam * n_feat, MATCH_FEAT_DTYPE)
    feats["cam"] = np.repeat(np.arange(n_cam), n_feat)
    feats["x"], feats["y"] = rng.uniform(5, W - 5, len(feats)), rng.uniform(5, H - 5, len(feats))
    feats["octave"] = rng.integers(0, n_levels, len(feats))
    feats["u_right"] = -1.0
    feats["desc"] = rng.integers(0, 2 ** 32, size=(len(feats), 8), dtype=np.uint64).astype(np.uint32)
    feats = feats[rng.permutation(len(feats))]
    cell_start, cell_feat = build_grid(feats, gcams)
    kfm = Keyframe(kf, kcams, gcams, sf, cell_start, cell_feat, feats)
    hyps = []
    for _ in range(n_hyp):
        pts = np.zeros(n_points, S3P_POINT_DTYPE)
        target = rng.integers(0, len(feats), n_points)
        target[rng.random(n_points) < crowd] = target[0]                                # a crowd on one feature
        for p in range(n_points):
            f = feats[target[p]]
            c = int(f["cam"])
            depth = rng.uniform(2.0, 15.0)
            uv = np.array([f["x"], f["y"]], float) + rng.normal(0, 1.0, 2)
            Xc = np.array([(uv[0] - cx) / fx * depth, (uv[1] - cy) / fy * depth, depth])
            Xw = Rcw[c].T @ (Xc - tcw[c])
            PO = Xw - kcams[c]["ow"].astype(float)
            dist = np.linalg.norm(PO)
            n = PO / dist + rng.normal(0, 0.3, 3)
            lvl = int(f["octave"]) + int(rng.integers(0, 2))                          # the keypoint at level or level - 1
            pts[p]["pos"], pts[p]["normal"] = Xw, n / np.linalg.norm(n)
            maxd = dist * scale ** (lvl - rng.uniform(0.2, 0.8))
            pts[p]["max_distance"] = maxd
            pts[p]["max_dist"], pts[p]["min_dist"] = 1.2 * maxd, 0.8 * maxd / scale ** (n_levels - 1)
            pts[p]["desc"] = flip_bits(f["desc"], rng.integers(bits[0], bits[1] + 1), rng)
            pts[p]["skip"] = rng.random() < 0.05
        eR, et = _se3_exp(rng.normal(0, hyp_noise, 6))
        s = 1.0 + rng.normal(0, 0.01)
        R_h, t_h = eR @ R_kf, (eR @ t_kf + et) * s                                    # Sbw: t / s is the SE3's translation
        hyps.append(Hypothesis(mat_to_quat(R_h), t_h, s, pts))
    return kfm, hyps
