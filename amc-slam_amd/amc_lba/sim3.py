"""Loop closing's Sim3 optimisation (Optimizer::OptimizeSim3, src/Optimizer.cc:2049-2362) through the C ABI
(lba_sim3_optimize on an lba_tracker): a batch of candidate pairs (KF1, KF2), one GPU workgroup each, one launch.

`Tracker.sim3_optimize` is the call, `sim3_rows` the reference's caller-side filtering of the matches
(:2125-2216) on plain arrays, `make_sim3_pairs` synthetic candidates: two rigs that see the same points.
"""
import ctypes

import numpy as np

from . import LbaError
from .abi import ptr
from .track import Tracker, _bind as _bind_track, kernel_ms

SIM3_CAM_DTYPE = np.dtype([
    ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"),
], align=True)
SIM3_CORR_DTYPE = np.dtype([
    ("cam1", "<i4"), ("cam2", "<i4"), ("outlier", "<i4"), ("pad", "<i4"),
    ("X1c", "<f8", (3,)), ("X2c", "<f8", (3,)), ("z1", "<f8", (2,)), ("z2", "<f8", (2,)), ("w1", "<f8"), ("w2", "<f8"),
], align=True)
SIM3_PAIR_DTYPE = np.dtype([
    ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("th2", "<f8"),
    ("fix_scale", "<i4"), ("corr0", "<i4"), ("n_corr", "<i4"), ("cam0", "<i4"),
    ("n_in", "<i4"), ("n_bad", "<i4"), ("iterations", "<i4"), ("pad", "<i4"),
], align=True)
assert SIM3_CAM_DTYPE.itemsize == 88
assert SIM3_CORR_DTYPE.itemsize == 112
assert SIM3_PAIR_DTYPE.itemsize == 104
SIM3_PAIR_OUTPUTS = ("q", "t", "s", "n_in", "n_bad", "iterations")   # every other field is an input
SIM3_MIN_INLIERS = 10                                                # nCorrespondences - nBad < 10 returns 0 (:2328)


def _bind():
    L = _bind_track()
    if not getattr(L, "_sim3_bound", False):
        vp = ctypes.c_void_p
        L.lba_sim3_optimize.argtypes = [vp, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, ctypes.c_int32, ctypes.c_int32]
        L._sim3_bound = True
    return L


def sim3_optimize(tracker, pairs, corr, cams, n_cam):
    """OptimizeSim3 for every pair, in place like vel_ransac: the pairs get S12 (q, t, s; untouched where the early
    return was taken), n_in (the reference's return value), n_bad, iterations; the rows their outlier flag
    (vpMatches1[vnIndexEdge[row]] = NULL).  `cams`: per pair its 2 * n_cam cameras from cam0 on, KF1's then KF2's.
    Arrays of the right dtype and layout are modified in place and returned; others are copied first."""
    pairs = np.ascontiguousarray(pairs, SIM3_PAIR_DTYPE)
    corr = np.ascontiguousarray(corr, SIM3_CORR_DTYPE)
    cams = np.ascontiguousarray(cams, SIM3_CAM_DTYPE)
    rc = _bind().lba_sim3_optimize(tracker.h, ptr(pairs), len(pairs), ptr(corr), len(corr), ptr(cams), len(cams), int(n_cam))
    if rc != 0:
        raise LbaError(rc, "lba_sim3_optimize failed")
    return pairs, corr


def sim3_kernel_ms(tracker, on=True):
    """track.kernel_ms for lba_sim3_optimize's launch"""
    return kernel_ms(tracker, "lba_sim3_profile", on)


Tracker.sim3_optimize = sim3_optimize
Tracker.sim3_kernel_ms = sim3_kernel_ms


def sim3_rows(match, has_mp1, bad1, bad2, i2, cam1, cam2, P3D1c, P3D2c, z1, z2, w1, w2):
    """The reference's loop over vpMatches1 (:2125-2216) on per-match arrays of length N:
      match    vpMatches1[i] != NULL                       has_mp1  vpMapPoints1[i] != NULL
      bad1     pMP1->isBad()                               bad2     pMP2->isBad()
      i2       pMP2's index in KF2 in camera cam2, the first camera with one, or -1 (:2139-2150)
      cam1     pKF1->mmpKeyToCam[i]                        cam2     that camera (0 when i2 < 0)
      P3D1c    vR1w[cam1] P3D1w + vt1w[cam1] (float)       P3D2c    vR2w[cam2] P3D2w + vt2w[cam2] (float)
      z1, w1   mvKeysUn[i].pt, mvInvLevelSigma2[octave] of KF1;  z2, w2  those of KF2's keypoint i2
    A match is skipped when it is null, has no index in KF2, either point is bad (nBadMPs), point 1 does not exist
    (nMatchWithoutMP) or P3D2c(2) < 0.  Returns (rows, vnIndexEdge, nCorrespondences, counters): `rows` the
    lba_sim3_corr array the kernel gets, vnIndexEdge[r] the match index of row r (an `outlier` row r means
    vpMatches1[vnIndexEdge[r]] = NULL), counters = {"nBadMPs", "nMatchWithoutMP"}."""
    N = len(match)
    idx, n_bad_mps, n_without = [], 0, 0
    for i in range(N):
        if not match[i]:
            continue
        if i2[i] < 0:
            continue
        if has_mp1[i]:
            if bad1[i] or bad2[i]:
                n_bad_mps += 1
                continue
        else:
            n_without += 1
            continue
        if np.float32(P3D2c[i][2]) < 0:
            continue
        idx.append(i)
    idx = np.array(idx, np.int64)
    rows = np.zeros(idx.size, SIM3_CORR_DTYPE)
    rows["cam1"], rows["cam2"] = np.asarray(cam1)[idx], np.asarray(cam2)[idx]
    rows["X1c"] = np.asarray(P3D1c, np.float32)[idx].reshape(-1, 3)
    rows["X2c"] = np.asarray(P3D2c, np.float32)[idx].reshape(-1, 3)
    rows["z1"] = np.asarray(z1, np.float32)[idx].reshape(-1, 2)
    rows["z2"] = np.asarray(z2, np.float32)[idx].reshape(-1, 2)
    rows["w1"], rows["w2"] = np.asarray(w1, np.float32)[idx], np.asarray(w2, np.float32)[idx]
    return rows, idx, int(idx.size), {"nBadMPs": n_bad_mps, "nMatchWithoutMP": n_without}


def quat_of(R):
    """Eigen's Quaterniond(R), normalised, (x, y, z, w): what g2o::SE3Quat(R, t) holds (safe at w = 0, where
    synth.rot_to_quat takes its signs from rounding noise)."""
    R = np.asarray(R, float)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if tr > 0:
        t = np.sqrt(tr + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[:3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3], q[j], q[k] = (R[k, j] - R[j, k]) * t, (R[j, i] + R[i, j]) * t, (R[k, i] + R[i, k]) * t
    return q / np.linalg.norm(q)


def sim3_exp(u):
    """g2o::Sim3(update) for the generator (closed form; tests/sim3_oracle.py restates the reference's branches):
    (R, t, s) of update = [omega; upsilon; sigma]."""
    from .synth import _expso3
    u = np.asarray(u, float)
    w, ups, sigma = u[:3], u[3:6], u[6]
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    s = np.exp(sigma)
    C = (s - 1) / sigma if abs(sigma) > 1e-9 else 1.0
    if th < 1e-9:
        A = ((sigma - 1) * s + 1) / sigma**2 if abs(sigma) > 1e-5 else 0.5
        B = ((0.5 * sigma**2 - sigma + 1) * s) / sigma**3 if abs(sigma) > 1e-3 else 1.0 / 6.0
    else:
        a, b, c = s * np.sin(th), s * np.cos(th), th * th + sigma * sigma
        A = (a * sigma + (1 - b) * th) / (th * c)
        B = (C - ((b - 1) * sigma + a * th) / c) / (th * th)
    return _expso3(w), (A * K + B * (K @ K) + C * np.eye(3)) @ ups, s


def make_sim3_pairs(n_pairs=1, n_corr=40, n_cam=4, noise=0.7, outlier_frac=0.1, seed=0, s_true=1.0, start_sigma=0.02,
                    fix_scale=False, th2=10.0, n_octaves=8, cam_yaws=None, pairing="first", start_update=None,
                    n_gross=None):
    """Synthetic OptimizeSim3 inputs: per pair two rigs of `n_cam` pinhole cameras (float-valued body poses T1bw, T2bw
    in their own maps, Tcw = Tcb Tbw rounded to float, Tcb recovered as (Tcw * Tbw^-1) in float and widened as
    :2083-2088), a true S12 (yaw about 0.15 rad, some decimetres, scale `s_true`) and `n_corr` points seen by a
    camera of either rig: P3D1w / P3D2w float values in either map, X1c / X2c = R w + t in float, the keypoints with
    `noise` pixels of Gaussian error (float values), a share `outlier_frac` of gross outliers (or exactly `n_gross`
    rows; 20 .. 100 px off in one of the two images), octave weights 1 / 1.2^(2k).  The start S12 is
    Sim3(start_sigma N(0, 1)) * truth, or Sim3(start_update) * truth.
    cam_yaws: the cameras' yaw angles in the body (default: as make_vel_frames, n_cam - 1 side cameras and a front
    one).  pairing: "first" takes for cam2 the first camera of rig 2 that sees the point (the reference's rule),
    "spread" walks row r through the camera pair (r mod n_cam^2) and needs overlapping fields of view.
    Returns (pairs, corr, cams, truth), truth = {"R", "t", "s": per pair, "gross": bool per row}."""
    from .synth import _expso3, _f32, _rotz, quat_to_rot, rot_to_quat
    rng = np.random.default_rng(seed)
    F = np.float32
    Rbc0 = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    if cam_yaws is None:
        yaws = [np.pi / 2, np.pi, -np.pi / 2]
        cam_yaws = [yaws[c % 3] for c in range(n_cam - 1)] + [0.0]
    fx, fy, cx, cy, width, height = 500.0, 500.0, 480.0, 300.0, 960.0, 600.0
    Rbc = np.stack([_rotz(y) @ Rbc0 for y in cam_yaws])
    tbc = np.stack([[0.5 * np.cos(y), 0.5 * np.sin(y), 0.2] for y in cam_yaws])
    pairs = np.zeros(n_pairs, SIM3_PAIR_DTYPE)
    corr = np.zeros(n_pairs * n_corr, SIM3_CORR_DTYPE)
    cams = np.zeros(n_pairs * 2 * n_cam, SIM3_CAM_DTYPE)
    truth = {"R": np.zeros((n_pairs, 3, 3)), "t": np.zeros((n_pairs, 3)), "s": np.zeros(n_pairs),
             "gross": np.zeros(n_pairs * n_corr, bool)}

    def rig(k):
        """float body pose Tbw of a keyframe, its cameras' float Tcw, and Tcb = (Tcw * Tbw^-1) in float, widened"""
        q = rot_to_quat(_rotz(rng.uniform(-np.pi, np.pi))).astype(F)
        Rbw = quat_to_rot((q / np.linalg.norm(q)).astype(np.float64)).astype(F)
        tbw = rng.uniform(-20, 20, 3).astype(F)
        Rcw, tcw, Rcb, tcb = [], [], [], []
        for c in range(n_cam):
            Rcb_true, tcb_true = Rbc[c].T, -Rbc[c].T @ tbc[c]
            Rc = (Rcb_true @ Rbw.astype(np.float64)).astype(F)
            tc = (Rcb_true @ tbw.astype(np.float64) + tcb_true).astype(F)
            Rwb, twb = Rbw.T, -(Rbw.T @ tbw)                        # Tbw^-1 in float
            Rcb.append((Rc @ Rwb).astype(np.float64))                # (Tcw * Tbw^-1) in float, then widened
            tcb.append((Rc @ twb + tc).astype(np.float64))
            Rcw.append(Rc)
            tcw.append(tc)
        for c in range(n_cam):
            cm = cams[(2 * k_pair + k) * n_cam + c]
            cm["q"], cm["t"] = quat_of(Rcb[c]), tcb[c]
            cm["fx"], cm["fy"], cm["cx"], cm["cy"] = fx, fy, cx, cy
        return Rbw.astype(np.float64), tbw.astype(np.float64), Rcw, tcw

    def sees(c, Yb):
        Xc = Rbc[c].T @ (Yb - tbc[c])
        if Xc[2] < 0.5:
            return False
        u, v = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
        return 10 < u < width - 10 and 10 < v < height - 10

    for k_pair in range(n_pairs):
        R1bw, t1bw, R1cw, t1cw = rig(0)
        R2bw, t2bw, R2cw, t2cw = rig(1)
        R12 = _rotz(0.15 + rng.normal(0, 0.03)) @ _expso3(rng.normal(0, 0.02, 3))
        t12 = np.array([0.8, -0.3, 0.1]) + rng.normal(0, 0.1, 3)
        truth["R"][k_pair], truth["t"][k_pair], truth["s"][k_pair] = R12, t12, s_true
        upd = rng.normal(0, start_sigma, 7) if start_update is None else np.asarray(start_update, float)
        if fix_scale:
            upd[6] = 0.0
        Ru, tu, su = sim3_exp(upd)
        P = pairs[k_pair]
        P["q"], P["t"], P["s"] = quat_of(Ru @ R12), su * (Ru @ t12) + tu, su * s_true
        P["th2"], P["fix_scale"] = np.float32(th2), int(fix_scale)
        P["corr0"], P["n_corr"], P["cam0"] = k_pair * n_corr, n_corr, k_pair * 2 * n_cam
        rows = corr[k_pair * n_corr:(k_pair + 1) * n_corr]
        if n_gross is None:
            gross = rng.random(n_corr) < outlier_frac
        else:
            gross = np.zeros(n_corr, bool)
            gross[rng.choice(n_corr, n_gross, replace=False)] = True
        truth["gross"][k_pair * n_corr:(k_pair + 1) * n_corr] = gross
        for r in range(n_corr):
            for _ in range(10000):
                c1 = int(rng.integers(0, n_cam)) if pairing == "first" else (r % (n_cam * n_cam)) // n_cam
                uv = np.array([rng.uniform(20, width - 20), rng.uniform(20, height - 20)])
                depth = rng.uniform(4.0, 30.0)
                Xc = np.array([(uv[0] - cx) / fx * depth, (uv[1] - cy) / fy * depth, depth])
                Pb1 = Rbc[c1] @ Xc + tbc[c1]
                Yb2 = R12.T @ (Pb1 - t12) / s_true
                if pairing == "first":
                    seen = [c for c in range(n_cam) if sees(c, Yb2)]
                    if seen:
                        c2 = seen[0]
                        break
                else:
                    c2 = (r % (n_cam * n_cam)) % n_cam
                    if sees(c2, Yb2):
                        break
            else:
                raise ValueError("no point seen by both rigs: the cameras' fields do not overlap")
            Pw1 = (R1bw.T @ (Pb1 - t1bw)).astype(F)                 # GetWorldPos() of either map: float
            Pw2 = (R2bw.T @ (Yb2 - t2bw)).astype(F)
            X1c = R1cw[c1] @ Pw1 + t1cw[c1]                          # float arithmetic (:2164, :2172)
            X2c = R2cw[c2] @ Pw2 + t2cw[c2]
            X1 = X1c.astype(np.float64)
            X2 = X2c.astype(np.float64)
            z1 = np.array([fx * X1[0] / X1[2] + cx, fy * X1[1] / X1[2] + cy]) + rng.normal(0, noise, 2)
            z2 = np.array([fx * X2[0] / X2[2] + cx, fy * X2[1] / X2[2] + cy]) + rng.normal(0, noise, 2)
            ang, far = rng.uniform(0, 2 * np.pi), rng.uniform(20, 100)
            if gross[r]:
                off = far * np.array([np.cos(ang), np.sin(ang)])
                if rng.random() < 0.5:
                    z1 = z1 + off
                else:
                    z2 = z2 + off
            o = rows[r]
            o["cam1"], o["cam2"] = c1, c2
            o["X1c"], o["X2c"] = X1, X2
            o["z1"], o["z2"] = _f32(z1), _f32(z2)
            o["w1"] = F(1.0 / 1.2 ** (2 * rng.integers(0, n_octaves)))
            o["w2"] = F(1.0 / 1.2 ** (2 * rng.integers(0, n_octaves)))
    return pairs, corr, cams, truth
