"""Local mapping's CreateNewMapPoints triangulation (src/LocalMapping.cc:408-587) through the C ABI (lba_triangulate
on an lba_tracker): a batch of (keyframe, neighbour) pairs with their matched rows, one GPU thread per row.

`Tracker.triangulate` is the call.  The caller's side of the reference on plain arrays: `tri_rows` (the row
construction, :412-432, :498, :525, :565), `ratio_factor` (:350), `new_point_geometry` (MapPoint::UpdateNormalAndDepth
for the point just made) and `first_wins` (the rule for batching all neighbours of one keyframe).
`make_tri_pairs` makes synthetic pairs: a multi-camera rig whose last camera is stereo, seen from two places.
"""
import ctypes

import numpy as np

from . import LbaError
from .abi import TRI_CAM_DTYPE, TRI_KF_DTYPE, TRI_PAIR_DTYPE, TRI_ROW_DTYPE, ptr
from .track import Tracker, _bind as _bind_track, kernel_ms

(TRI_OK, TRI_PARALLAX, TRI_W_ZERO, TRI_NO_DEPTH, TRI_BEHIND1, TRI_BEHIND2, TRI_REPROJ1, TRI_REPROJ2, TRI_DIST_ZERO,
 TRI_FAR, TRI_SCALE) = range(11)
TRI_STATUS_NAMES = ("OK", "PARALLAX", "W_ZERO", "NO_DEPTH", "BEHIND1", "BEHIND2", "REPROJ1", "REPROJ2", "DIST_ZERO",
                    "FAR", "SCALE")
TRI_MAX_CAM = 64       # LBA_E_LIMIT above (a pair's camera records are kept in LDS)
TRI_ROW_OUTPUTS = ("status", "stereo_point", "X")
TRI_PAIR_OUTPUTS = ("n_new", "n_stereo")


class LbaTriParams(ctypes.Structure):
    """lba_tri_params: ratioFactor (:350), mThFarPoints, mbFarPoints."""
    _fields_ = [("ratio_factor", ctypes.c_double), ("th_far", ctypes.c_double), ("far_points", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


def ratio_factor(scale=1.2):
    """ratioFactor = 1.5f * mfScaleFactor (:350): a float product, widened."""
    return float(np.float32(1.5) * np.float32(scale))


def tri_params(scale=1.2, far_points=False, th_far=0.0):
    return LbaTriParams(ratio_factor(scale), float(th_far), int(bool(far_points)), 0)


def _bind():
    L = _bind_track()
    if not getattr(L, "_tri_bound", False):
        vp = ctypes.c_void_p
        L.lba_triangulate.argtypes = [vp, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, ctypes.c_int32,
                                      ctypes.c_int32, ctypes.POINTER(LbaTriParams)]
        L._tri_bound = True
    return L


def triangulate(tracker, pairs, rows, kfs, cams, n_cam, params=None):
    """Every row of every pair, in place: the rows get status (TRI_*), stereo_point and, under TRI_OK, X; the pairs
    n_new and n_stereo.  `params`: an LbaTriParams (tri_params(...)) or None for ratio_factor 1.5 * 1.2 and no far-point
    cut.  Arrays of the right dtype and layout are modified in place and returned; others are copied first."""
    pairs = np.ascontiguousarray(pairs, TRI_PAIR_DTYPE)
    rows = np.ascontiguousarray(rows, TRI_ROW_DTYPE)
    kfs = np.ascontiguousarray(kfs, TRI_KF_DTYPE)
    cams = np.ascontiguousarray(cams, TRI_CAM_DTYPE)
    rc = _bind().lba_triangulate(tracker.h, ptr(pairs), len(pairs), ptr(rows), len(rows), ptr(kfs), len(kfs), ptr(cams),
                                 len(cams), int(n_cam), ctypes.byref(params) if params is not None else None)
    if rc != 0:
        raise LbaError(rc, "lba_triangulate failed")
    return pairs, rows


def triangulate_kernel_ms(tracker, on=True):
    """track.kernel_ms for lba_triangulate's launch"""
    return kernel_ms(tracker, "lba_triangulate_profile", on)


Tracker.triangulate_kernel_ms = triangulate_kernel_ms


def tri_rows(matches, kf1, kf2, n_cam):
    """The row construction of the loop over vMatchedIndices (:410-432, :498, :525, :565) on plain arrays.
    `matches` [n, 2]: (idx1, idx2) as SearchForTriangulation returns them.  kf1 / kf2: a mapping per keyframe with
      key_to_cam       mmpKeyToCam[idx]                    keys_un   mvKeysUn[idx].pt [N, 2]
      keys             mvKeys[idx].pt [N, 2]               octave    mvKeysUn[idx].octave
      global_to_local  mmpGlobalToLocalID[idx]             u_right   mvuRight[local]
      depth            mvDepth[local]                      level_sigma2, scale_factors   per octave
    ur is mvuRight only for a keypoint of the LAST camera (n_cam - 1), -1 otherwise; depth is looked up for every row
    whose local index exists (it is read only when that side is stereo), 0 otherwise.
    Returns the lba_tri_row array the kernel gets (status, stereo_point and X zero)."""
    matches = np.asarray(matches, np.int64).reshape(-1, 2)
    rows = np.zeros(len(matches), TRI_ROW_DTYPE)
    for side, (kf, idx) in enumerate(((kf1, matches[:, 0]), (kf2, matches[:, 1])), start=1):
        cam = np.asarray(kf["key_to_cam"], np.int64)[idx]
        octave = np.asarray(kf["octave"], np.int64)[idx]
        local = np.asarray(kf["global_to_local"], np.int64)[idx]
        u_right, depth = np.asarray(kf["u_right"], np.float32), np.asarray(kf["depth"], np.float32)
        has = (local >= 0) & (local < len(u_right))
        safe = np.where(has, local, 0)
        last = cam == n_cam - 1
        if (last & ~has).any():
            raise ValueError("a keypoint of the last camera without a local index")
        rows[f"cam{side}"] = cam
        rows[f"z{side}"] = np.asarray(kf["keys_un"], np.float32)[idx]
        rows[f"k{side}"] = np.asarray(kf["keys"], np.float32)[idx]
        rows[f"ur{side}"] = np.where(last, u_right[safe] if len(u_right) else -1.0, np.float32(-1.0))
        rows[f"depth{side}"] = np.where(has, depth[safe] if len(depth) else 0.0, np.float32(0.0))
        rows[f"sigma2_{side}"] = np.asarray(kf["level_sigma2"], np.float32)[octave]
        rows[f"scale{side}"] = np.asarray(kf["scale_factors"], np.float32)[octave]
    return rows


def new_point_geometry(X, Ow1, Ow2, scale1, scale_last):
    """MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:611-700) for the point CreateNewMapPoints has just made: two
    observations (Ow1, Ow2: the centres of the observing cameras), reference keyframe KF1.  In float, as the map:
    normal = (n1 / |n1| + n2 / |n2|) / 2, mfMaxDistance = |X - Ow1| scale1, mfMinDistance = that / scale_last
    (scale1 = mvScaleFactors[kp1.octave], scale_last = mvScaleFactors[nLevels - 1]).
    Returns (normal [n, 3], min_distance [n], max_distance [n]) as float32."""
    f = np.float32
    X, Ow1, Ow2 = (np.atleast_2d(np.asarray(a, f)) for a in (X, Ow1, Ow2))
    scale1, scale_last = np.atleast_1d(np.asarray(scale1, f)), f(scale_last)

    def norm(v):   # Eigen's norm(): sqrt of the squared sum in order
        return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2], dtype=f)

    n1, n2 = X - Ow1, X - Ow2
    d1, d2 = norm(n1), norm(n2)
    with np.errstate(all="ignore"):
        normal = (n1 / d1[:, None] + n2 / d2[:, None]) / f(2)
        max_d = np.maximum(np.finfo(f).tiny, d1 * scale1)
        min_d = np.minimum(np.finfo(f).max, d1 * scale1 / scale_last)
    return normal.astype(f), min_d.astype(f), max_d.astype(f)


def first_wins(pairs, rows, idx1, idx2):
    """The rule for batching ALL neighbours of one keyframe in one call, when their matches were made up front.

    The reference matches neighbour i + 1 only after neighbour i's points exist: SearchForTriangulation skips keypoints
    that already have a map point (ORBmatcher.cc:1002-1007).  One call per neighbour (n_pairs = 1), matching in
    between, is therefore the exact sequence, and pairs of DIFFERENT current keyframes batch exactly.  With the matches
    of all neighbours made before any point exists, a keypoint can be matched in several pairs; this keeps, per keypoint
    of either keyframe, the first accepted row (TRI_OK) in pair order, row order within a pair.

    This is a DEVIATION from the reference: there the matcher would not have offered the later rows at all, and would
    have re-matched, which can free their partner for another keypoint; a row dropped here is simply lost.

    idx1, idx2 [n_rows]: the keypoint indices (vMatchedIndices) of every row.  Returns the bool mask of the rows kept."""
    pairs, rows = np.asarray(pairs), np.asarray(rows)
    keep = np.zeros(len(rows), bool)
    taken = set()
    for P in pairs:
        for r in range(int(P["row0"]), int(P["row0"]) + int(P["n_rows"])):
            if rows["status"][r] != TRI_OK or keep[r]:
                continue
            a, b = (int(P["kf1"]), int(idx1[r])), (int(P["kf2"]), int(idx2[r]))
            if a in taken or b in taken:
                continue
            taken.update((a, b))
            keep[r] = True
    return keep


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def scale_pyramid(n_levels=8, scale=1.2):
    """mvScaleFactors / mvLevelSigma2 as ORBextractor builds them: float products level by level."""
    sf = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        sf[i] = sf[i - 1] * np.float32(scale)
    return sf, sf * sf


TRI_K = (500.0, 500.0, 480.0, 300.0)   # fx, fy, cx, cy of the synthetic cameras
_RBC0 = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])   # camera axes (z ahead) in a z-up frame


def tri_rig(n_cam):
    """The synthetic rig: (Rbc [n_cam], tbc [n_cam]); cameras at yaws 90, 180, -90 degrees, ..., the LAST one looking
    ahead.  The body frame IS the last camera's: UnprojectStereo places its point with the body pose."""
    from .synth import _rotz
    yaws = [np.pi / 2, np.pi, -np.pi / 2]
    cam_yaw = [yaws[c % 3] for c in range(n_cam - 1)] + [0.0]
    Rbc = [_rotz(y) @ _RBC0 for y in cam_yaw]
    tbc = [np.array([0.5 * np.cos(y), 0.5 * np.sin(y), 0.2]) for y in cam_yaw]
    return [Rbc[-1].T @ R for R in Rbc], [Rbc[-1].T @ (t - tbc[-1]) for t in tbc]


def tri_keyframes(poses, n_cam, stereo_b=0.12):
    """lba_tri_kf / lba_tri_cam records of keyframes at the body poses [(Rwb, twb)] with the rig of tri_rig: every
    value rounded to float as the map holds it; keyframe k's cameras at rows [k n_cam, (k + 1) n_cam)."""
    fx, fy, cx, cy = TRI_K
    Rbc, tbc = tri_rig(n_cam)
    kfs = np.zeros(len(poses), TRI_KF_DTYPE)
    cams = np.zeros(len(poses) * n_cam, TRI_CAM_DTYPE)
    for k, (Rwb, twb) in enumerate(poses):
        Rwb, twb = _f32(Rwb), _f32(twb)
        kfs[k]["Rwb"], kfs[k]["twb"], kfs[k]["cam0"] = Rwb.ravel(), twb, k * n_cam
        kfs[k]["bf"], kfs[k]["b"] = np.float32(fx * stereo_b), np.float32(stereo_b)
        for c in range(n_cam):
            Rwc, twc = Rwb @ Rbc[c], Rwb @ tbc[c] + twb
            C = cams[k * n_cam + c]
            C["Tcw"], C["Ow"] = _f32(np.hstack([Rwc.T, (-Rwc.T @ twc)[:, None]])).ravel(), _f32(twc)
            C["fx"], C["fy"], C["cx"], C["cy"] = fx, fy, cx, cy
            C["invfx"], C["invfy"] = np.float32(1.0) / np.float32(fx), np.float32(1.0) / np.float32(fy)
    return kfs, cams


def tri_project(cam, X):
    """(u, v, z) of the world point X in the camera record `cam`, in double"""
    T = np.asarray(cam["Tcw"]).reshape(3, 4)
    Y = T[:, :3] @ np.asarray(X, float) + T[:, 3]
    return np.array([cam["fx"] * Y[0] / Y[2] + cam["cx"], cam["fy"] * Y[1] / Y[2] + cam["cy"], Y[2]])


def make_tri_pairs(n_pairs=1, n_rows=300, n_cam=4, baselines=(1.0, 1.5, 2.0, 3.0), noise=0.5, outlier_frac=0.1,
                   seed=0, depth_range=(3.0, 25.0), stereo_frac=0.7, stereo_b=0.12, raw_offset=0.0, n_octaves=8,
                   shared_current=True):
    """Synthetic CreateNewMapPoints inputs: a rig of `n_cam` pinhole cameras (yaws 90, 180, -90 degrees, the LAST one
    looking ahead and stereo with baseline `stereo_b`), a current keyframe and `n_pairs` neighbours, neighbour p
    displaced by `baselines[p % len]` metres diagonally to the rig's axes (so every camera gets parallax) and turned a
    few degrees.  Per pair `n_rows` matches: a point at a depth in `depth_range` in front of a random camera of the
    current keyframe, seen by the neighbour's camera that has it nearest its image centre; keypoints with `noise`
    pixels of Gaussian error, a share `outlier_frac` of gross outliers (20 .. 100 px off in the neighbour); a share
    `stereo_frac` of the last camera's keypoints has a right coordinate and a depth; octaves follow the distance ratio,
    so the scale gate passes unless the row is a gross outlier.  The raw keypoint is the undistorted one plus
    `raw_offset` pixels.  Every value is rounded to float as the map holds it.  shared_current=False gives every pair
    a current keyframe of its own.
    Baselines of 1 m and more against depths to 25 m keep well over a third of the rows through the parallax gate.
    Returns (pairs, rows, kfs, cams, truth) with truth = {"X": the points, "gross": bool, "idx1", "idx2": keypoint
    indices for first_wins, "octave1", "octave2"}."""
    from .synth import _rotz, _expso3
    rng = np.random.default_rng([seed, 0x7219])
    fx, fy, cx, cy = TRI_K
    W, H = 960.0, 600.0
    sf, sig2 = scale_pyramid(n_octaves)
    bf = float(np.float32(fx * stereo_b))

    def current():
        return _rotz(rng.uniform(-np.pi, np.pi)) @ _RBC0, rng.uniform(-20, 20, 3)

    poses, cur = [], current()
    for p in range(n_pairs):
        if p == 0 or not shared_current:
            if p:
                cur = current()
            poses.append(cur)
        b = baselines[p % len(baselines)]
        d = cur[0] @ (np.array([np.cos(0.7 + 0.9 * p), 0.1, np.sin(0.7 + 0.9 * p)]) * b)
        poses.append((cur[0] @ _expso3(rng.normal(0, np.deg2rad(3.0), 3)), cur[1] + d))
    kfs, cams = tri_keyframes(poses, n_cam, stereo_b)
    pose = [[(C["Tcw"].reshape(3, 4)[:, :3], C["Tcw"].reshape(3, 4)[:, 3], C["Ow"]) for C in cams[k * n_cam:(k + 1) * n_cam]]
            for k in range(len(kfs))]

    pairs = np.zeros(n_pairs, TRI_PAIR_DTYPE)
    rows = np.zeros(n_pairs * n_rows, TRI_ROW_DTYPE)
    truth = {"X": np.zeros((len(rows), 3)), "gross": np.zeros(len(rows), bool), "idx1": np.zeros(len(rows), np.int64),
             "idx2": np.zeros(len(rows), np.int64), "octave1": np.zeros(len(rows), np.int64),
             "octave2": np.zeros(len(rows), np.int64)}
    for p in range(n_pairs):
        k1, k2 = (0, p + 1) if shared_current else (2 * p, 2 * p + 1)
        pairs[p]["kf1"], pairs[p]["kf2"], pairs[p]["row0"], pairs[p]["n_rows"] = k1, k2, p * n_rows, n_rows
        for i in range(n_rows):
            r = rows[p * n_rows + i]
            c1 = int(rng.integers(0, n_cam))
            R1, t1, O1 = pose[k1][c1]
            uv = np.array([rng.uniform(20, W - 20), rng.uniform(20, H - 20)])
            z = rng.uniform(*depth_range)
            Xc = np.array([(uv[0] - cx) / fx * z, (uv[1] - cy) / fy * z, z])
            Xw = R1.T @ (Xc - t1)
            # the neighbour's camera that sees it nearest its centre
            best, c2 = np.inf, c1
            for c in range(n_cam):
                Y = pose[k2][c][0] @ Xw + pose[k2][c][1]
                if Y[2] > 0.1:
                    off = np.hypot(fx * Y[0] / Y[2], fy * Y[1] / Y[2])
                    if off < best:
                        best, c2 = off, c
            R2, t2, O2 = pose[k2][c2]
            Y1, Y2 = R1 @ Xw + t1, R2 @ Xw + t2
            gross = rng.random() < outlier_frac
            o1 = int(rng.integers(0, n_octaves))
            ratio = np.linalg.norm(Xw - O2) / np.linalg.norm(Xw - O1)
            o2 = int(np.clip(o1 - np.round(np.log(ratio) / np.log(1.2)), 0, n_octaves - 1))
            for side, (Y, c, o, kf) in enumerate(((Y1, c1, o1, k1), (Y2, c2, o2, k2)), start=1):
                u = np.array([fx * Y[0] / Y[2] + cx, fy * Y[1] / Y[2] + cy]) + rng.normal(0, noise, 2) * float(sf[o])
                if gross and side == 2:
                    ang, far = rng.uniform(0, 2 * np.pi), rng.uniform(20, 100)
                    u = u + far * np.array([np.cos(ang), np.sin(ang)])
                r[f"cam{side}"], r[f"z{side}"], r[f"k{side}"] = c, _f32(u), _f32(u + raw_offset)
                r[f"sigma2_{side}"], r[f"scale{side}"] = sig2[o], sf[o]
                r[f"ur{side}"], r[f"depth{side}"] = -1.0, 0.0
                if c == n_cam - 1 and rng.random() < stereo_frac and Y[2] > 0.1:
                    ur = np.float32(u[0] - bf / Y[2] + rng.normal(0, noise * 0.5))
                    disp = np.float32(u[0]) - ur
                    if ur >= 0 and disp > 0:
                        r[f"ur{side}"], r[f"depth{side}"] = ur, np.float32(bf) / disp
            j = p * n_rows + i
            truth["X"][j], truth["gross"][j] = Xw, gross
            truth["idx1"][j], truth["idx2"][j] = rng.integers(0, max(1, 2 * n_rows)), j
            truth["octave1"][j], truth["octave2"][j] = o1, o2
    return pairs, rows, kfs, cams, truth
