"""Loop closing's Sim3Solver RANSAC (src/Sim3Solver.cc, driven by LoopClosing.cc:527-539) through the C ABI
(lba_sim3_ransac on an lba_tracker): a batch of candidate pairs, one GPU wave per hypothesis, then one per pair.

`Tracker.sim3_ransac` is the call.  The caller's side of the reference on plain arrays: `sim3_ransac_rows` (the
constructor's filtering, :85-147), `ransac_max_iterations` (SetRansacParameters, :155-179), `draw_triples` (:277-291)
and `seed_sim3_pairs` (LoopClosing.cc:576: the selected transform as lba_sim3_optimize's start).
`make_sim3_ransac_pairs` makes synthetic candidates: two rigs that see the same points.
"""
import ctypes
import math

import numpy as np

from . import LbaError
from .abi import ptr
from .sim3 import SIM3_CAM_DTYPE, SIM3_PAIR_DTYPE, _bind as _bind_sim3, make_sim3_pairs
from .track import Tracker, kernel_ms

S3R_CORR_DTYPE = np.dtype([
    ("cam1", "<i4"), ("cam2", "<i4"), ("inlier", "<i4"), ("pad", "<i4"),
    ("X1b", "<f8", (3,)), ("X2b", "<f8", (3,)), ("max_err1", "<f8"), ("max_err2", "<f8"),
], align=True)
S3R_PAIR_DTYPE = np.dtype([
    ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"),
    ("fix_scale", "<i4"), ("min_inliers", "<i4"), ("corr0", "<i4"), ("n_corr", "<i4"), ("cam0", "<i4"),
    ("hyp0", "<i4"), ("n_hyp", "<i4"), ("best_hyp", "<i4"), ("n_inliers", "<i4"), ("converged", "<i4"),
], align=True)
assert S3R_CORR_DTYPE.itemsize == 80
assert S3R_PAIR_DTYPE.itemsize == 104
S3R_PAIR_OUTPUTS = ("q", "t", "s", "best_hyp", "n_inliers", "converged")   # every other field is an input
S3R_DEGENERATE = 1     # hyp_flags: |vec| < 1e-5, the hypothesis was skipped (Sim3Solver.cc:399-400)
S3R_NONFINITE = 2      # hyp_flags: q, t or s is not finite
S3R_MAX_CAM = 64       # LBA_E_LIMIT above (a pair's camera records are kept in LDS)
CHI2_GATE = 9.210      # Sim3Solver.cc:129-130


def _bind():
    L = _bind_sim3()
    if not getattr(L, "_s3r_bound", False):
        vp = ctypes.c_void_p
        L.lba_sim3_ransac.argtypes = [vp, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, ctypes.c_int32,
                                      ctypes.c_int32, vp, vp, vp]
        L._s3r_bound = True
    return L


def sim3_ransac(tracker, pairs, corr, samples, cams, n_cam, per_hyp=True):
    """The whole RANSAC loop of every pair, in place: the pairs get best_hyp, n_inliers, converged and q, t, s of the
    selected hypothesis (untouched when best_hyp < 0), the rows their inlier flag.  `samples` [n_hyp, 3]: pair-local
    row indices, each pair's at [hyp0, hyp0 + n_hyp).  With per_hyp also returns {"S12" [n_hyp, 8], "inliers", "flags"}.
    Arrays of the right dtype and layout are modified in place and returned; others are copied first."""
    pairs = np.ascontiguousarray(pairs, S3R_PAIR_DTYPE)
    corr = np.ascontiguousarray(corr, S3R_CORR_DTYPE)
    cams = np.ascontiguousarray(cams, SIM3_CAM_DTYPE)
    samples = np.ascontiguousarray(samples, np.int32).reshape(-1, 3)
    n_hyp = len(samples)
    hyp = {"S12": np.zeros((n_hyp, 8)), "inliers": np.zeros(n_hyp, np.int32), "flags": np.zeros(n_hyp, np.int32)} if per_hyp else None
    out = [ptr(hyp[k]) for k in ("S12", "inliers", "flags")] if per_hyp else [None] * 3
    rc = _bind().lba_sim3_ransac(tracker.h, ptr(pairs), len(pairs), ptr(corr), len(corr), ptr(samples), n_hyp, ptr(cams),
                                 len(cams), int(n_cam), *out)
    if rc != 0:
        raise LbaError(rc, "lba_sim3_ransac failed")
    return (pairs, corr, hyp) if per_hyp else (pairs, corr)


def sim3_ransac_kernel_ms(tracker, on=True):
    """track.kernel_ms for lba_sim3_ransac's two launches together"""
    return kernel_ms(tracker, "lba_sim3_ransac_profile", on)


Tracker.sim3_ransac = sim3_ransac
Tracker.sim3_ransac_kernel_ms = sim3_ransac_kernel_ms


def max_error(sigma2):
    """mvnMaxError1/2 as the reference holds them: std::vector<size_t>, so 9.210 * sigma2 (a double product of the
    float sigma2) is truncated to an integer: 9 at level 0, 13 at level 1 of a 1.2 pyramid."""
    return np.floor(CHI2_GATE * np.asarray(sigma2, np.float32).astype(np.float64))


def sim3_ransac_rows(match, has_mp1, bad1, bad2, index1, index2, cam1, cam2, X1b, X2b, sigma2_1, sigma2_2):
    """The constructor's loop over vpMatched12 (:85-147) on per-match arrays of length mN1:
      match     vpMatched12[i1] != NULL                    has_mp1   vpKeyFrameMP1[i1] != NULL
      bad1      pMP1->isBad()                              bad2      pMP2->isBad()
      index1    pMP1->GetIndexInKeyFrame(pKF1)[cam1]       cam1      pKF1->mmpKeyToCam[i1]
      index2    pMP2's index in the matched keyframe in camera cam2, the first camera with one, or -1 (:110-118)
      cam2      that camera (0 when index2 < 0)
      X1b, X2b  Rbw1 X3D1w + tbw1, Rbw2 X3D2w + tbw2 (float)
      sigma2_1  pKF1->mvLevelSigma2[kp1.octave]            sigma2_2  that of the matched keyframe's keypoint
    A match is skipped when it is null, point 1 does not exist, either point is bad, or either index is negative.
    Returns (rows, mvnIndices1): `rows` the lba_s3r_corr array the kernel gets, mvnIndices1[r] the match index of row r
    (vbInliers[mvnIndices1[r]] = rows["inlier"][r], :309-311)."""
    idx = [i for i in range(len(match))
           if match[i] and has_mp1[i] and not (bad1[i] or bad2[i]) and index1[i] >= 0 and index2[i] >= 0]
    idx = np.array(idx, np.int64)
    rows = np.zeros(idx.size, S3R_CORR_DTYPE)
    rows["cam1"], rows["cam2"] = np.asarray(cam1)[idx], np.asarray(cam2)[idx]
    rows["X1b"] = np.asarray(X1b, np.float32)[idx].reshape(-1, 3)
    rows["X2b"] = np.asarray(X2b, np.float32)[idx].reshape(-1, 3)
    rows["max_err1"] = max_error(np.asarray(sigma2_1)[idx])
    rows["max_err2"] = max_error(np.asarray(sigma2_2)[idx])
    return rows, idx


def ransac_max_iterations(N, prob=0.99, min_inliers=15, max_its=300):
    """mRansacMaxIts after SetRansacParameters(prob, min_inliers, max_its) with N correspondences (:155-179):
    epsilon is a float quotient, pow and log are double; min_inliers == N gives 1.  Where the reference converts a
    value that is not finite to int (N = 0, min_inliers = 0 or > N; x86 gives INT_MIN) the result is 1."""
    if min_inliers == N:
        n_it = 1
    else:
        with np.errstate(all="ignore"):
            eps = np.float32(min_inliers) / np.float32(N)
            x = np.log(1.0 - prob) / np.log(1.0 - float(eps) ** 3)
        n_it = int(math.ceil(x)) if np.isfinite(x) else -2**31
    return max(1, min(n_it, int(max_its)))


def draw_triples(N, n_hyp, rng):
    """n_hyp minimal sets drawn as iterate() does (:277-291): three draws without replacement from a fresh
    vAvailableIndices, the drawn slot refilled with the back.  rng: numpy Generator (DUtils::Random in the reference).
    Returns [n_hyp, 3] int32 row indices."""
    if N < 3:
        raise ValueError("a minimal set needs three correspondences")
    out = np.zeros((n_hyp, 3), np.int32)
    for h in range(n_hyp):
        avail = list(range(N))
        for i in range(3):
            r = int(rng.integers(0, len(avail)))
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def seed_sim3_pairs(ransac_pairs, sim3_pairs):
    """gScm = Sim3(GetEstimatedRotation(), GetEstimatedTranslation(), GetEstimatedScale()) (LoopClosing.cc:576): the
    selected q, t, s of every pair with a selected hypothesis written into the lba_sim3_pair of the same index, the
    start of lba_sim3_optimize.  Returns the mask of the pairs that converged (the ones the reference goes on with)."""
    ransac_pairs = np.asarray(ransac_pairs)
    if len(ransac_pairs) != len(sim3_pairs) or sim3_pairs.dtype != SIM3_PAIR_DTYPE:
        raise ValueError("one lba_sim3_pair per RANSAC pair")
    got = ransac_pairs["best_hyp"] >= 0
    for k in ("q", "t", "s"):
        sim3_pairs[k][got] = ransac_pairs[k][got]
    return ransac_pairs["converged"] != 0


def make_sim3_ransac_pairs(n_pairs=1, n_corr=100, n_cam=4, noise=0.004, outlier_frac=0.3, seed=0, s_true=1.0,
                           fix_scale=False, min_inliers=15, n_hyp=300, n_octaves=2, n_gross=None, **geometry):
    """Synthetic Sim3Solver inputs on the geometry of make_sim3_pairs (two rigs of `n_cam` pinhole cameras, a true S12
    of scale `s_true`, `n_corr` points seen by a camera of either rig; `geometry` goes to it): the body points
    X1b = Tc1b^-1 X1c and X2b = Tc2b^-1 X2c rounded to float, X2b with `noise` metres of Gaussian error, a share
    `outlier_frac` of gross outliers (or exactly `n_gross` rows; X2b 1 .. 5 m off), octave gates
    floor(9.210 * 1.2^(2k)), k < n_octaves, and `n_hyp` triples per pair from draw_triples.
    Returns (pairs, corr, samples, cams, truth); truth also carries the lba_sim3_pair / lba_sim3_corr arrays of the
    same candidates ("sim3_pairs", "sim3_corr": noiseless keypoints) for chaining into lba_sim3_optimize."""
    from .synth import quat_to_rot
    s3_pairs, s3_corr, cams, truth = make_sim3_pairs(n_pairs=n_pairs, n_corr=n_corr, n_cam=n_cam, noise=0.0,
                                                     outlier_frac=0.0, seed=seed, s_true=s_true, fix_scale=fix_scale,
                                                     n_gross=0, **geometry)
    rng = np.random.default_rng([seed, 0x53335])
    pairs = np.zeros(n_pairs, S3R_PAIR_DTYPE)
    corr = np.zeros(n_pairs * n_corr, S3R_CORR_DTYPE)
    samples = np.zeros((n_pairs * n_hyp, 3), np.int32)
    corr["cam1"], corr["cam2"] = s3_corr["cam1"], s3_corr["cam2"]
    gross_all = np.zeros(n_pairs * n_corr, bool)
    for p in range(n_pairs):
        P = pairs[p]
        P["fix_scale"], P["min_inliers"] = int(fix_scale), min_inliers
        P["corr0"], P["n_corr"], P["cam0"] = p * n_corr, n_corr, p * 2 * n_cam
        P["hyp0"], P["n_hyp"] = p * n_hyp, n_hyp
        P["best_hyp"] = -1
        if n_gross is None:
            gross = rng.random(n_corr) < outlier_frac
        else:
            gross = np.zeros(n_corr, bool)
            gross[rng.choice(n_corr, n_gross, replace=False)] = True
        gross_all[p * n_corr:(p + 1) * n_corr] = gross
        for r in range(n_corr):
            o, src = corr[p * n_corr + r], s3_corr[p * n_corr + r]
            c1, c2 = cams[P["cam0"] + src["cam1"]], cams[P["cam0"] + n_cam + src["cam2"]]
            X1b = quat_to_rot(c1["q"]).T @ (src["X1c"] - c1["t"])
            X2b = quat_to_rot(c2["q"]).T @ (src["X2c"] - c2["t"]) + rng.normal(0, noise, 3)
            if gross[r]:
                d = rng.normal(0, 1, 3)
                X2b = X2b + rng.uniform(1.0, 5.0) * d / np.linalg.norm(d)
            o["X1b"], o["X2b"] = X1b.astype(np.float32), X2b.astype(np.float32)
            o["max_err1"] = max_error(np.float32(1.2 ** (2 * rng.integers(0, n_octaves))))
            o["max_err2"] = max_error(np.float32(1.2 ** (2 * rng.integers(0, n_octaves))))
        if n_hyp:
            samples[p * n_hyp:(p + 1) * n_hyp] = draw_triples(n_corr, n_hyp, rng)
    truth = dict(truth, gross=gross_all, sim3_pairs=s3_pairs, sim3_corr=s3_corr)
    return pairs, corr, samples, cams, truth
