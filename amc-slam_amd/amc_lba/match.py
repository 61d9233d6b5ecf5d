"""ORBmatcher's two projection searches (src/ORBmatcher.cc:43-217 and :1439-1568) through the C ABI
(lba_match_project on an lba_tracker): a batch of searches, one GPU wave per (point, camera) job, then one workgroup
per (search, camera) that reproduces the reference's sequential loop exactly.

`match_project` is the call on packed arrays; `Search` holds one frame's arrays and `pack_searches` makes a batch.
The caller's side of the reference on plain arrays, in float32 numpy: `build_grid` (AssignFeaturesToGrid with
PosInGrid's round), `jobs_local_points` (isInFrustum's fields, RadiusByViewingCos and the th factor, :64-75) and
`jobs_last_frame` (the projection and tests of :1459-1480).  These helpers are host-side restatements for building
inputs; they are NOT held to the reference's float bits (Eigen's SE3f * Vector3f is not reproduced bit for bit).
`make_match_search` makes a seeded multi-camera frame with 256-bit descriptors.
"""
import ctypes

import numpy as np

from . import LbaError
from .abi import MATCH_CAM_DTYPE, MATCH_FEAT_DTYPE, MATCH_JOB_DTYPE, MATCH_SEARCH_DTYPE, ptr
from .track import Tracker, _bind as _bind_track, kernel_ms

MATCH_RATIO, MATCH_BEST = 0, 1
MATCH_OK, MATCH_NO_CAND, MATCH_TOO_FAR, MATCH_RATIO_FAIL, MATCH_ROT = range(5)
MATCH_STATUS_NAMES = ("OK", "NO_CAND", "TOO_FAR", "RATIO_FAIL", "ROT")
MATCH_MAX_FEAT = 8192       # per camera; LBA_E_LIMIT above
GRID_COLS, GRID_ROWS = 64, 48
GRID_CELLS = GRID_COLS * GRID_ROWS
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30
MATCH_JOB_OUTPUTS = ("feat", "status", "best_dist", "best_dist2")
F = np.float32


class LbaMatchParams(ctypes.Structure):
    """lba_match_params"""
    _fields_ = [("mode", ctypes.c_int32), ("th_high", ctypes.c_int32), ("nn_ratio", ctypes.c_float),
                ("stereo_cam", ctypes.c_int32), ("ur_truncate", ctypes.c_int32), ("check_orientation", ctypes.c_int32)]


def match_params(mode, n_cam, th_high=TH_HIGH, nn_ratio=0.8, stereo_cam=None, ur_truncate=None, check_orientation=None):
    """The reference's settings of either function: the stereo camera is the last one; the last-frame function
    truncates u_right and checks the orientation; SearchLocalPoints builds its matcher with nnratio 0.8."""
    best = mode == MATCH_BEST
    return LbaMatchParams(int(mode), int(th_high), float(nn_ratio), n_cam - 1 if stereo_cam is None else int(stereo_cam),
                          int(best if ur_truncate is None else ur_truncate),
                          int(best if check_orientation is None else check_orientation))


def _bind():
    L = _bind_track()
    if not getattr(L, "_match_bound", False):
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.lba_match_project.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32,
                                        ctypes.POINTER(LbaMatchParams)]
        L.lba_tracker_last_error.argtypes = [vp]
        L.lba_tracker_last_error.restype = ctypes.c_char_p
        L._match_bound = True
    return L


def tracker_last_error(tracker):
    return _bind().lba_tracker_last_error(tracker.h).decode()


def match_project(tracker, searches, cams, cell_start, cell_feat, feats, jobs, params):
    """Every job of every search, in place: jobs get feat / status / best_dist / best_dist2, features `job`, cameras
    `rounds`, searches n_matches / n_matches_mono.  Arrays of the right dtype and layout are modified in place and
    returned; others are copied first.  Returns (searches, cams, feats, jobs)."""
    searches = np.ascontiguousarray(searches, MATCH_SEARCH_DTYPE)
    cams = np.ascontiguousarray(cams, MATCH_CAM_DTYPE)
    cell_start = np.ascontiguousarray(cell_start, np.int32)
    cell_feat = np.ascontiguousarray(cell_feat, np.int32)
    feats = np.ascontiguousarray(feats, MATCH_FEAT_DTYPE)
    jobs = np.ascontiguousarray(jobs, MATCH_JOB_DTYPE)
    rc = _bind().lba_match_project(tracker.h, ptr(searches), len(searches), ptr(cams), len(cams), ptr(cell_start),
                                   len(cell_start), ptr(cell_feat), len(cell_feat), ptr(feats), len(feats), ptr(jobs),
                                   len(jobs), ctypes.byref(params))
    if rc != 0:
        raise LbaError(rc, "lba_match_project failed: " + tracker_last_error(tracker))
    return searches, cams, feats, jobs


def match_kernel_ms(tracker, on=True):
    """track.kernel_ms for lba_match_project's two launches: (k_match_gather, k_match_resolve)"""
    return kernel_ms(tracker, "lba_match_profile", on, 2)


Tracker.match_project = match_project
Tracker.match_kernel_ms = match_kernel_ms
Tracker.last_error = tracker_last_error


class Search:
    """One frame: cams [n_cam], cell_start [n_cam * 3072 + 1], cell_feat, feats, jobs (the ABI's dtypes)."""

    def __init__(self, cams, cell_start, cell_feat, feats, jobs):
        self.cams = np.ascontiguousarray(cams, MATCH_CAM_DTYPE)
        self.cell_start = np.ascontiguousarray(cell_start, np.int32)
        self.cell_feat = np.ascontiguousarray(cell_feat, np.int32)
        self.feats = np.ascontiguousarray(feats, MATCH_FEAT_DTYPE)
        self.jobs = np.ascontiguousarray(jobs, MATCH_JOB_DTYPE)

    @property
    def n_cam(self):
        return len(self.cams)

    def copy(self):
        return Search(self.cams.copy(), self.cell_start.copy(), self.cell_feat.copy(), self.feats.copy(), self.jobs.copy())


def pack_searches(searches):
    """A batch: (searches, cams, cell_start, cell_feat, feats, jobs), the searches one behind the other."""
    S = np.zeros(len(searches), MATCH_SEARCH_DTYPE)
    at = dict(cam=0, feat=0, job=0, cell=0, cf=0)
    for k, s in enumerate(searches):
        S[k]["cam0"], S[k]["n_cam"], S[k]["feat0"], S[k]["n_feat"] = at["cam"], len(s.cams), at["feat"], len(s.feats)
        S[k]["job0"], S[k]["n_jobs"], S[k]["cell0"], S[k]["cf0"] = at["job"], len(s.jobs), at["cell"], at["cf"]
        at["cam"] += len(s.cams); at["feat"] += len(s.feats); at["job"] += len(s.jobs)
        at["cell"] += len(s.cell_start); at["cf"] += len(s.cell_feat)

    def cat(name, dtype):
        parts = [getattr(s, name) for s in searches]
        return np.concatenate(parts) if parts else np.zeros(0, dtype)

    return (S, cat("cams", MATCH_CAM_DTYPE), cat("cell_start", np.int32), cat("cell_feat", np.int32),
            cat("feats", MATCH_FEAT_DTYPE), cat("jobs", MATCH_JOB_DTYPE))


def match_searches(tracker, searches, params):
    """`searches`: Search objects.  Returns (search records, [Search with the outputs filled in])."""
    S, cams, cs, cf, feats, jobs = pack_searches(searches)
    S, cams, feats, jobs = match_project(tracker, S, cams, cs, cf, feats, jobs, params)
    out = []
    for k, s in enumerate(searches):
        R = S[k]
        out.append(Search(cams[R["cam0"]:R["cam0"] + R["n_cam"]], s.cell_start, s.cell_feat,
                          feats[R["feat0"]:R["feat0"] + R["n_feat"]], jobs[R["job0"]:R["job0"] + R["n_jobs"]]))
    return S, out


def c_round(v):
    """C's round() (half away from zero) of float32 values, as integers"""
    v = np.asarray(v, F)
    return (np.sign(v) * np.floor(np.abs(v) + F(0.5))).astype(np.int64)


def match_cams(n_cam, min_x=0.0, min_y=0.0, max_x=640.0, max_y=480.0):
    """mvGridElementWidthInv = FRAME_GRID_COLS / (mvMaxX - mvMinX), in float"""
    cams = np.zeros(n_cam, MATCH_CAM_DTYPE)
    cams["min_x"], cams["min_y"] = min_x, min_y
    cams["grid_w_inv"] = F(GRID_COLS) / (F(max_x) - F(min_x))
    cams["grid_h_inv"] = F(GRID_ROWS) / (F(max_y) - F(min_y))
    return cams


def build_grid(feats, cams):
    """AssignFeaturesToGrid: every feature, in index order, goes to the cell PosInGrid gives it (round, in float32), or
    nowhere when that is outside the grid.  Returns (cell_start [n_cam * 3072 + 1], cell_feat)."""
    feats, cams = np.asarray(feats), np.asarray(cams)
    n_cam = len(cams)
    c = feats["cam"].astype(np.int64)
    px = c_round((feats["x"] - cams["min_x"][c]) * cams["grid_w_inv"][c])
    py = c_round((feats["y"] - cams["min_y"][c]) * cams["grid_h_inv"][c])
    inside = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    cell = (c * GRID_CELLS + px * GRID_ROWS + py)[inside]
    idx = np.flatnonzero(inside)
    order = np.argsort(cell, kind="stable")          # stable: insertion order within a cell
    cell_start = np.zeros(n_cam * GRID_CELLS + 1, np.int32)
    np.cumsum(np.bincount(cell, minlength=n_cam * GRID_CELLS), out=cell_start[1:])
    return cell_start, idx[order].astype(np.int32)


def radius_by_viewing_cos(view_cos):
    """ORBmatcher::RadiusByViewingCos: 2.5 above 0.998, else 4.0"""
    return np.where(np.asarray(view_cos, F) > F(0.998), F(2.5), F(4.0)).astype(F)


def scale_factors(n_levels=8, scale=1.2):
    sf = np.ones(n_levels, F)
    for i in range(1, n_levels):
        sf[i] = sf[i - 1] * F(scale)
    return sf


def jobs_local_points(in_view, proj_x, proj_y, proj_xr, level, view_cos, desc, blocks, sf, th=1.0, point=None):
    """The jobs of SearchByProjection(F, vpMapPoints, th) (:50-75): per point and camera with mvbTrackInView, the
    window r * mvScaleFactors[level] with r = RadiusByViewingCos(viewCos) (times th when th != 1), levels
    [level - 1, level].  The [n_points, n_cam] arrays are isInFrustum's fields; desc [n_points, 8] uint32; blocks
    [n_points]: Observations() > 0.  The caller leaves out bad points and, under bFarPoints, the far ones."""
    in_view = np.asarray(in_view, bool)
    p, c = np.nonzero(in_view)                      # point-major, cameras inner
    jobs = np.zeros(len(p), MATCH_JOB_DTYPE)
    lvl = np.asarray(level, np.int64)[p, c]
    r = radius_by_viewing_cos(np.asarray(view_cos, F)[p, c])
    if F(th) != F(1.0):
        r = r * F(th)
    jobs["x"], jobs["y"], jobs["ur"] = np.asarray(proj_x, F)[p, c], np.asarray(proj_y, F)[p, c], np.asarray(proj_xr, F)[p, c]
    jobs["radius"] = r * np.asarray(sf, F)[lvl]
    jobs["cam"], jobs["min_level"], jobs["max_level"] = c, lvl - 1, lvl
    jobs["point"] = p if point is None else np.asarray(point)[p]
    jobs["blocks"] = np.asarray(blocks)[p] != 0
    jobs["desc"] = np.asarray(desc, np.uint32)[p]
    return jobs


def jobs_last_frame(Xw, Rcw, tcw, K, bounds, octave, angle, desc, blocks, sf, bf, th, point=None):
    """The jobs of SearchByProjection(Current, Last, th) (:1452-1480): per last-frame point and camera, x3Dc = Tcw x3Dw,
    invzc = 1 / z (skipped when negative), the pinhole projection, the image bounds, radius = th * mvScaleFactors[octave],
    levels [octave - 1, octave + 1], ur = u - mbf * invzc.  Rcw [n_cam, 3, 3], tcw [n_cam, 3], K [n_cam, 4]
    (fx, fy, cx, cy), bounds [n_cam, 4] (min_x, max_x, min_y, max_y); float32 throughout."""
    Xw, Rcw, tcw, K, bounds = (np.asarray(a, F) for a in (Xw, Rcw, tcw, K, bounds))
    n, n_cam = len(Xw), len(Rcw)
    Xc = np.zeros((n, n_cam, 3), F)
    for c in range(n_cam):
        R = Rcw[c]
        for i in range(3):
            Xc[:, c, i] = (R[i, 0] * Xw[:, 0] + R[i, 1] * Xw[:, 1]) + R[i, 2] * Xw[:, 2] + tcw[c, i]
    with np.errstate(all="ignore"):
        invz = (1.0 / Xc[..., 2].astype(np.float64)).astype(F)
        u = K[None, :, 0] * Xc[..., 0] / Xc[..., 2] + K[None, :, 2]
        v = K[None, :, 1] * Xc[..., 1] / Xc[..., 2] + K[None, :, 3]
        keep = ~(invz < 0) & ~(u < bounds[None, :, 0]) & ~(u > bounds[None, :, 1]) & ~(v < bounds[None, :, 2]) \
            & ~(v > bounds[None, :, 3])
    p, c = np.nonzero(keep)
    octv = np.asarray(octave, np.int64)[p]
    jobs = np.zeros(len(p), MATCH_JOB_DTYPE)
    jobs["x"], jobs["y"] = u[p, c], v[p, c]
    jobs["radius"] = F(th) * np.asarray(sf, F)[octv]
    jobs["ur"] = u[p, c] - F(bf) * invz[p, c]
    jobs["angle"] = np.asarray(angle, F)[p]
    jobs["cam"], jobs["min_level"], jobs["max_level"] = c, octv - 1, octv + 1
    jobs["point"] = p if point is None else np.asarray(point)[p]
    jobs["blocks"] = np.asarray(blocks)[p] != 0
    jobs["desc"] = np.asarray(desc, np.uint32)[p]
    return jobs


def flip_bits(desc, n_bits, rng):
    """a copy of the 256-bit descriptor [8] uint32 with n_bits distinct bits flipped"""
    out = np.array(desc, np.uint32)
    for b in rng.choice(256, size=int(n_bits), replace=False):
        out[b >> 5] ^= np.uint32(1) << np.uint32(b & 31)
    return out


MATCH_K = (320.0, 320.0, 320.0, 240.0)     # fx, fy, cx, cy of the synthetic cameras (640 x 480)


def match_rig(n_cam):
    """cameras looking along yaws of 360 / n_cam degrees apart, a few centimetres off the body's origin; the body frame
    is the world's: (Rcw [n_cam, 3, 3], tcw [n_cam, 3])"""
    Rcw, tcw = [], []
    for c in range(n_cam):
        a = 2 * np.pi * c / n_cam
        R = np.array([[np.cos(a), 0.0, -np.sin(a)], [0.0, 1.0, 0.0], [np.sin(a), 0.0, np.cos(a)]])
        Rcw.append(R)
        tcw.append(-R @ np.array([0.05 * np.cos(a), 0.0, 0.05 * np.sin(a)]))
    return np.array(Rcw, F), np.array(tcw, F)


def make_match_search(mode=MATCH_RATIO, n_cam=4, n_feat=400, n_points=600, seed=0, cluster=4, spread=6.0,
                      bits=(0, 70), taken_frac=0.1, blocks_frac=0.8, second_cam_frac=0.3, th=None, n_levels=8):
    """A seeded frame: per camera `n_feat` features in a 640 x 480 image, the LAST camera stereo (u_right on 70 % of its
    features); `n_points` map points in clusters of `cluster`: the points of a cluster share a base descriptor (each a
    few bits off it) and project within `spread` pixels of each other, so their windows overlap and they compete for
    the same features.  Each point is observed in one camera (a share `second_cam_frac` in a second one as well) by a
    feature that carries the point's descriptor with a number of flipped bits drawn from `bits`, so distances land on
    both sides of TH_HIGH and of the ratio.  A share `taken_frac` of the features is taken on entry, `blocks_frac` of
    the points block.  LBA_MATCH_RATIO: the jobs come from jobs_local_points on isInFrustum-style fields;
    LBA_MATCH_BEST: the points are placed in space behind their pixels and jobs_last_frame projects them (th 15 by
    default, 7 for a stereo-like narrow window when given).  Returns a Search."""
    rng = np.random.default_rng([seed, 0x6d61, mode])
    sf = scale_factors(n_levels)
    fx, fy, cx, cy = MATCH_K
    W, H, bf = 640.0, 480.0, 40.0
    cams = match_cams(n_cam, 0.0, 0.0, W, H)
    n_clusters = max(1, -(-n_points // max(1, cluster)))
    base = rng.integers(0, 2 ** 32, size=(n_clusters, 8), dtype=np.uint64).astype(np.uint32)
    centre = np.stack([rng.uniform(10, W - 10, n_clusters), rng.uniform(10, H - 10, n_clusters)], 1)
    ccam = rng.integers(0, n_cam, n_clusters)
    pdesc = np.zeros((n_points, 8), np.uint32)
    feats = np.zeros(n_cam * n_feat, MATCH_FEAT_DTYPE)
    feats["cam"] = np.repeat(np.arange(n_cam), n_feat)
    feats["x"], feats["y"] = rng.uniform(0, W, len(feats)), rng.uniform(0, H, len(feats))
    feats["octave"] = rng.integers(0, n_levels, len(feats))
    feats["angle"] = rng.uniform(0, 360, len(feats))
    feats["desc"] = rng.integers(0, 2 ** 32, size=(len(feats), 8), dtype=np.uint64).astype(np.uint32)
    nxt = np.zeros(n_cam, np.int64)                      # the next free feature of each camera
    in_view = np.zeros((n_points, n_cam), bool)
    px, py = np.zeros((n_points, n_cam), F), np.zeros((n_points, n_cam), F)
    level = np.zeros((n_points, n_cam), np.int64)
    pangle = rng.uniform(0, 360, n_points).astype(F)
    depth = rng.uniform(2.0, 20.0, n_points)
    for p in range(n_points):
        k = p // max(1, cluster)
        pdesc[p] = flip_bits(base[k], rng.integers(0, 12), rng)
        c0 = int(ccam[k])
        views = [c0] + ([int((c0 + 1) % n_cam)] if n_cam > 1 and rng.random() < second_cam_frac else [])
        lvl = int(rng.integers(0, n_levels))
        for c in views:
            uv = np.clip(centre[k] + rng.uniform(-spread, spread, 2), 1.0, [W - 1.0, H - 1.0])
            in_view[p, c], px[p, c], py[p, c], level[p, c] = True, uv[0], uv[1], lvl
            if nxt[c] < n_feat and rng.random() < 0.8:   # its observation, a pixel or two off
                f = feats[c * n_feat + nxt[c]]
                nxt[c] += 1
                f["x"], f["y"] = np.clip(uv + rng.normal(0, 1.0, 2), 0.0, [W - 0.01, H - 0.01])
                f["octave"] = np.clip(lvl + rng.integers(-1, 1), 0, n_levels - 1)
                f["desc"] = flip_bits(pdesc[p], rng.integers(bits[0], bits[1] + 1), rng)
                rot = [0.0, 0.0, 0.0, 45.0, 200.0][int(rng.integers(0, 5))]
                f["angle"] = (pangle[p] - rot + rng.normal(0, 3.0)) % 360.0
    last = feats["cam"] == n_cam - 1
    feats["u_right"] = np.where(last & (rng.random(len(feats)) < 0.7), feats["x"] - bf / rng.uniform(2.0, 20.0, len(feats)), -1.0)
    feats["taken"] = rng.random(len(feats)) < taken_frac
    perm = rng.permutation(len(feats))                   # features of the cameras interleaved, as mmpKeyToCam allows
    feats = feats[perm]
    blocks = rng.random(n_points) < blocks_frac
    if mode == MATCH_RATIO:
        view_cos = np.where(rng.random((n_points, n_cam)) < 0.5, 0.9995, 0.9)
        z = depth[:, None]
        jobs = jobs_local_points(in_view, px, py, px - F(bf) / z.astype(F), level, view_cos, pdesc, blocks, sf,
                                 1.0 if th is None else th)
    else:
        Rcw, tcw = match_rig(n_cam)
        Xw = np.zeros((n_points, 3))
        for p in range(n_points):
            c = int(np.flatnonzero(in_view[p])[0])
            Xc = np.array([(px[p, c] - cx) / fx * depth[p], (py[p, c] - cy) / fy * depth[p], depth[p]])
            Xw[p] = Rcw[c].astype(float).T @ (Xc - tcw[c])
        K = np.tile(np.array(MATCH_K, F), (n_cam, 1))
        bounds = np.tile(np.array([0.0, W, 0.0, H], F), (n_cam, 1))
        jobs = jobs_last_frame(Xw, Rcw, tcw, K, bounds, level.max(axis=1), pangle, pdesc, blocks, sf, bf,
                               15.0 if th is None else th)
    cell_start, cell_feat = build_grid(feats, cams)
    return Search(cams, cell_start, cell_feat, feats, jobs)
