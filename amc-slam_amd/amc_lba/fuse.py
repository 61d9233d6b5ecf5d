"""ORBmatcher::Fuse (src/ORBmatcher.cc:1133-1316 and :1318-1437) split in two: the SEARCH through the C ABI
(lba_match_fuse on an lba_tracker), a pure function of a snapshot that the device decides for every (search, point,
camera) at once, and the order-dependent TAIL (`fuse_walk`), which applies the rows to the caller's map in the
reference's order and redoes, on the CPU, the few jobs whose row an earlier decision has invalidated.  See
include/amc_lba.h for the contract and the quirks that are kept.

`fuse` is the call on packed arrays (`fuse_raw` on the caller's own); `Target` holds one keyframe, `pack_targets` lays
several out one behind the other.  `fuse_walk` and `search_and_fuse_replaces` work on a small map interface (the tests'
ToyMap implements it).  `make_fuse_problem` makes a seeded scene: keyframes around it, map points, their observations.
"""
import numpy as np

from . import LbaError
from .abi import (FUSE_CAM_DTYPE, FUSE_ROW_DTYPE, FUSE_SEARCH_DTYPE, FUSE_TARGET_DTYPE, MATCH_CAM_DTYPE,
                  MATCH_FEAT_DTYPE, ptr)
from .match import build_grid, flip_bits, match_cams, scale_factors, tracker_last_error
from .sim3_project import S3P_POINT_DTYPE, mat_to_quat, _bind as _bind_s3p, _so3_exp
from .track import Tracker, kernel_ms

FUSE_KF, FUSE_SIM3 = 0, 1
(FUSE_OK, FUSE_NO_CAND, FUSE_TOO_FAR, FUSE_SKIPPED, FUSE_BEHIND, FUSE_OUT_OF_IMAGE, FUSE_DIST, FUSE_ANGLE,
 FUSE_NO_CAMERA) = range(9)
FUSE_STATUS_NAMES = ("OK", "NO_CAND", "TOO_FAR", "SKIPPED", "BEHIND", "OUT_OF_IMAGE", "DIST", "ANGLE", "NO_CAMERA")
FUSE_MAX_CAM = 64
TH_LOW = 50
TH_KF, TH_SIM3 = 3.0, 4.0          # Fuse's default th (ORBmatcher.h) and SearchAndFuse's (LoopClosing.cc:1071, :1116)
F = np.float32


def _bind():
    L = _bind_s3p()
    if not getattr(L, "_fuse_bound", False):
        import ctypes
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.lba_match_fuse.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32,
                                     vp, i32, vp, i32, i32]
        L._fuse_bound = True
    return L


class Target:
    """One keyframe: fcams [n_cam] FUSE_CAM_DTYPE, gcams [n_cam] MATCH_CAM_DTYPE, sf and sigma [n_levels]
    (mvScaleFactors, mvInvLevelSigma2), cell_start / cell_feat (amc_lba.match.build_grid), feats MATCH_FEAT_DTYPE
    (numbered from 0; `cam` is the camera within the keyframe), bf, log_scale_factor."""

    def __init__(self, fcams, gcams, sf, sigma, cell_start, cell_feat, feats, bf, log_scale_factor):
        self.fcams = np.ascontiguousarray(fcams, FUSE_CAM_DTYPE)
        self.gcams = np.ascontiguousarray(gcams, MATCH_CAM_DTYPE)
        self.sf = np.ascontiguousarray(sf, F)
        self.sigma = np.ascontiguousarray(sigma, F)
        self.cell_start = np.ascontiguousarray(cell_start, np.int32)
        self.cell_feat = np.ascontiguousarray(cell_feat, np.int32)
        self.feats = np.ascontiguousarray(feats, MATCH_FEAT_DTYPE)
        self.bf, self.log_scale_factor = F(bf), F(log_scale_factor)

    @property
    def n_cam(self):
        return len(self.fcams)

    @property
    def n_levels(self):
        return len(self.sf)

    def copy(self):
        return Target(self.fcams.copy(), self.gcams.copy(), self.sf.copy(), self.sigma.copy(), self.cell_start.copy(),
                      self.cell_feat.copy(), self.feats.copy(), self.bf, self.log_scale_factor)


class FusePack:
    """Targets one behind the other: T [n] FUSE_TARGET_DTYPE and the seven concatenated arrays"""
    ARRAYS = ("T", "fcams", "gcams", "sf", "sigma", "cell_start", "cell_feat", "feats")

    def __init__(self, T, fcams, gcams, sf, sigma, cell_start, cell_feat, feats):
        self.T, self.fcams, self.gcams, self.sf, self.sigma = T, fcams, gcams, sf, sigma
        self.cell_start, self.cell_feat, self.feats = cell_start, cell_feat, feats

    def copy(self):
        return FusePack(*(getattr(self, a).copy() for a in self.ARRAYS))


def pack_targets(targets):
    T = np.zeros(len(targets), FUSE_TARGET_DTYPE)
    at = dict(cam=0, feat=0, cell=0, cf=0, sf=0, sg=0)
    for k, t in enumerate(targets):
        T[k]["cam0"], T[k]["n_cam"], T[k]["feat0"], T[k]["n_feat"] = at["cam"], t.n_cam, at["feat"], len(t.feats)
        T[k]["cell0"], T[k]["cf0"], T[k]["sf0"], T[k]["sigma0"] = at["cell"], at["cf"], at["sf"], at["sg"]
        T[k]["bf"], T[k]["log_scale_factor"], T[k]["n_levels"] = t.bf, t.log_scale_factor, t.n_levels
        at["cam"] += t.n_cam; at["feat"] += len(t.feats); at["cell"] += len(t.cell_start)
        at["cf"] += len(t.cell_feat); at["sf"] += len(t.sf); at["sg"] += len(t.sigma)

    def cat(name, dtype):
        parts = [getattr(t, name) for t in targets]
        return np.concatenate(parts) if parts else np.zeros(0, dtype)

    return FusePack(T, cat("fcams", FUSE_CAM_DTYPE), cat("gcams", MATCH_CAM_DTYPE), cat("sf", F), cat("sigma", F),
                    cat("cell_start", np.int32), cat("cell_feat", np.int32), cat("feats", MATCH_FEAT_DTYPE))


def pack_searches(T, specs):
    """specs: (target, point0, n_points, mode, th) per search; the rows one search behind the other"""
    S = np.zeros(len(specs), FUSE_SEARCH_DTYPE)
    at = 0
    for k, (tg, p0, n, mode, th) in enumerate(specs):
        S[k]["target"], S[k]["point0"], S[k]["n_points"], S[k]["mode"], S[k]["th"], S[k]["row0"] = tg, p0, n, mode, th, at
        at += n * int(T[tg]["n_cam"])
    return S


def fuse_raw(tracker, pk, searches, points, rows, th_low=TH_LOW):
    """The call itself on the caller's arrays (searches and rows are written); returns the status code."""
    return _bind().lba_match_fuse(
        tracker.h, ptr(pk.T), len(pk.T), ptr(pk.fcams), ptr(pk.gcams), len(pk.fcams), ptr(pk.sf), len(pk.sf),
        ptr(pk.sigma), len(pk.sigma), ptr(pk.cell_start), len(pk.cell_start), ptr(pk.cell_feat), len(pk.cell_feat),
        ptr(pk.feats), len(pk.feats), ptr(searches), len(searches), ptr(points), len(points), ptr(rows), len(rows),
        int(th_low))


def split_rows(T, S, rows):
    """per search its rows as [n_points, n_cam]"""
    out = []
    for s in S:
        n_cam, n = int(T[s["target"]]["n_cam"]), int(s["n_points"])
        out.append(rows[int(s["row0"]):int(s["row0"]) + n * n_cam].reshape(n, n_cam))
    return out


def fuse(tracker, targets, points, specs, th_low=TH_LOW):
    """Every search of `specs` ((target, point0, n_points, mode, th)) on the Targets `targets` and the shared
    S3P_POINT_DTYPE array `points`: (search records, [rows [n_points, n_cam] FUSE_ROW_DTYPE per search])."""
    pk = pack_targets(targets)
    S = pack_searches(pk.T, specs)
    points = np.ascontiguousarray(points, S3P_POINT_DTYPE)
    rows = np.zeros(sum(int(s["n_points"]) * int(pk.T[s["target"]]["n_cam"]) for s in S), FUSE_ROW_DTYPE)
    rc = fuse_raw(tracker, pk, S, points, rows, th_low)
    if rc != 0:
        raise LbaError(rc, "lba_match_fuse failed: " + tracker_last_error(tracker))
    return S, split_rows(pk.T, S, rows)


def fuse_kernel_ms(tracker, on=True):
    """track.kernel_ms for lba_match_fuse's one launch (k_fuse)"""
    return kernel_ms(tracker, "lba_match_fuse_profile", on, 1)


Tracker.fuse = fuse
Tracker.fuse_kernel_ms = fuse_kernel_ms


# ---------------------------------------------------------------- the tail: the reference's order on the caller's map
def fuse_walk(rows, searches, point_ids, uploaded_desc, map, redo, kf_ids=None):
    """The map-editing tail of both Fuse overloads on the device's rows, exactly: searches in order, points in order,
    cameras inner.

    rows: per search [n_points, n_cam] FUSE_ROW_DTYPE; searches: FUSE_SEARCH_DTYPE records (target, point0, n_points,
    mode are read); point_ids / uploaded_desc: per entry of the uploaded `points` array the map's id (-1: a NULL entry)
    and the descriptor that went up; kf_ids: the map's keyframe per target (default: the target's index).
    map: is_bad(id), in_camera(id, kf, c), points_of(kf), occupant(kf, f) (-1: none), observations(id), descriptor(id),
    add(id, kf, f), replace(loser, winner).
    redo(search, point, camera) -> a row computed on the LIVE point; it is called, and its row used, when the device's
    row is OK or TOO_FAR and map.descriptor(id) differs from the uploaded bits, or when the row is SKIPPED though the
    live map does not skip the point, and in no other case: every other status is decided before the descriptor is read.
    Returns (n_fused per search, replace_out per search (None in mode KF, else ids, -1: none), the redone jobs)."""
    n_fused, replace_out, redone = [], [], []

    def row_of(s, i, c, pid):
        r = rows[s][i, c]
        st = int(r["status"])
        stale = (st in (FUSE_OK, FUSE_TOO_FAR) and
                 np.asarray(map.descriptor(pid)).tobytes() != np.asarray(uploaded_desc[int(searches[s]["point0"]) + i]).tobytes())
        if stale or st == FUSE_SKIPPED:
            redone.append((s, i, c))
            r = redo(s, i, c)
        return int(r["status"]), int(r["feat"])

    for s, S in enumerate(searches):
        kf = int(S["target"]) if kf_ids is None else kf_ids[int(S["target"])]
        n_cam, p0, n, nf = rows[s].shape[1], int(S["point0"]), int(S["n_points"]), 0
        if int(S["mode"]) == FUSE_KF:
            replace_out.append(None)
            for i in range(n):
                pid = int(point_ids[p0 + i])
                if pid < 0 or map.is_bad(pid):
                    continue
                for c in range(n_cam):
                    if map.in_camera(pid, kf, c):
                        continue
                    st, f = row_of(s, i, c, pid)
                    if st != FUSE_OK:
                        continue
                    occ = map.occupant(kf, f)
                    if occ >= 0:
                        if not map.is_bad(occ):
                            if map.observations(occ) > map.observations(pid):
                                map.replace(pid, occ)
                            else:
                                map.replace(occ, pid)
                    else:
                        map.add(pid, kf, f)
                    nf += 1
        else:
            found = set(int(x) for x in map.points_of(kf))
            rep = np.full(n, -1, np.int64)
            for i in range(n):
                pid = int(point_ids[p0 + i])
                if map.is_bad(pid) or pid in found:
                    continue
                for c in range(n_cam - 1):
                    st, f = row_of(s, i, c, pid)
                    if st != FUSE_OK:
                        continue
                    occ = map.occupant(kf, f)
                    if occ >= 0:
                        if not map.is_bad(occ):
                            rep[i] = occ
                    else:
                        map.add(pid, kf, f)
                    nf += 1
            replace_out.append(rep)
        n_fused.append(nf)
    return n_fused, replace_out, redone


def search_and_fuse_replaces(map, list_ids, replace_out):
    """LoopClosing::SearchAndFuse's loop after each keyframe (:1076-1087): pRep->Replace(vpMapPoints[i]); returns the
    number of replaces"""
    n = 0
    for i, rep in enumerate(replace_out):
        if rep >= 0:
            map.replace(int(rep), int(list_ids[i]))
            n += 1
    return n


def distinctive_descriptor(descs):
    """MapPoint::ComputeDistinctiveDescriptors' choice (src/MapPoint.cc:543-577) among `descs` [N, 8] uint32: the index
    of the first descriptor with the least median distance to the rest"""
    ints = [int.from_bytes(np.ascontiguousarray(d, np.uint32).tobytes(), "little") for d in descs]
    n = len(ints)
    best, best_i = None, 0
    for i in range(n):
        d = sorted(bin(ints[i] ^ ints[j]).count("1") for j in range(n))
        m = d[int(0.5 * (n - 1))]
        if best is None or m < best:
            best, best_i = m, i
    return best_i


# ---------------------------------------------------------------- a seeded problem
FUSE_K = (320.0, 320.0, 320.0, 240.0)
_W, _H = 640.0, 480.0


class FuseProblem:
    """targets: [Target] (the keyframes); per map point id: pos, normal, max_distance, min_dist, max_dist, desc [.., 8],
    bad; obs [n, 3] (id, keyframe, feature): the initial observations in insertion order; source [kf][f]: the scene
    point a feature was made from, or -1."""

    def __init__(self, targets, pos, normal, max_distance, desc, bad, obs, source, n_levels, scale):
        self.targets, self.pos, self.normal, self.max_distance = targets, pos, normal, max_distance
        self.desc, self.bad, self.obs, self.source = desc, bad, obs, source
        sf_top = scale_factors(n_levels, scale)[-1]
        self.min_dist = (F(0.8) * (max_distance / sf_top)).astype(F)
        self.max_dist = (F(1.2) * max_distance).astype(F)

    @property
    def n_ids(self):
        return len(self.pos)

    def points(self, ids, skip=None, desc=None):
        """the S3P_POINT_DTYPE entries of a list of ids (-1: a NULL entry, uploaded with skip = 1)"""
        ids = np.asarray(ids, np.int64)
        P = np.zeros(len(ids), S3P_POINT_DTYPE)
        ok = ids >= 0
        j = ids[ok]
        P["pos"][ok], P["normal"][ok], P["max_distance"][ok] = self.pos[j], self.normal[j], self.max_distance[j]
        P["min_dist"][ok], P["max_dist"][ok] = self.min_dist[j], self.max_dist[j]
        P["desc"][ok] = (self.desc if desc is None else desc)[j]
        P["skip"] = ~ok
        P["skip"][ok] = self.bad[j] if skip is None else np.asarray(skip)[j]
        return P

    def kf_points(self, k):
        """GetMapPointMatches of keyframe k under the initial observations: per feature an id or -1"""
        out = np.full(len(self.targets[k].feats), -1, np.int64)
        for pid, kf, f in self.obs:
            if kf == k:
                out[f] = pid
        return out


def fuse_rig(n_cam, yaw_step):
    """(R_bc, t_bc) per camera: yaws `yaw_step` apart, so that neighbouring cameras overlap"""
    out = []
    for c in range(n_cam):
        a = yaw_step * (c - 0.5 * (n_cam - 1))
        R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        out.append((R, np.array([0.05 * np.sin(a), 0.0, 0.05 * np.cos(a)])))
    return out


def fuse_cams(Rcw, tcw, n_cam):
    """FUSE_CAM_DTYPE records of float64 poses: the float quaternion, t, the intrinsics, ow = -R^T t"""
    fc = np.zeros(n_cam, FUSE_CAM_DTYPE)
    fx, fy, cx, cy = FUSE_K
    for c in range(n_cam):
        fc[c]["q_cw"], fc[c]["t_cw"] = mat_to_quat(Rcw[c]), tcw[c]
        fc[c]["fx"], fc[c]["fy"], fc[c]["cx"], fc[c]["cy"] = fx, fy, cx, cy
        fc[c]["min_x"], fc[c]["max_x"], fc[c]["min_y"], fc[c]["max_y"] = 0.0, _W, 0.0, _H
        fc[c]["ow"] = -Rcw[c].T @ tcw[c]
    return fc


def level_quotients(max_distance, pos, ow, log_sf):
    """PredictScale's quotient of every (point, camera centre) as the device forms it: float32 up to the ratio, the
    logarithm and the quotient in float64.  [n_points, n_centres]"""
    o = pos[:, None, :].astype(F) - np.asarray(ow, F)[None, :, :]
    dist = np.sqrt((o[..., 0] * o[..., 0] + o[..., 1] * o[..., 1]) + o[..., 2] * o[..., 2])
    with np.errstate(all="ignore"):
        return np.log((max_distance[:, None].astype(F) / dist).astype(np.float64)) / np.float64(F(log_sf))


def make_fuse_problem(n_kf=6, n_cam=4, n_feat=300, n_points=400, seed=0, n_levels=8, scale=1.2, bits=(0, 40),
                      see=0.7, observed=0.45, duplicates=0.04, stereo=0.6, yaw_step=np.radians(50.0), bf=40.0,
                      off_normal=0.05, settle=1e-9):
    """A seeded scene.  `n_points` scene points lie 3 to 12 m around `n_kf` keyframes whose rigs of `n_cam` overlapping
    cameras (640 x 480, yaws `yaw_step` apart) stand close together, so a point is seen by several keyframes and, near
    a seam, by two cameras of one keyframe.  A camera that sees a point gets, with probability `see`, a feature on its
    projection (0.7 px noise) whose descriptor lies up to `bits` bits from the point's and whose octave is the
    predicted level or one below; features of the last camera carry u_right = x - bf / z with probability `stereo`;
    clutter fills every camera up to `n_feat`.  Such a feature is observed by its point with probability `observed`
    (occupied), and a share `duplicates` of the points has a DUPLICATE map point (a centimetre away, a few bits off)
    that holds the feature instead in some keyframes, so lists meet occupants to replace.  Every map point's descriptor
    is ComputeDistinctiveDescriptors' choice among its observations, as local mapping leaves it.  max_distance is
    nudged until every PredictScale quotient is further than `settle` from an integer.  Returns a FuseProblem."""
    rng = np.random.default_rng([seed, 0xF05E])
    sf = scale_factors(n_levels, scale)
    sigma = (F(1.0) / (sf * sf)).astype(F)
    log_sf = F(np.log(scale))
    fx, fy, cx, cy = FUSE_K
    rig = fuse_rig(n_cam, yaw_step)
    half = 0.5 * (n_cam - 1) * yaw_step + np.radians(40.0)
    yaw, pitch = rng.uniform(-half, half, n_points), rng.uniform(-0.45, 0.45, n_points)
    rad = rng.uniform(3.0, 12.0, n_points)
    pos = np.stack([rad * np.sin(yaw) * np.cos(pitch), rad * np.sin(pitch), rad * np.cos(yaw) * np.cos(pitch)], 1)
    base = rng.integers(0, 2 ** 32, size=(n_points, 8), dtype=np.uint64).astype(np.uint32)
    lr = rng.integers(1, max(2, n_levels - 2), n_points)
    maxd = (rad * scale ** (lr - rng.uniform(0.25, 0.75, n_points))).astype(F)
    normal = pos / rad[:, None] + rng.normal(0, 0.15, (n_points, 3))
    off = rng.random(n_points) < off_normal
    normal[off] = rng.normal(0, 1.0, (int(off.sum()), 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    # ---- the keyframes' poses; max_distance settled against every camera centre
    poses = []
    for k in range(n_kf):
        R_wb, t_wb = _so3_exp(rng.normal(0, 0.05, 3)), rng.normal(0, 0.25, 3)
        Rcw, tcw = [], []
        for R_bc, t_bc in rig:
            R_wc, t_wc = R_wb @ R_bc, t_wb + R_wb @ t_bc
            Rcw.append(R_wc.T)
            tcw.append(-R_wc.T @ t_wc)
        poses.append((Rcw, tcw, fuse_cams(Rcw, tcw, n_cam)))
    centres = np.concatenate([p[2]["ow"] for p in poses])
    posf = pos.astype(F)
    for _ in range(50):
        q = level_quotients(maxd, posf, centres, log_sf)
        bad = (np.abs(q - np.round(q)) <= settle).any(axis=1)
        if not bad.any():
            break
        maxd[bad] = (maxd[bad] * F(1.0007)).astype(F)
    # ---- duplicates: ids n_points .. ; the same place within a centimetre, a few bits off
    dup_of = np.flatnonzero(rng.random(n_points) < duplicates)
    dup_id = {int(p): n_points + i for i, p in enumerate(dup_of)}
    n_ids = n_points + len(dup_of)
    all_pos = np.concatenate([posf, (pos[dup_of] + rng.normal(0, 0.01, (len(dup_of), 3))).astype(F)])
    all_normal = np.concatenate([normal, normal[dup_of]]).astype(F)
    all_maxd = np.concatenate([maxd, maxd[dup_of]])
    for _ in range(50):
        q = level_quotients(all_maxd[n_points:], all_pos[n_points:], centres, log_sf)
        bad = (np.abs(q - np.round(q)) <= settle).any(axis=1) if len(dup_of) else np.zeros(0, bool)
        if not bad.any():
            break
        all_maxd[n_points:][bad] = (all_maxd[n_points:][bad] * F(1.0007)).astype(F)
    # ---- features and observations
    targets, obs, source = [], [], []
    for k in range(n_kf):
        Rcw, tcw, fc = poses[k]
        per_cam = []
        for c in range(n_cam):
            Xc = pos @ Rcw[c].T + tcw[c]
            z = Xc[:, 2]
            with np.errstate(all="ignore"):
                u, v = fx * Xc[:, 0] / z + cx, fy * Xc[:, 1] / z + cy
            vis = np.flatnonzero((z > 0.5) & (u > 4) & (u < _W - 4) & (v > 4) & (v < _H - 4))
            vis = vis[rng.random(len(vis)) < see][:n_feat]
            ft = np.zeros(n_feat, MATCH_FEAT_DTYPE)
            src = np.full(n_feat, -1, np.int64)
            m = len(vis)
            ft["cam"] = c
            ft["x"][:m], ft["y"][:m] = u[vis] + rng.normal(0, 0.7, m), v[vis] + rng.normal(0, 0.7, m)
            dist = np.linalg.norm(pos[vis] - fc[c]["ow"].astype(float), axis=1)
            lvl = np.clip(np.ceil(np.log(maxd[vis] / dist) / np.log(scale)), 0, n_levels - 1).astype(np.int64)
            ft["octave"][:m] = np.clip(lvl - rng.integers(0, 2, m), 0, n_levels - 1)
            for i, p in enumerate(vis):
                ft["desc"][i] = flip_bits(base[p], rng.integers(bits[0], bits[1] + 1), rng)
            src[:m] = vis
            ft["x"][m:], ft["y"][m:] = rng.uniform(5, _W - 5, n_feat - m), rng.uniform(5, _H - 5, n_feat - m)
            ft["octave"][m:] = rng.integers(0, n_levels, n_feat - m)
            ft["desc"][m:] = rng.integers(0, 2 ** 32, size=(n_feat - m, 8), dtype=np.uint64).astype(np.uint32)
            ft["u_right"] = -1.0
            if c == n_cam - 1:
                st = rng.random(n_feat) < stereo
                depth = np.concatenate([z[vis], rng.uniform(3.0, 12.0, n_feat - m)])
                ft["u_right"][st] = (ft["x"] - bf / depth + rng.normal(0, 0.4, n_feat))[st]
            elif c == 0:
                ft["u_right"][rng.random(n_feat) < 0.1] = 0.0          # quirk (c) where it must not matter
            per_cam.append((ft, src))
        feats = np.concatenate([p[0] for p in per_cam])
        src = np.concatenate([p[1] for p in per_cam])
        perm = rng.permutation(len(feats))
        feats, src = feats[perm], src[perm]
        gc = match_cams(n_cam, 0.0, 0.0, _W, _H)
        cs, cf = build_grid(feats, gc)
        targets.append(Target(fc, gc, sf, sigma, cs, cf, feats, bf, log_sf))
        source.append(src)
        held = set()                                                    # a point holds one feature per (keyframe, camera)
        for f in np.flatnonzero(src >= 0):
            p, c = int(src[f]), int(feats[f]["cam"])
            r = rng.random()
            pid = p if r < observed else dup_id.get(p, -1) if r < observed + 0.35 else -1
            if pid < 0 or (pid, c) in held:
                continue
            held.add((pid, c))
            obs.append((pid, k, int(f)))
    obs = np.array(obs, np.int64).reshape(-1, 3)
    # ---- descriptors: the distinctive one of each point's observations (in keyframe, camera order), else its base
    desc = np.concatenate([base, np.stack([flip_bits(base[p], 5, rng) for p in dup_of]) if len(dup_of) else
                           np.zeros((0, 8), np.uint32)])
    by_id = {}
    for pid, k, f in obs:
        by_id.setdefault(int(pid), []).append((int(k), int(targets[k].feats[f]["cam"]), int(f)))
    for pid, lst in by_id.items():
        lst.sort()
        ds = np.stack([targets[k].feats[f]["desc"] for k, _, f in lst])
        desc[pid] = ds[distinctive_descriptor(ds)]
    return FuseProblem(targets, all_pos, all_normal, all_maxd, desc, np.zeros(n_ids, bool), obs, source, n_levels, scale)
