"""numpy restatements of ORBmatcher::Fuse's search (src/ORBmatcher.cc:1133-1316 and :1318-1437) on the arrays
lba_match_fuse takes, and a small faithful map to run the whole of Fuse on.

`sequential` is the loop as written, job after job, every float expression in np.float32 in the stated order.
`vectorised` is a second route: the projection of every (point, camera) at once, then per live job an arg-min over
the camera's features in cell_feat order (a cell's index is ix * 48 + iy, so that order IS GetFeaturesInArea's walk
order for any rectangle).  `variant=` switches on one deliberate mistake ("ties_last", "no_error_gate",
"matrix_rotation") for the tests that count the rows each would change.

`ToyMap` is the map: observations per (keyframe, camera), AddObservation's nObs rule with the stereo + 2, Replace
(src/MapPoint.cc:392-469) with ComputeDistinctiveDescriptors (:498-578), ReplaceMapPointMatch / EraseMapPointMatch.
It iterates a point's keyframes by keyframe id where the reference iterates a std::map keyed by POINTER: the order in
which ComputeDistinctiveDescriptors lists descriptors, and so which of two equally good ones it picks, follows the
allocator there and the id here.  `fuse_sequential` is the whole Fuse run directly on a ToyMap, search and tail in one
loop as the reference has it.
"""
import copy

import numpy as np

import match_oracle as mo
from amc_lba.abi import FUSE_ROW_DTYPE
from amc_lba.fuse import (FUSE_ANGLE, FUSE_BEHIND, FUSE_DIST, FUSE_KF, FUSE_NO_CAMERA, FUSE_NO_CAND, FUSE_OK,
                          FUSE_OUT_OF_IMAGE, FUSE_SIM3, FUSE_SKIPPED, FUSE_TOO_FAR, TH_LOW)
from amc_lba.match import GRID_CELLS, GRID_ROWS

F = np.float32
PENDING = -1
INT_MAX = 2 ** 31 - 1


def level_quotient(max_distance, dist, log_sf):
    with np.errstate(all="ignore"):
        ratio = F(max_distance) / F(dist)
        return np.log(np.float64(ratio)) / np.float64(F(log_sf))


def level_of(q, n_levels):
    q = np.ceil(q)
    if not q > 0:
        return 0
    if q >= n_levels:
        return n_levels - 1
    return int(q)


def rotate(q, p, matrix=False):
    """vTcw[c].so3() * p in float32: Sophus' operator* (so3.hpp:358-367), or (variant) the rotation matrix's rows"""
    qx, qy, qz, qw = (F(v) for v in q)
    px, py, pz = (F(v) for v in p)
    if matrix:
        two = F(2.0)
        R = [[F(1) - two * (qy * qy + qz * qz), two * (qx * qy - qz * qw), two * (qx * qz + qy * qw)],
             [two * (qx * qy + qz * qw), F(1) - two * (qx * qx + qz * qz), two * (qy * qz - qx * qw)],
             [two * (qx * qz - qy * qw), two * (qy * qz + qx * qw), F(1) - two * (qx * qx + qy * qy)]]
        return tuple((r[0] * px + r[1] * py) + r[2] * pz for r in R)
    ux, uy, uz = qy * pz - qz * py, qz * px - qx * pz, qx * py - qy * px
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    wx, wy, wz = qy * uz - qz * uy, qz * ux - qx * uz, qx * uy - qy * ux
    return (px + qw * ux) + wx, (py + qw * uy) + wy, (pz + qw * uz) + wz


def job(tg, c, P, mode, th, variant=None):
    """(status, level, x, y, radius, ur, quotient) of one (point, camera) up to its window"""
    z0 = F(0.0)
    C = tg.fcams[c]
    if mode == FUSE_SIM3 and c >= tg.n_cam - 1:
        return FUSE_NO_CAMERA, -1, z0, z0, z0, z0, None
    if P["skip"]:
        return FUSE_SKIPPED, -1, z0, z0, z0, z0, None
    with np.errstate(all="ignore"):
        rx, ry, rz = rotate(C["q_cw"], P["pos"], variant == "matrix_rotation")
        X, Y, Z = rx + C["t_cw"][0], ry + C["t_cw"][1], rz + C["t_cw"][2]
        if Z < 0:
            return FUSE_BEHIND, -1, z0, z0, z0, z0, None
        invz = F(1.0) / Z
        u, v = C["fx"] * X / Z + C["cx"], C["fy"] * Y / Z + C["cy"]
        if not (u >= C["min_x"] and u < C["max_x"] and v >= C["min_y"] and v < C["max_y"]):
            return FUSE_OUT_OF_IMAGE, -1, u, v, z0, z0, None
        ur = u - F(tg.bf) * invz
        px, py, pz = (F(a) for a in P["pos"])
        ox, oy, oz = px - C["ow"][0], py - C["ow"][1], pz - C["ow"][2]
        dist = np.sqrt((ox * ox + oy * oy) + oz * oz)
        if dist < P["min_dist"] or dist > P["max_dist"]:
            return FUSE_DIST, -1, u, v, z0, ur, None
        nx, ny, nz = (F(a) for a in P["normal"])
        if (ox * nx + oy * ny) + oz * nz < F(0.5) * dist:
            return FUSE_ANGLE, -1, u, v, z0, ur, None
        q = level_quotient(P["max_distance"], dist, tg.log_scale_factor)
    lvl = level_of(q, tg.n_levels)
    return PENDING, lvl, u, v, F(th) * F(tg.sf[lvl]), ur, q


def error_gate(tg, mode, last_cam, u, v, ur, fx, fy, u_right, octave, variant=None):
    """True: the feature passes the chi-square gate of overload 1 (always in overload 2)"""
    if mode != FUSE_KF or variant == "no_error_gate":
        return True
    ex, ey = F(u) - F(fx), F(v) - F(fy)
    inv = F(tg.sigma[octave])
    if last_cam and F(u_right) >= 0:
        er = F(ur) - F(u_right)
        e2 = (ex * ex + ey * ey) + er * er
        return not np.float64(e2 * inv) > 7.8
    e2 = ex * ex + ey * ey
    return not np.float64(e2 * inv) > 5.99


def decide(mode, n, best, idx, th_low):
    """(status, feat, best_dist) of a walked job"""
    if n == 0:
        return FUSE_NO_CAND, -1, 256
    if mode == FUSE_KF and best >= 256:
        return FUSE_TOO_FAR, -1, 256
    return (FUSE_OK if best <= th_low else FUSE_TOO_FAR), idx, best


def _ints(desc):
    return [int.from_bytes(np.ascontiguousarray(d).tobytes(), "little") for d in desc]


def new_rows(n, n_cam):
    rows = np.zeros((n, n_cam), FUSE_ROW_DTYPE)
    rows["feat"], rows["best_dist"], rows["level"] = -1, 256, -1
    return rows


def one_job(tg, c, P, mode, th, th_low=TH_LOW, variant=None, fd=None):
    """the whole of one job as the reference's loops run it: (row record, quotient)"""
    R = new_rows(1, 1)[0, 0]
    st, lvl, u, v, r, ur, q = job(tg, c, P, mode, th, variant)
    R["status"], R["level"], R["x"], R["y"], R["radius"] = st, lvl, u, v, r
    if st != PENDING:
        return R, q
    fd = _ints(tg.feats["desc"]) if fd is None else fd
    pd = int.from_bytes(np.ascontiguousarray(P["desc"]).tobytes(), "little")
    ft = tg.feats
    best, idx, n = (256 if mode == FUSE_KF else INT_MAX), -1, 0
    rect = mo.cell_rect(u, v, r, tg.gcams[c])
    if rect is not None:
        for ix in range(rect[0], rect[1] + 1):
            for iy in range(rect[2], rect[3] + 1):
                cell = c * GRID_CELLS + ix * GRID_ROWS + iy
                for f in tg.cell_feat[tg.cell_start[cell]:tg.cell_start[cell + 1]]:
                    f = int(f)
                    if not (abs(F(ft["x"][f]) - u) < r and abs(F(ft["y"][f]) - v) < r):
                        continue
                    o = int(ft["octave"][f])
                    if o < lvl - 1 or o > lvl:
                        continue
                    if not error_gate(tg, mode, c == tg.n_cam - 1, u, v, ur, ft["x"][f], ft["y"][f], ft["u_right"][f], o,
                                      variant):
                        continue
                    n += 1
                    d = bin(fd[f] ^ pd).count("1")
                    if d < best or (variant == "ties_last" and d == best and d < 256):
                        best, idx = d, f
    R["status"], R["feat"], R["best_dist"] = decide(mode, n, best, idx, th_low)
    R["n_cand"] = n
    return R, q


def sequential(tg, points, mode, th, th_low=TH_LOW, variant=None):
    """the loop as written: (rows [n_points, n_cam], quotients [n_points, n_cam] (NaN where not reached))"""
    rows, quot = new_rows(len(points), tg.n_cam), np.full((len(points), tg.n_cam), np.nan)
    fd = _ints(tg.feats["desc"])
    for p, P in enumerate(points):
        for c in range(tg.n_cam):
            rows[p, c], q = one_job(tg, c, P, mode, th, th_low, variant, fd)
            if q is not None:
                quot[p, c] = q
    return rows, quot


_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def vectorised(tg, points, mode, th, th_low=TH_LOW):
    """the second route: rows [n_points, n_cam]"""
    n, n_cam = len(points), tg.n_cam
    rows = new_rows(n, n_cam)
    if n == 0:
        return rows
    C, P = tg.fcams, points
    q = C["q_cw"].astype(F)[None, :, :]
    qx, qy, qz, qw = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    px, py, pz = (P["pos"][:, i:i + 1].astype(F) for i in range(3))
    with np.errstate(all="ignore"):
        ux, uy, uz = qy * pz - qz * py, qz * px - qx * pz, qx * py - qy * px
        ux, uy, uz = ux + ux, uy + uy, uz + uz
        wx, wy, wz = qy * uz - qz * uy, qz * ux - qx * uz, qx * uy - qy * ux
        X = ((px + qw * ux) + wx) + C["t_cw"][None, :, 0]
        Y = ((py + qw * uy) + wy) + C["t_cw"][None, :, 1]
        Z = ((pz + qw * uz) + wz) + C["t_cw"][None, :, 2]
        u, v = C["fx"][None] * X / Z + C["cx"][None], C["fy"][None] * Y / Z + C["cy"][None]
        ur = u - F(tg.bf) * (F(1.0) / Z)
        inside = (u >= C["min_x"][None]) & (u < C["max_x"][None]) & (v >= C["min_y"][None]) & (v < C["max_y"][None])
        ox, oy, oz = (P["pos"][:, i:i + 1] - C["ow"][None, :, i] for i in range(3))
        dist = np.sqrt((ox * ox + oy * oy) + oz * oz)
        dist_ok = ~((dist < P["min_dist"][:, None]) | (dist > P["max_dist"][:, None]))
        dot = (ox * P["normal"][:, 0:1] + oy * P["normal"][:, 1:2]) + oz * P["normal"][:, 2:3]
        angle_ok = ~(dot < F(0.5) * dist)
        quot = np.log((P["max_distance"][:, None] / dist).astype(np.float64)) / np.float64(F(tg.log_scale_factor))
    st = np.full((n, n_cam), PENDING, np.int32)
    st[~angle_ok] = FUSE_ANGLE
    st[~dist_ok] = FUSE_DIST
    st[~inside] = FUSE_OUT_OF_IMAGE
    st[Z < 0] = FUSE_BEHIND
    st[P["skip"] != 0, :] = FUSE_SKIPPED
    if mode == FUSE_SIM3:
        st[:, n_cam - 1] = FUSE_NO_CAMERA
    reached = (st != FUSE_SKIPPED) & (st != FUSE_BEHIND) & (st != FUSE_NO_CAMERA)
    live = st == PENDING
    level = np.array([[level_of(x, tg.n_levels) for x in r] for r in quot], np.int64).reshape(n, n_cam)
    rows["status"] = st
    rows["x"], rows["y"] = np.where(reached, u, F(0)).astype(F), np.where(reached, v, F(0)).astype(F)
    rows["level"] = np.where(live, level, -1)
    rows["radius"] = np.where(live, F(th) * tg.sf[np.where(live, level, 0)], F(0))
    # the camera's features in walk order
    ft = tg.feats
    fbytes = ft["desc"].view(np.uint8).reshape(len(ft), 32)
    for c in range(n_cam):
        order = tg.cell_feat[tg.cell_start[c * GRID_CELLS]:tg.cell_start[(c + 1) * GRID_CELLS]].astype(np.int64)
        cell = np.repeat(np.arange(GRID_CELLS), np.diff(tg.cell_start[c * GRID_CELLS:(c + 1) * GRID_CELLS + 1]))
        cix, ciy = cell // GRID_ROWS, cell % GRID_ROWS
        fx, fy, fo, fur = ft["x"][order], ft["y"][order], ft["octave"][order], ft["u_right"][order]
        inv = tg.sigma[np.minimum(fo, tg.n_levels - 1)]
        for p in np.flatnonzero(live[:, c]):
            R = rows[p, c]
            x, y, r, lv = R["x"], R["y"], R["radius"], int(R["level"])
            rect = mo.cell_rect(x, y, r, tg.gcams[c])
            if rect is None:
                R["status"] = FUSE_NO_CAND
                continue
            m = (cix >= rect[0]) & (cix <= rect[1]) & (ciy >= rect[2]) & (ciy <= rect[3])
            m &= (np.abs(fx - x) < r) & (np.abs(fy - y) < r) & (fo >= lv - 1) & (fo <= lv)
            if mode == FUSE_KF:
                ex, ey = x - fx, y - fy
                e2m = ex * ex + ey * ey
                mono_ok = ~((e2m * inv).astype(np.float64) > 5.99)
                if c == n_cam - 1:
                    er = ur[p, c] - fur
                    e2s = e2m + er * er
                    st_ok = ~((e2s * inv).astype(np.float64) > 7.8)
                    m &= np.where(fur >= 0, st_ok, mono_ok)
                else:
                    m &= mono_ok
            k = np.flatnonzero(m)
            if len(k) == 0:
                R["status"] = FUSE_NO_CAND
                continue
            d = _POP[fbytes[order[k]] ^ P["desc"][p].view(np.uint8)[None, :]].sum(axis=1)
            i = int(np.argmin(d))                                      # the first of the smallest
            R["status"], R["feat"], R["best_dist"] = decide(mode, len(k), int(d[i]), int(order[k[i]]), th_low)
            R["n_cand"] = len(k)
    return rows


def same_rows(a, b):
    return bool(all((a[k] == b[k]).all() for k in ("status", "feat", "best_dist", "level", "n_cand")) and
                all((a[k].view(np.uint32) == b[k].view(np.uint32)).all() for k in ("x", "y", "radius")))


def diff_rows(a, b):
    """how many rows differ in status, feat or best_dist"""
    return int(((a["status"] != b["status"]) | (a["feat"] != b["feat"]) | (a["best_dist"] != b["best_dist"])).sum())


# ---------------------------------------------------------------- the map
class ToyPoint:
    def __init__(self, desc):
        self.obs = {}            # keyframe -> [feature per camera, -1: none]  (mObservations)
        self.n_obs = 0           # nObs: NOT reset by Replace
        self.bad = False
        self.replaced = -1
        self.desc = np.array(desc, np.uint32)


class ToyMap:
    """kfs: {keyframe id: (cam [n_feat], u_right [n_feat], desc [n_feat, 8])}; n_cam is the map's nCamera"""

    def __init__(self, n_cam, kfs, descs):
        self.n_cam = n_cam
        self.kfs = kfs
        self.mp = {k: np.full(len(v[0]), -1, np.int64) for k, v in kfs.items()}      # mvpMapPoints
        self.pts = [ToyPoint(d) for d in descs]

    @classmethod
    def from_problem(cls, prob):
        kfs = {k: (t.feats["cam"].copy(), t.feats["u_right"].copy(), t.feats["desc"].copy())
               for k, t in enumerate(prob.targets)}
        m = cls(prob.targets[0].n_cam, kfs, prob.desc)
        for pid, kf, f in prob.obs:
            m.add(int(pid), int(kf), int(f))
        for pid in np.flatnonzero(prob.bad):
            m.pts[pid].bad = True
        return m

    def copy(self):
        return copy.deepcopy(self)

    # ---- the interface fuse_walk uses
    def is_bad(self, pid):
        return self.pts[pid].bad

    def in_camera(self, pid, kf, c):
        o = self.pts[pid].obs.get(kf)
        return o is not None and o[c] != -1

    def points_of(self, kf):
        """GetMapPoints: the keyframe's points that are not bad"""
        return set(int(i) for i in self.mp[kf] if i >= 0 and not self.pts[i].bad)

    def occupant(self, kf, f):
        return int(self.mp[kf][f])

    def observations(self, pid):
        return self.pts[pid].n_obs

    def descriptor(self, pid):
        return self.pts[pid].desc

    def add(self, pid, kf, f):
        """pMP->AddObservation(pKF, idx); pKF->AddMapPoint(pMP, idx)"""
        self._add_observation(pid, kf, f)
        self.mp[kf][f] = pid

    def _add_observation(self, pid, kf, f):
        P = self.pts[pid]
        idx = list(P.obs.get(kf, [-1] * self.n_cam))
        cam = int(self.kfs[kf][0][f])
        idx[cam] = f
        P.obs[kf] = idx
        P.n_obs += 2 if (cam == self.n_cam - 1 and self.kfs[kf][1][f] >= 0) else 1

    def replace(self, loser, winner):
        """self[loser].Replace(self[winner]) (src/MapPoint.cc:392-469)"""
        if loser == winner:
            return
        L, Wn = self.pts[loser], self.pts[winner]
        obs = L.obs
        obsmp = {k: list(v) for k, v in Wn.obs.items()}                      # the copy taken on entry
        L.obs = {}
        L.bad = True
        L.replaced = winner
        for kf in sorted(obs):
            if kf not in obsmp:
                for i in obs[kf]:
                    if i != -1:
                        self.mp[kf][i] = winner
                        self._add_observation(winner, kf, i)
            else:
                for c in range(self.n_cam):
                    i = obs[kf][c]
                    if i == -1:
                        continue
                    if obsmp[kf][c] != -1:
                        self.mp[kf][i] = -1
                    else:
                        self.mp[kf][i] = winner
                        self._add_observation(winner, kf, i)
        self.compute_distinctive_descriptors(winner)

    def compute_distinctive_descriptors(self, pid):
        P = self.pts[pid]
        if P.bad or not P.obs:
            return
        ds = [self.kfs[kf][2][i] for kf in sorted(P.obs) for i in P.obs[kf] if i != -1]
        if not ds:
            return
        ints = _ints(ds)
        n = len(ints)
        best, best_i = INT_MAX, 0
        for i in range(n):
            d = sorted(bin(ints[i] ^ ints[j]).count("1") for j in range(n))
            med = d[int(0.5 * (n - 1))]
            if med < best:
                best, best_i = med, i
        P.desc = np.array(ds[best_i], np.uint32)

    def state(self):
        """everything the property compares: observations, occupants, bad flags, nObs, descriptors"""
        return ([(sorted((k, tuple(v)) for k, v in P.obs.items()), P.n_obs, P.bad, P.replaced, P.desc.tobytes())
                 for P in self.pts], {k: v.tobytes() for k, v in self.mp.items()})


def live_point(prob, m, pid):
    """the S3P_POINT_DTYPE entry of a point as the reference reads it at this moment (skip 0: the loop is past it)"""
    P = prob.points([pid], skip=np.zeros(prob.n_ids, bool))
    P["desc"][0] = m.pts[pid].desc
    return P[0]


def fuse_sequential(m, prob, kf, tg, list_ids, mode, th, th_low=TH_LOW):
    """One ORBmatcher::Fuse call directly on the ToyMap `m`: keyframe id `kf` with Target `tg`, the list of ids (-1:
    NULL).  Returns (nFused, vpReplacePoint or None)."""
    fd = _ints(tg.feats["desc"])
    n_fused = 0
    if mode == FUSE_KF:
        for pid in list_ids:
            pid = int(pid)
            if pid < 0 or m.is_bad(pid):
                continue
            for c in range(tg.n_cam):
                if m.in_camera(pid, kf, c):
                    continue
                R, _ = one_job(tg, c, live_point(prob, m, pid), mode, th, th_low, None, fd)
                if R["status"] != FUSE_OK:
                    continue
                occ = m.occupant(kf, int(R["feat"]))
                if occ >= 0:
                    if not m.is_bad(occ):
                        if m.observations(occ) > m.observations(pid):
                            m.replace(pid, occ)
                        else:
                            m.replace(occ, pid)
                else:
                    m.add(pid, kf, int(R["feat"]))
                n_fused += 1
        return n_fused, None
    found = m.points_of(kf)
    rep = np.full(len(list_ids), -1, np.int64)
    for i, pid in enumerate(list_ids):
        pid = int(pid)
        if m.is_bad(pid) or pid in found:
            continue
        for c in range(tg.n_cam - 1):
            R, _ = one_job(tg, c, live_point(prob, m, pid), mode, th, th_low, None, fd)
            if R["status"] != FUSE_OK:
                continue
            occ = m.occupant(kf, int(R["feat"]))
            if occ >= 0:
                if not m.is_bad(occ):
                    rep[i] = occ
            else:
                m.add(pid, kf, int(R["feat"]))
            n_fused += 1
    return n_fused, rep
