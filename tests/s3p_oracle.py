"""numpy restatements of the Sim3 ORBmatcher::SearchByProjection (src/ORBmatcher.cc:423-548 and :550-685) on the arrays
lba_match_sim3_project takes.

`pose_f64` is the pose chain in fp64: quaternion algebra in numpy around the C oracle's QueryPose (orc.gp_query_pose), an
implementation independent of csrc/lba_s3p_math.hpp.  `pose_float32_chain` does the SE3f products around QueryPose in
float32, the reference's precision.  From the float Tcw on everything is np.float32 in the stated operation order.
`sequential` is the loop as written, job after job.  `by_jobs` is a second route: a vectorised projection that emits
lba_match_job-shaped jobs and runs tests/match_oracle.py's LBA_MATCH_BEST on them (th_high = floor(th_low * ratio),
blocks = 1, no stereo camera); its by_rounds defines `rounds`.  `variant=` switches on one deliberate mistake
(no resolve, quirk (a) or (b) "fixed"), for the tests that show each would be caught.
"""
import math

import numpy as np

import match_oracle as mo
import orc
from amc_lba.abi import MATCH_JOB_DTYPE
from amc_lba.match import GRID_CELLS, GRID_ROWS, MATCH_BEST, Search, match_params
from amc_lba.sim3_project import (S3P_ANGLE, S3P_BEHIND, S3P_DIST, S3P_NO_CAND, S3P_NO_PREV, S3P_OK, S3P_OUT_OF_IMAGE,
                                  S3P_POSE_DTYPE, S3P_ROW_DTYPE, S3P_SKIPPED, S3P_TOO_FAR)

F = np.float32
PENDING = -1


# ---------------------------------------------------------------- fp64 pose chain
def _qn(q):
    q = np.asarray(q, np.float64)
    return q / math.sqrt(float(q @ q))


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return _qn([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _qmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _mul(A, B):
    return _qmul(A[0], B[0]), A[1] + _qmat(A[0]) @ B[1]


def _inv(A):
    qi = _qn([-A[0][0], -A[0][1], -A[0][2], A[0][3]])
    return qi, _qmat(qi) @ (-A[1])          # Sophus: R^-1 * (t * -1)


def _se3(q, t):
    return _qn(q), np.asarray(t, np.float64)


def pose_f64(kfm, hyp):
    """Tcw[c] of :445-453 as [n_cam, 12] float64 (R row-major, t), on the float inputs widened"""
    K = kfm.kf[0]
    Tbw = (_qn(hyp.q), np.asarray(hyp.t, np.float64) / np.float64(hyp.s))
    Twb = _inv(Tbw)
    Tcl = _mul(_se3(K["q"], K["t"]), _inv(_se3(K["q_prev"], K["t_prev"])))
    Twl = _mul(Twb, Tcl)
    out = np.zeros((kfm.n_cam, 12))
    for c in range(kfm.n_cam):
        C = kfm.kcams[c]
        qo, to = orc.gp_query_pose(np.eye(6), Twl[0], Twl[1], Twb[0], Twb[1], K["v_prev"].astype(float),
                                   K["v"].astype(float), float(K["stamp_prev"]), float(K["stamp"]), float(C["stamp"]))[:2]
        Tcw = _inv(_mul((_qn(qo), to), _se3(C["q_bc"], C["t_bc"])))
        out[c, :9] = _qmat(Tcw[0]).ravel()
        out[c, 9:] = Tcw[1]
    return out


# ---------------------------------------------------------------- the reference's precision: SE3f around QueryPose
def _qn32(q):
    q = np.asarray(q, F)
    n = F(np.sqrt(F(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])))
    return (q / n).astype(F)


def _qmul32(a, b):
    ax, ay, az, aw = (F(v) for v in a)
    bx, by, bz, bw = (F(v) for v in b)
    return _qn32([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                  aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _qmat32(q):
    return np.array(_qmat([F(v) for v in q]), F)


def _mul32(A, B):
    return _qmul32(A[0], B[0]), (A[1] + (_qmat32(A[0]) @ B[1]).astype(F)).astype(F)


def _inv32(A):
    qi = _qn32([-A[0][0], -A[0][1], -A[0][2], A[0][3]])
    return qi, (_qmat32(qi) @ (-A[1])).astype(F)


def pose_float32_chain(kfm, hyp):
    """[n_cam, 12] float32: Tbw, Twb, Tcl, Twl in float32, QueryPose in fp64 on their casts, its result cast to
    float32, (Twb_c * Tbc)^-1 in float32.  Not Sophus's exact operation order: the reference's PRECISION."""
    K = kfm.kf[0]
    Tbw = (_qn32(hyp.q), (np.asarray(hyp.t, F) / F(hyp.s)).astype(F))
    Twb = _inv32(Tbw)
    Tcl = _mul32((_qn32(K["q"]), K["t"].astype(F)), _inv32((_qn32(K["q_prev"]), K["t_prev"].astype(F))))
    Twl = _mul32(Twb, Tcl)
    out = np.zeros((kfm.n_cam, 12), F)
    for c in range(kfm.n_cam):
        C = kfm.kcams[c]
        qo, to = orc.gp_query_pose(np.eye(6), _qn(Twl[0]), Twl[1].astype(float), _qn(Twb[0]), Twb[1].astype(float),
                                   K["v_prev"].astype(float), K["v"].astype(float), float(K["stamp_prev"]),
                                   float(K["stamp"]), float(C["stamp"]))[:2]
        Tcw = _inv32(_mul32((_qn32(qo.astype(F)), to.astype(F)), (_qn32(C["q_bc"]), C["t_bc"].astype(F))))
        out[c, :9] = _qmat32(Tcw[0]).ravel()
        out[c, 9:] = Tcw[1]
    return out


# ---------------------------------------------------------------- settledness
def _pose_scale(tcw_d):
    """per entry of [.., 12]: 1 for the rotation's, max(1, |t|_inf) for the translation's"""
    v = np.asarray(tcw_d, np.float64).reshape(-1, 12)
    sc = np.ones_like(v)
    sc[:, 9:] = np.maximum(1.0, np.abs(v[:, 9:]).max(axis=1))[:, None]
    return sc


def pose_diff(a, b):
    """per entry |a - b| relative to the entry's scale (of b)"""
    a, b = np.asarray(a, np.float64).reshape(-1, 12), np.asarray(b, np.float64).reshape(-1, 12)
    return np.abs(a - b) / _pose_scale(b)


def pose_margin(tcw_d):
    """per entry: the distance of the fp64 value from the nearest midpoint between adjacent floats, relative to the
    entry's scale.  An entry that is exactly 0 or +-1 is exact (the identity chains: every product is of zeros and ones,
    and the host tests find the header and the restatement equal in every fp64 bit there): its margin is infinite."""
    v = np.asarray(tcw_d, np.float64).reshape(-1, 12)
    f = v.astype(F)
    up = np.nextafter(f, F(np.inf)).astype(np.float64)
    dn = np.nextafter(f, F(-np.inf)).astype(np.float64)
    fm = f.astype(np.float64)
    d = np.minimum(np.abs(v - (fm + up) / 2), np.abs(v - (fm + dn) / 2)) / _pose_scale(v)
    return np.where((v == 0) | (np.abs(v) == 1), np.inf, d)


def level_quotient(max_distance, dist, log_sf):
    with np.errstate(all="ignore"):
        ratio = F(max_distance) / F(dist)
        return np.log(np.float64(ratio)) / np.float64(F(log_sf))


def level_of(q, n_levels):
    """quirk (h): the ceil of the quotient clamped before the conversion; NaN -> 0"""
    q = np.ceil(q)
    if not q > 0:
        return 0
    if q >= n_levels:
        return n_levels - 1
    return int(q)


# ---------------------------------------------------------------- one job, float32
def job(T, C, P, kfm, prm, ow=None):
    """(status, level, x, y, radius, q): q is PredictScale's quotient (None before it).  T [12] float32."""
    T = np.asarray(T, F)
    z0 = F(0.0)
    if P["skip"]:
        return S3P_SKIPPED, -1, z0, z0, z0, None
    px, py, pz = (F(v) for v in P["pos"])
    with np.errstate(all="ignore"):
        X = ((T[0] * px + T[1] * py) + T[2] * pz) + T[9]
        Y = ((T[3] * px + T[4] * py) + T[5] * pz) + T[10]
        Z = ((T[6] * px + T[7] * py) + T[8] * pz) + T[11]
        if Z < 0:
            return S3P_BEHIND, -1, z0, z0, z0, None
        fx, fy, cx, cy = (F(C[k]) for k in ("fx", "fy", "cx", "cy"))
        if prm.proj_form == 0:
            u, v = fx * X / Z + cx, fy * Y / Z + cy
        else:
            invz = F(1.0) / Z
            u, v = fx * (X * invz) + cx, fy * (Y * invz) + cy
        if not (u >= C["min_x"] and u < C["max_x"] and v >= C["min_y"] and v < C["max_y"]):
            return S3P_OUT_OF_IMAGE, -1, u, v, z0, None
        o = C["ow"] if ow is None else ow
        ox, oy, oz = px - F(o[0]), py - F(o[1]), pz - F(o[2])
        dist = np.sqrt((ox * ox + oy * oy) + oz * oz)
        if dist < P["min_dist"] or dist > P["max_dist"]:
            return S3P_DIST, -1, u, v, z0, None
        nx, ny, nz = (F(a) for a in P["normal"])
        if (ox * nx + oy * ny) + oz * nz < F(0.5) * dist:
            return S3P_ANGLE, -1, u, v, z0, None
        q = level_quotient(P["max_distance"], dist, kfm.kf[0]["log_scale_factor"])
    lvl = level_of(q, int(kfm.kf[0]["n_levels"]))
    return PENDING, lvl, u, v, F(prm.th) * F(kfm.sf[lvl]), q


def gate_quantities(T, C, P, prm):
    """for the float32-chain comparison: (Z, u - min_x, max_x - u, v - min_y, max_y - v) in float64 from a float32 T"""
    T = np.asarray(T, np.float64)
    p = np.asarray(P["pos"], np.float64)
    X, Y, Z = T[0:3] @ p + T[9], T[3:6] @ p + T[10], T[6:9] @ p + T[11]
    with np.errstate(all="ignore"):
        u, v = C["fx"] * X / Z + C["cx"], C["fy"] * Y / Z + C["cy"]
    return Z, u, v


class Result:
    def __init__(self, n_points, n_cam, n_feat):
        self.rows = np.zeros((n_points, n_cam), S3P_ROW_DTYPE)
        self.rows["feat"], self.rows["best_dist"], self.rows["level"] = -1, 256, -1
        self.feat_point = np.full(n_feat, -1, np.int32)
        self.poses = np.zeros(n_cam, S3P_POSE_DTYPE)
        self.quot = np.full((n_points, n_cam), np.nan)
        self.n_matches = 0

    def same(self, o, rounds=False):
        keys = ("status", "feat", "best_dist", "level")
        ok = all((self.rows[k] == o.rows[k]).all() for k in keys)
        ok = ok and all((self.rows[k].view(np.uint32) == o.rows[k].view(np.uint32)).all() for k in ("x", "y", "radius"))
        ok = ok and (self.feat_point == o.feat_point).all() and self.n_matches == int(o.n_matches)
        ok = ok and (self.poses["tcw"].view(np.uint32) == o.poses["tcw"].view(np.uint32)).all()
        return bool(ok and (not rounds or (self.poses["rounds"] == o.poses["rounds"]).all()))


def _ints(desc):
    return [int.from_bytes(np.ascontiguousarray(d).tobytes(), "little") for d in desc]


def _fill_poses(res, kfm, hyp, tcw):
    res.poses["tcw_d"] = pose_f64(kfm, hyp)
    res.poses["tcw"] = res.poses["tcw_d"].astype(F) if tcw is None else tcw


def _threshold_ok(best, prm):
    return F(best) <= F(prm.th_low) * F(prm.ratio_hamming)


def sequential(kfm, hyp, prm, tcw=None, variant=None):
    """the loop as written.  tcw: a float32 [n_cam, 12] to use instead of the fp64 chain's rounding.
    variant: None, "no_resolve" (vpMatched is never updated), "fix_a" (PO from the corrected pose's centre),
    "fix_b" (a point that matched stops at that camera)."""
    n_cam, nf = kfm.n_cam, len(kfm.feats)
    res = Result(len(hyp.points), n_cam, nf)
    if not kfm.kf[0]["has_prev"]:
        res.rows["status"] = S3P_NO_PREV
        return res
    _fill_poses(res, kfm, hyp, tcw)
    taken = np.zeros(nf, bool) if hyp.taken is None else hyp.taken.astype(bool).copy()
    fd, pd = _ints(kfm.feats["desc"]), _ints(hyp.points["desc"])
    fx, fy, fo = kfm.feats["x"], kfm.feats["y"], kfm.feats["octave"]
    ows = None
    if variant == "fix_a":                      # the centre of the corrected pose: -R^T t
        ows = [(-(res.poses["tcw_d"][c][:9].reshape(3, 3).T @ res.poses["tcw_d"][c][9:])).astype(F) for c in range(n_cam)]
    for p, P in enumerate(hyp.points):
        for c in range(n_cam):
            st, lvl, u, v, r, q = job(res.poses["tcw"][c], kfm.kcams[c], P, kfm, prm, None if ows is None else ows[c])
            R = res.rows[p, c]
            R["status"], R["level"], R["x"], R["y"], R["radius"] = st, lvl, u, v, r
            if st != PENDING:
                continue
            res.quot[p, c] = q
            best, idx, n = 256, -1, 0
            rect = mo.cell_rect(u, v, r, kfm.gcams[c])
            if rect is not None:
                for ix in range(rect[0], rect[1] + 1):
                    for iy in range(rect[2], rect[3] + 1):
                        cell = c * GRID_CELLS + ix * GRID_ROWS + iy
                        for f in kfm.cell_feat[kfm.cell_start[cell]:kfm.cell_start[cell + 1]]:
                            f = int(f)
                            if not (abs(F(fx[f]) - u) < r and abs(F(fy[f]) - v) < r):
                                continue
                            if taken[f] or fo[f] < lvl - 1 or fo[f] > lvl:
                                continue
                            n += 1
                            d = bin(fd[f] ^ pd[p]).count("1")
                            if d < best:
                                best, idx = d, f
            R["best_dist"] = best
            if n == 0:
                R["status"] = S3P_NO_CAND
            elif _threshold_ok(best, prm):
                R["status"], R["feat"] = S3P_OK, idx
                res.feat_point[idx] = p
                if variant != "no_resolve":
                    taken[idx] = True
                res.n_matches += 1
                if variant == "fix_b":
                    res.rows["status"][p, c + 1:] = S3P_SKIPPED
                    break
            else:
                R["status"] = S3P_TOO_FAR
    return res


def project_all(kfm, hyp, prm, tcw):
    """the projection of every (point, camera), vectorised in float32: dict of [n_points, n_cam] arrays"""
    P, C = hyp.points, kfm.kcams
    n, n_cam = len(P), kfm.n_cam
    T = np.asarray(tcw, F)[None, :, :]
    px, py, pz = (P["pos"][:, i:i + 1].astype(F) for i in range(3))
    with np.errstate(all="ignore"):
        X = ((T[..., 0] * px + T[..., 1] * py) + T[..., 2] * pz) + T[..., 9]
        Y = ((T[..., 3] * px + T[..., 4] * py) + T[..., 5] * pz) + T[..., 10]
        Z = ((T[..., 6] * px + T[..., 7] * py) + T[..., 8] * pz) + T[..., 11]
        fx, fy, cx, cy = (C[k][None, :] for k in ("fx", "fy", "cx", "cy"))
        if prm.proj_form == 0:
            u, v = fx * X / Z + cx, fy * Y / Z + cy
        else:
            invz = F(1.0) / Z
            u, v = fx * (X * invz) + cx, fy * (Y * invz) + cy
        inside = (u >= C["min_x"][None]) & (u < C["max_x"][None]) & (v >= C["min_y"][None]) & (v < C["max_y"][None])
        ox, oy, oz = (P["pos"][:, i:i + 1] - C["ow"][None, :, i] for i in range(3))
        dist = np.sqrt((ox * ox + oy * oy) + oz * oz)
        dist_ok = ~((dist < P["min_dist"][:, None]) | (dist > P["max_dist"][:, None]))
        dot = (ox * P["normal"][:, 0:1] + oy * P["normal"][:, 1:2]) + oz * P["normal"][:, 2:3]
        angle_ok = ~(dot < F(0.5) * dist)
        quot = np.log((P["max_distance"][:, None] / dist).astype(np.float64)) / np.float64(kfm.kf[0]["log_scale_factor"])
    status = np.full((n, n_cam), PENDING, np.int32)
    status[~angle_ok] = S3P_ANGLE
    status[~dist_ok] = S3P_DIST
    status[~inside] = S3P_OUT_OF_IMAGE
    status[Z < 0] = S3P_BEHIND
    status[P["skip"] != 0, :] = S3P_SKIPPED
    nl = int(kfm.kf[0]["n_levels"])
    level = np.array([[level_of(q, nl) for q in row] for row in quot], np.int64).reshape(n, n_cam)
    return dict(status=status, u=u.astype(F), v=v.astype(F), level=level, quot=quot, Z=Z, dist=dist, dot=dot)


def by_jobs(kfm, hyp, prm, tcw=None):
    """the second route: (Result with rounds, the Search handed to match_oracle, its params, the live (p, c) list)"""
    n_cam, nf = kfm.n_cam, len(kfm.feats)
    res = Result(len(hyp.points), n_cam, nf)
    if not kfm.kf[0]["has_prev"]:
        res.rows["status"] = S3P_NO_PREV
        return res, None, None, []
    _fill_poses(res, kfm, hyp, tcw)
    pr = project_all(kfm, hyp, prm, res.poses["tcw"])
    st = pr["status"]
    reached = (st != S3P_SKIPPED) & (st != S3P_BEHIND)
    res.rows["status"] = st
    res.rows["x"], res.rows["y"] = np.where(reached, pr["u"], F(0)), np.where(reached, pr["v"], F(0))
    live = st == PENDING
    res.rows["level"] = np.where(live, pr["level"], -1)
    res.rows["radius"] = np.where(live, F(prm.th) * kfm.sf[np.where(live, pr["level"], 0)], F(0))
    res.quot = np.where(live, pr["quot"], np.nan)
    p, c = np.nonzero(live)                              # point-major, cameras inner
    jobs = np.zeros(len(p), MATCH_JOB_DTYPE)
    jobs["x"], jobs["y"], jobs["radius"] = res.rows["x"][p, c], res.rows["y"][p, c], res.rows["radius"][p, c]
    jobs["cam"], jobs["min_level"], jobs["max_level"] = c, pr["level"][p, c] - 1, pr["level"][p, c]
    jobs["point"], jobs["blocks"], jobs["desc"] = p, 1, hyp.points["desc"][p]
    feats = kfm.feats.copy()
    feats["taken"] = 0 if hyp.taken is None else hyp.taken
    s = Search(kfm.gcams, kfm.cell_start, kfm.cell_feat, feats, jobs)
    th_high = int(math.floor(float(F(prm.th_low) * F(prm.ratio_hamming))))
    mp = match_params(MATCH_BEST, n_cam, th_high=th_high, stereo_cam=-1, ur_truncate=0, check_orientation=0)
    cands = mo.candidates(s, mp)
    r = mo.by_rounds(s, mp, cands)
    assert r.same_outputs(mo.sequential(s, mp, cands))
    res.rows["status"][p, c] = r.status
    res.rows["feat"][p, c] = r.feat
    res.rows["best_dist"][p, c] = r.best_dist
    has = r.job >= 0
    res.feat_point[has] = p[r.job[has]]
    res.n_matches = r.n_matches
    res.poses["rounds"] = r.rounds
    return res, s, mp, list(zip(p.tolist(), c.tolist()))
