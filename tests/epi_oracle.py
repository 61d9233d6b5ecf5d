"""Two independent numpy restatements of ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:947-1131, with
Pinhole::project and Pinhole::epipolarConstrain) for one (keyframe, neighbour) pair on the arrays of lba_match_epipolar:

  sequential   the merge walk with lower_bound and the shrinking bestDist, line for line, in fp64 or in float32 (the
               reference's precision: float tables and gates, the `3.84 * unc` comparison in double);
  by_argmin    per idx1, over all eligible candidates of its node with dist <= th_low that pass both gates, the minimum
               distance and the LAST index of the ties.

Their agreement (tests/test_epi_cases.py) is what licenses any parallel form.  `settled` is the rule of
tests/test_tri_cases.py on every gate comparison of every eligible candidate with dist <= th_low."""
from collections import namedtuple

import numpy as np

OK, HAS_POINT, NOT_STEREO, NO_NODE, NO_MATCH, ROT = range(6)
SETTLE = 1e-9
HISTO = 30
_POP = np.array([bin(i).count("1") for i in range(65536)], np.int64)

Job = namedtuple("Job", "f1 f2 fv1 fv2 cams1 cams2 n_cam prm")          # fv: (node_id, node_start, node_feat) of a keyframe
Result = namedtuple("Result", "idx2 dist status n_matches")
PRM = dict(th_low=50, only_stereo=0, coarse=0, check_orientation=0)


def jobs_of(c):
    """the pairs of a case (tests/epi_cases.py: the arrays of the call) as Jobs"""
    out = []
    for P in c.pairs:
        side = []
        for k in (int(P["kf1"]), int(P["kf2"])):
            E = c.ekfs[k]
            ids = c.node_id[E["node0"]:E["node0"] + E["n_node"]]
            st = c.node_start[E["node0"]:E["node0"] + E["n_node"] + 1] if E["n_node"] else np.zeros(1, np.int32)
            nf = c.node_feat[E["nf0"]:E["nf0"] + st[-1]]
            cams = c.cams[c.kfs[k]["cam0"]:c.kfs[k]["cam0"] + c.n_cam]
            side.append((c.feats[E["feat0"]:E["feat0"] + E["n_feat"]], (ids, st, nf), cams))
        out.append(Job(side[0][0], side[1][0], side[0][1], side[1][1], side[0][2], side[1][2], c.n_cam, dict(PRM, **c.prm)))
    return out


def hamming(d1, d2):
    """the 256-bit distance of d1 [8] to every row of d2 [n, 8]"""
    x = np.bitwise_xor(np.asarray(d2, np.uint32), np.asarray(d1, np.uint32)[None, :])
    return (_POP[x & 0xFFFF] + _POP[x >> 16]).sum(axis=1)


def _mul33(A, B, dt):
    C = np.zeros((3, 3), dt)
    for i in range(3):
        for j in range(3):
            C[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
    return C


def table(c1, c2, dt=np.float64):
    """(F12 [3, 3], ep [2]) of KF1's camera record c1 and KF2's c2, every operation in dt"""
    T1, T2 = np.asarray(c1["Tcw"], dt).reshape(3, 4), np.asarray(c2["Tcw"], dt).reshape(3, 4)
    O1, O2 = np.asarray(c1["Ow"], dt), np.asarray(c2["Ow"], dt)
    R1, R2 = T1[:, :3], T2[:, :3]
    with np.errstate(all="ignore"):
        R12 = _mul33(R1, R2.T, dt)
        t12 = np.array([((R1[i, 0] * O2[0] + R1[i, 1] * O2[1]) + R1[i, 2] * O2[2]) + T1[i, 3] for i in range(3)], dt)
        z, one = dt(0), dt(1)
        tx = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], dt)
        fx1, fy1, cx1, cy1 = (dt(c1[k]) for k in ("fx", "fy", "cx", "cy"))
        fx2, fy2, cx2, cy2 = (dt(c2[k]) for k in ("fx", "fy", "cx", "cy"))
        K1it = np.array([[one / fx1, z, z], [z, one / fy1, z], [-cx1 / fx1, -cy1 / fy1, one]], dt)
        K2i = np.array([[one / fx2, z, -cx2 / fx2], [z, one / fy2, -cy2 / fy2], [z, z, one]], dt)
        F = _mul33(_mul33(_mul33(K1it, tx, dt), R12, dt), K2i, dt)
        C2 = np.array([((R2[i, 0] * O1[0] + R2[i, 1] * O1[1]) + R2[i, 2] * O1[2]) + T2[i, 3] for i in range(3)], dt)
        ep = np.array([fx2 * C2[0] / C2[2] + cx2, fy2 * C2[1] / C2[2] + cy2], dt)
    return F, ep


def tables(job, dt=np.float64, swap=False):
    """[c1][c2] -> (F12, ep); swap=True indexes them (c2, c1): what a transposed table would be"""
    T = [[table(job.cams1[a], job.cams2[b], dt) for b in range(job.n_cam)] for a in range(job.n_cam)]
    return [[T[b][a] for b in range(job.n_cam)] for a in range(job.n_cam)] if swap else T


def is_stereo(f, n_cam):
    return bool(f["cam"] == n_cam - 1 and f["u_right"] >= 0)


def _rel(lhs, rhs):
    """relative distance of a comparison from its gate; a non-finite side is settled (inf)"""
    lhs, rhs = float(lhs), float(rhs)
    if not (np.isfinite(lhs) and np.isfinite(rhs)):
        return np.inf
    m = max(abs(lhs), abs(rhs))
    return abs(lhs - rhs) / m if m else 0.0


def near_epipole(ep, f2, dt):
    """(skipped, margin, (lhs, rhs)) of :1049-1052"""
    with np.errstate(all="ignore"):
        ex, ey = ep[0] - dt(f2["x"]), ep[1] - dt(f2["y"])
        lhs, rhs = ex * ex + ey * ey, dt(100) * dt(f2["scale"])
    return bool(lhs < rhs), _rel(lhs, rhs), (float(lhs), float(rhs))


def epi_gate(F, f1, f2, dt, unc=None):
    """(passed, margin, (lhs, rhs)) of Pinhole::epipolarConstrain; the last comparison in double, as `dsqr < 3.84 * unc` is.
    den == 0 is settled when a and b are both exactly 0, or den > 0."""
    x1, y1, x2, y2 = dt(f1["x"]), dt(f1["y"]), dt(f2["x"]), dt(f2["y"])
    unc = f2["sigma2"] if unc is None else unc
    with np.errstate(all="ignore"):
        a = (x1 * F[0, 0] + y1 * F[1, 0]) + F[2, 0]
        b = (x1 * F[0, 1] + y1 * F[1, 1]) + F[2, 1]
        c = (x1 * F[0, 2] + y1 * F[1, 2]) + F[2, 2]
        num = (a * x2 + b * y2) + c
        den = a * a + b * b
        if den == 0:
            return False, (np.inf if (a == 0 and b == 0) else 0.0), (np.nan, np.nan)
        dsqr = num * num / den
        rhs = 3.84 * float(np.float32(unc))
    return bool(float(dsqr) < rhs), _rel(dsqr, rhs), (float(dsqr), rhs)


def rot_bin(a1, a2):
    f = np.float32
    rot = f(a1) - f(a2)
    if rot < 0:
        rot = f(rot + f(360.0))
    v = f(rot * (f(1.0) / f(HISTO)))
    b = int(np.sign(v) * np.floor(np.abs(v) + f(0.5)))     # C's round()
    return 0 if b == HISTO else b


def three_maxima(h):
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(h):
        if s > max1:
            max3, max2, max1, i3, i2, i1 = max2, max1, s, i2, i1, i
        elif s > max2:
            max3, max2, i3, i2 = max2, s, i2, i
        elif s > max3:
            max3, i3 = s, i
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        i2 = i3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        i3 = -1
    return i1, i2, i3


def _finish(job, idx2, dist, status):
    """nmatches and the rotation pass (:1098-1117): the bins that ARE the maxima lose their matches (quirk c)"""
    n = int((status == OK).sum())
    if job.prm["check_orientation"]:
        ok = np.flatnonzero(status == OK)
        bins = np.array([rot_bin(job.f1["angle"][i], job.f2["angle"][idx2[i]]) for i in ok], np.int64)
        maxima = three_maxima(np.bincount(bins, minlength=HISTO)) if len(ok) else (-1, -1, -1)
        for i, b in zip(ok, bins):
            if b in maxima:
                status[i] = ROT
                n -= 1
    return Result(idx2, dist, status, n)


def _lower_bound(ids, lo, key):
    return lo + int(np.searchsorted(ids[lo:], key, side="left"))


def sequential(job, dt=np.float64, gate=True, tie="last", kp1_sigma=False, swap=False):
    """The function as written.  The variants are what a wrong device would compute: gate=False drops the epipolar
    gate, tie="first" skips on `dist >= bestDist`, kp1_sigma uses kp1's level sigma2, swap the (c2, c1) tables."""
    p, n_cam = job.prm, job.n_cam
    T = tables(job, dt, swap)
    n1 = len(job.f1)
    idx2_out, dist_out = np.full(n1, -1, np.int64), np.full(n1, p["th_low"], np.int64)
    status = np.full(n1, NO_NODE, np.int64)
    (id1, s1, nf1), (id2, s2, nf2) = job.fv1, job.fv2
    a = b = 0
    while a < len(id1) and b < len(id2):
        if id1[a] == id2[b]:
            l2 = nf2[s2[b]:s2[b + 1]]
            for idx1 in nf1[s1[a]:s1[a + 1]]:
                k1 = job.f1[idx1]
                if k1["has_point"]:
                    status[idx1] = HAS_POINT
                    continue
                st1 = is_stereo(k1, n_cam)
                if p["only_stereo"] and not st1:
                    status[idx1] = NOT_STEREO
                    continue
                best_dist, best_idx2 = p["th_low"], -1
                d = hamming(k1["desc"], job.f2["desc"][l2]) if len(l2) else []
                for k, idx2 in enumerate(l2):
                    k2 = job.f2[idx2]
                    if k2["has_point"]:
                        continue
                    st2 = is_stereo(k2, n_cam)
                    if p["only_stereo"] and not st2:
                        continue
                    dist = int(d[k])
                    if dist > p["th_low"] or (dist >= best_dist if tie == "first" and best_idx2 >= 0 else dist > best_dist):
                        continue
                    F, ep = T[int(k1["cam"])][int(k2["cam"])]
                    if not st1 and not st2 and near_epipole(ep, k2, dt)[0]:
                        continue
                    if p["coarse"] or not gate or epi_gate(F, k1, k2, dt, k1["sigma2"] if kp1_sigma else None)[0]:
                        best_idx2, best_dist = int(idx2), dist
                idx2_out[idx1], dist_out[idx1] = best_idx2, best_dist
                status[idx1] = OK if best_idx2 >= 0 else NO_MATCH
            a += 1
            b += 1
        elif id1[a] < id2[b]:
            a = _lower_bound(id1, a, id2[b])
        else:
            b = _lower_bound(id2, b, id1[a])
    return _finish(job, idx2_out, dist_out, status)


def candidates(job, dt=np.float64):
    """Per idx1 of a common node that searches: [(idx2, dist, passes, margin, [(lhs, rhs) per comparison])] over ALL eligible candidates of its node
    with dist <= th_low, in list order; margin: the smallest relative distance of its comparisons from their gates."""
    p, n_cam = job.prm, job.n_cam
    T = tables(job, dt)
    (id1, s1, nf1), (id2, s2, nf2) = job.fv1, job.fv2
    pos2 = {int(n): k for k, n in enumerate(id2)}
    st2 = np.array([is_stereo(f, n_cam) for f in job.f2], bool)
    elig2 = (job.f2["has_point"] == 0) & (st2 if p["only_stereo"] else True)
    out = {}
    for a, node in enumerate(id1):
        b = pos2.get(int(node))
        if b is None:
            continue
        l2 = nf2[s2[b]:s2[b + 1]]
        l2 = l2[elig2[l2]] if len(l2) else l2
        for idx1 in nf1[s1[a]:s1[a + 1]]:
            k1 = job.f1[idx1]
            st1 = is_stereo(k1, n_cam)
            if k1["has_point"] or (p["only_stereo"] and not st1):
                continue
            rows = []
            d = hamming(k1["desc"], job.f2["desc"][l2]) if len(l2) else np.zeros(0, np.int64)
            for k in np.flatnonzero(d <= p["th_low"]):
                k2 = job.f2[l2[k]]
                F, ep = T[int(k1["cam"])][int(k2["cam"])]
                ok, margin, vals = True, np.inf, []
                if not st1 and not st2[l2[k]]:
                    skip, margin, v = near_epipole(ep, k2, dt)
                    ok = not skip
                    vals.append(v)
                if not p["coarse"]:
                    g, m, v = epi_gate(F, k1, k2, dt)
                    ok, margin = ok and g, min(margin, m)
                    vals.append(v)
                rows.append((int(l2[k]), int(d[k]), ok, margin, vals))
            out[int(idx1)] = rows
    return out


def by_argmin(job, dt=np.float64, cands=None):
    p = job.prm
    n1 = len(job.f1)
    idx2, dist, status = np.full(n1, -1, np.int64), np.full(n1, p["th_low"], np.int64), np.full(n1, NO_NODE, np.int64)
    common = set(int(n) for n in job.fv1[0]) & set(int(n) for n in job.fv2[0])
    id1, s1, nf1 = job.fv1
    st1 = np.array([is_stereo(f, job.n_cam) for f in job.f1], bool)
    for a, node in enumerate(id1):
        if int(node) in common:
            l1 = nf1[s1[a]:s1[a + 1]]
            status[l1] = np.where(job.f1["has_point"][l1] != 0, HAS_POINT,
                                  np.where(~st1[l1] if p["only_stereo"] else False, NOT_STEREO, NO_MATCH))
    for idx1, rows in (candidates(job, dt) if cands is None else cands).items():
        good = [(d, k, i2) for k, (i2, d, ok, _, _) in enumerate(rows) if ok]
        if good:
            dmin = min(g[0] for g in good)
            idx2[idx1], dist[idx1], status[idx1] = [g[2] for g in good if g[0] == dmin][-1], dmin, OK
    return _finish(job, idx2, dist, status)


def margins(job, dt=np.float64, cands=None):
    """per keypoint of KF1 the smallest margin of its comparisons (inf where it has none)"""
    m = np.full(len(job.f1), np.inf)
    for idx1, rows in (candidates(job, dt) if cands is None else cands).items():
        if rows:
            m[idx1] = min(r[3] for r in rows)
    return m


def settled(job, cands=None):
    """per keypoint of KF1: every gate comparison of every eligible candidate with dist <= th_low lies further than
    1e-9 relative from its gate (non-finite sides and a den of exactly zero operands count as settled)"""
    return margins(job, np.float64, cands) > SETTLE
