"""Numpy restatement of Sim3Solver's RANSAC (src/Sim3Solver.cc: ComputeSim3 :343-459, CheckInliers / Project /
FromCameraToImage :462-536, iterate :250-326), independent of csrc/, vectorised over hypotheses and rows.

dtype=float64 is what the device is held to: the reference's formulas in double on the float-valued inputs.
dtype=float32 is the reference-faithful run: every array operation in float32, double only where the reference uses
`double`: the entries of N, `ang`, `nom / den`.  (The reference's Eigen::EigenSolver is restated by numpy's symmetric
solver in the same precision.)

Besides the flags it returns, per hypothesis, the relative eigen-gap (l1 - l2) / |l1| and, per (hypothesis, row), the
gate margin min(|err1 - max1| / max1, |err2 - max2| / max2): what decides whether another precision may disagree.
"""
import numpy as np

DEGENERATE = 1e-5


def _quat_rot(q, T):
    """rotation matrices [..., 3, 3] of unit quaternions [..., 4] (x, y, z, w), Eigen's toRotationMatrix, in dtype T"""
    q = np.asarray(q, T)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two = T(2)
    R = np.empty(q.shape[:-1] + (3, 3), T)
    R[..., 0, 0] = 1 - two * (y * y + z * z); R[..., 0, 1] = two * (x * y - w * z); R[..., 0, 2] = two * (x * z + w * y)
    R[..., 1, 0] = two * (x * y + w * z); R[..., 1, 1] = 1 - two * (x * x + z * z); R[..., 1, 2] = two * (y * z - w * x)
    R[..., 2, 0] = two * (x * z - w * y); R[..., 2, 1] = two * (y * z + w * x); R[..., 2, 2] = 1 - two * (x * x + y * y)
    return R


def _so3_exp(v, T):
    """Sophus::SO3::exp(v).matrix() for rotation vectors [..., 3] in dtype T (Rodrigues)"""
    v = np.asarray(v, T)
    th = np.sqrt((v * v).sum(-1))[..., None, None]
    K = np.zeros(v.shape[:-1] + (3, 3), T)
    K[..., 0, 1], K[..., 0, 2] = -v[..., 2], v[..., 1]
    K[..., 1, 0], K[..., 1, 2] = v[..., 2], -v[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -v[..., 1], v[..., 0]
    with np.errstate(all="ignore"):
        a = np.where(th > 0, np.sin(th) / th, T(1))
        b = np.where(th > 0, (1 - np.cos(th)) / (th * th), T(0.5))
    return (np.eye(3, dtype=T) + a * K + b * (K @ K)).astype(T)


def cameras(cams, T):
    """(R [n, 3, 3], t [n, 3], fx, fy, cx, cy [n]) of lba_sim3_cam rows in dtype T (the quaternion normalised in double)"""
    q = np.asarray(cams["q"], np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return (_quat_rot(q, np.float64).astype(T), np.asarray(cams["t"], T), np.asarray(cams["fx"], T), np.asarray(cams["fy"], T),
            np.asarray(cams["cx"], T), np.asarray(cams["cy"], T))


def _project(cam, idx, Y):
    """pi(Tcb[idx] Y) for Y [..., n, 3] and per-row camera indices idx [n]: pinhole, no depth test"""
    R, t, fx, fy, cx, cy = cam
    Xc = np.einsum("nij,...nj->...ni", R[idx], Y) + t[idx]
    with np.errstate(all="ignore"):
        return np.stack([fx[idx] * Xc[..., 0] / Xc[..., 2] + cx[idx], fy[idx] * Xc[..., 1] / Xc[..., 2] + cy[idx]], -1)


def hypotheses(rows, tri, fix_scale, dtype=np.float64):
    """ComputeSim3 for every triple [H, 3] of `rows`: dict of q [H, 4] (x, y, z, w; w >= 0), R, t, s, degenerate, gap"""
    T = np.dtype(dtype).type
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    H = len(tri)
    P1 = np.asarray(rows["X1b"], T)[tri]          # [H, point, coordinate]
    P2 = np.asarray(rows["X2b"], T)[tri]
    O1 = ((P1[:, 0] + P1[:, 1]) + P1[:, 2]) / T(3)
    O2 = ((P2[:, 0] + P2[:, 1]) + P2[:, 2]) / T(3)
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    M = np.zeros((H, 3, 3), T)
    for k in range(3):
        M = M + Pr2[:, k, :, None] * Pr1[:, k, None, :]
    Md = M.astype(np.float64)                      # `double N11 ...` (:363-376)
    N = np.zeros((H, 4, 4))
    N[:, 0, 0] = Md[:, 0, 0] + Md[:, 1, 1] + Md[:, 2, 2]
    N[:, 0, 1] = Md[:, 1, 2] - Md[:, 2, 1]
    N[:, 0, 2] = Md[:, 2, 0] - Md[:, 0, 2]
    N[:, 0, 3] = Md[:, 0, 1] - Md[:, 1, 0]
    N[:, 1, 1] = Md[:, 0, 0] - Md[:, 1, 1] - Md[:, 2, 2]
    N[:, 1, 2] = Md[:, 0, 1] + Md[:, 1, 0]
    N[:, 1, 3] = Md[:, 2, 0] + Md[:, 0, 2]
    N[:, 2, 2] = -Md[:, 0, 0] + Md[:, 1, 1] - Md[:, 2, 2]
    N[:, 2, 3] = Md[:, 1, 2] + Md[:, 2, 1]
    N[:, 3, 3] = -Md[:, 0, 0] - Md[:, 1, 1] + Md[:, 2, 2]
    N = N + np.triu(N, 1).transpose(0, 2, 1)
    N = N.astype(T)                                # Eigen::Matrix4f N
    finite = np.isfinite(N).all((1, 2))
    zero = (N == 0).all((1, 2))
    lam = np.full((H, 4), np.nan, T)
    vec = np.full((H, 4, 4), np.nan, T)
    solve = finite & ~zero
    if solve.any():
        lam[solve], vec[solve] = np.linalg.eigh(N[solve])
    e = vec[:, :, 3]                               # ascending: the last is the largest
    e[zero] = (1, 0, 0, 0)                         # N = 0: the first unit vector (maxCoeff takes the first maximum)
    lam[zero] = 0
    with np.errstate(all="ignore"):
        gap = ((lam[:, 3] - lam[:, 2]) / np.abs(lam[:, 3])).astype(np.float64)
        e = e / np.sqrt((e * e).sum(-1, keepdims=True))
        e = np.where(e[:, :1] < 0, -e, e)
        nv = np.sqrt((e[:, 1:] ** 2).sum(-1))
        degenerate = nv < T(DEGENERATE)
        q = np.concatenate([e[:, 1:], e[:, :1]], 1)
        if T is np.float64:
            R = _quat_rot(q, T)
        else:                                      # ang in double, the rotation vector and SO3::exp in float (:397-415)
            ang = np.arctan2(nv.astype(np.float64), e[:, 0].astype(np.float64))
            rv = (2 * ang[:, None] * e[:, 1:].astype(np.float64) / nv[:, None].astype(np.float64)).astype(T)
            R = _so3_exp(rv, T)
        P3 = np.einsum("hij,hkj->hki", R, Pr2)
        nom = (Pr1 * P3).sum((1, 2))
        den = (P3 * P3).sum((1, 2))
        s = np.ones(H, T) if fix_scale else (nom.astype(np.float64) / den.astype(np.float64)).astype(T)
        t = O1 - s[:, None] * np.einsum("hij,hj->hi", R, O2)
    return {"q": q, "R": R, "t": t, "s": s, "degenerate": degenerate, "gap": gap}


def errors(hyp, rows, cams, n_cam, dtype=np.float64):
    """CheckInliers' err1, err2 [H, n] of every hypothesis on every row (cams: the pair's 2 n_cam rows)"""
    T = np.dtype(dtype).type
    cam1, cam2 = cameras(cams[:n_cam], T), cameras(cams[n_cam:2 * n_cam], T)
    i1, i2 = np.asarray(rows["cam1"], np.int64), np.asarray(rows["cam2"], np.int64)
    X1, X2 = np.asarray(rows["X1b"], T), np.asarray(rows["X2b"], T)
    R, t, s = hyp["R"], hyp["t"], hyp["s"]
    with np.errstate(all="ignore"):
        sR = s[:, None, None] * R
        sRi = (T(1) / s)[:, None, None] * R.transpose(0, 2, 1)
        ti = -np.einsum("hij,hj->hi", sRi, t)
        p11, p22 = _project(cam1, i1, X1), _project(cam2, i2, X2)
        p21 = _project(cam1, i1, np.einsum("hij,nj->hni", sR, X2) + t[:, None])
        p12 = _project(cam2, i2, np.einsum("hij,nj->hni", sRi, X1) + ti[:, None])
        d1, d2 = p11[None] - p21, p12 - p22[None]
        return (d1 * d1).sum(-1), (d2 * d2).sum(-1)


def select(counts, degenerate, min_inliers):
    """iterate()'s loop (:272-325) over the counts, degenerate hypotheses skipped: (best_hyp, n_inliers, converged)"""
    best, best_n = -1, 0
    for h, c in enumerate(counts):
        if degenerate[h]:
            continue
        if c >= best_n:
            best, best_n = h, int(c)
            if c > min_inliers:
                return best, best_n, 1
    return best, best_n, 0


def run(pair, rows, tri, cams, n_cam, dtype=np.float64):
    """One pair: rows = its lba_s3r_corr rows, tri = its triples, cams = its 2 n_cam cameras.  Returns the hypotheses'
    dict extended by err1, err2, inlier [H, n], count [H], nonfinite [H], margin [H, n] and best_hyp, n_inliers,
    converged, row_inlier [n]."""
    T = np.dtype(dtype).type
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    hyp = hypotheses(rows, tri, bool(pair["fix_scale"]), dtype)
    e1, e2 = errors(hyp, rows, cams, n_cam, dtype)
    m1, m2 = np.asarray(rows["max_err1"], T), np.asarray(rows["max_err2"], T)
    with np.errstate(all="ignore"):
        inl = (e1 < m1) & (e2 < m2) & ~hyp["degenerate"][:, None]
        g1 = np.where(np.isfinite(e1), np.abs(e1 - m1) / m1, np.inf)
        g2 = np.where(np.isfinite(e2), np.abs(e2 - m2) / m2, np.inf)
    count = inl.sum(1)
    best, n_in, conv = select(count, hyp["degenerate"], int(pair["min_inliers"]))
    finite = np.isfinite(hyp["q"]).all(1) & np.isfinite(hyp["t"]).all(1) & np.isfinite(hyp["s"])
    hyp.update(err1=e1, err2=e2, gate1=g1.astype(np.float64), gate2=g2.astype(np.float64), inlier=inl, count=count,
               margin=np.minimum(g1, g2).astype(np.float64), nonfinite=~finite, best_hyp=best, n_inliers=n_in, converged=conv,
               row_inlier=inl[best].astype(np.int32) if best >= 0 else np.zeros(len(rows), np.int32))
    return hyp


def settled(res, pair, m, gap_min=1e-6):
    """Settledness of an fp64 run `res`: flag_ok [H, n] (gate margin > m, or a degenerate hypothesis's all-zero row),
    transform_ok [H] (eigen-gap >= gap_min, finite, not degenerate) and whether the selection survives forcing every
    unsettled flag to 0 and to 1."""
    flag_ok = (res["margin"] > m) | res["degenerate"][:, None]
    with np.errstate(invalid="ignore"):
        transform_ok = (res["gap"] >= gap_min) & ~res["degenerate"] & ~res["nonfinite"]
    nominal = (res["best_hyp"], res["converged"])
    sel_ok = True
    for force in (False, True):
        inl = np.where(flag_ok, res["inlier"], force)
        b, _, c = select(inl.sum(1), res["degenerate"], int(pair["min_inliers"]))
        sel_ok = sel_ok and (b, c) == nominal
    return flag_ok, transform_ok, sel_ok
