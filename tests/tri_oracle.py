"""numpy restatement of one match of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:408-587, with
GeometricTools::Triangulate and MultiKeyFrame::UnprojectStereo), written from the reference's behaviour, with
numpy.linalg.svd for the 4 x 4.

`run(..., precision="f64")` is what the device is held to: double arithmetic on the float-valued inputs.
`run(..., precision="f32")` is the reference's precision: every operation in np.float32, float cos / atan2, the
double constants (5.991, 7.8, 0.9998) applied as the reference's mixed expressions do.

Per row the result also carries every comparison evaluated, as (name, lhs, rhs, exact): `exact` marks a comparison of
an input as given (ur >= 0, depth > 0), in which no arithmetic can differ between two evaluations; and the singular
values of A (NaN where the row was not triangulated).
"""
import numpy as np

(OK, PARALLAX, W_ZERO, NO_DEPTH, BEHIND1, BEHIND2, REPROJ1, REPROJ2, DIST_ZERO, FAR, SCALE) = range(11)
SETTLED = 1e-9


class Result:
    def __init__(self, n):
        self.status = np.full(n, -1, np.int32)
        self.stereo = np.zeros(n, np.int32)
        self.X = np.full((n, 3), np.nan)
        self.sigma = np.full((n, 4), np.nan)
        self.cmp = [[] for _ in range(n)]
        self.triangulated = np.zeros(n, bool)
        self.n_new = None
        self.n_stereo = None


def build_A(xn1, T1, xn2, T2):
    """GeometricTools.cc:50-53; T [3, 4]"""
    return np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])


def _norm3(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _row(r, c1, c2, last1, last2, kf1, kf2, F, ratio_factor, far_points, th_far, cmps):
    """one match; returns (status, stereo_point, X or None, sigma or None)"""
    f64 = F is np.float64

    def cmp(name, lhs, rhs, exact=False):
        cmps.append((name, float(lhs), float(rhs), exact))

    def g(rec, name):   # a float-valued input in the working precision
        return np.asarray(rec[name], F)

    T1, T2 = g(c1, "Tcw").reshape(3, 4), g(c2, "Tcw").reshape(3, 4)
    z1, z2, ur1, ur2 = g(r, "z1"), g(r, "z2"), F(r["ur1"]), F(r["ur2"])
    cmp("ur1>=0", ur1, 0.0, True)
    cmp("ur2>=0", ur2, 0.0, True)
    stereo1, stereo2 = bool(ur1 >= 0), bool(ur2 >= 0)
    xn1 = np.array([(z1[0] - F(c1["cx"])) / F(c1["fx"]), (z1[1] - F(c1["cy"])) / F(c1["fy"]), F(1)], F)
    xn2 = np.array([(z2[0] - F(c2["cx"])) / F(c2["fx"]), (z2[1] - F(c2["cy"])) / F(c2["fy"]), F(1)], F)
    ray1, ray2 = T1[:, :3].T @ xn1, T2[:, :3].T @ xn2
    cos_rays = F(ray1 @ ray2) / (_norm3(ray1) * _norm3(ray2))
    cs1 = cs2 = cos_rays + F(1)

    def cos_stereo(b, depth):
        return np.cos(F(2) * np.arctan2(F(b) / F(2), F(depth)))

    if stereo1:
        cs1 = cos_stereo(kf1["b"], r["depth1"])
    elif stereo2:
        cs2 = cos_stereo(kf2["b"], r["depth2"])
    cs = cs2 if cs2 < cs1 else cs1
    if stereo1 or stereo2:   # otherwise both are the same number
        cmp("min(cs1,cs2)", cs2, cs1)
    cmp("cosRays<cosStereo", cos_rays, cs)
    cmp("cosRays>0", cos_rays, 0.0)
    tri = bool(cos_rays < cs) and bool(cos_rays > 0)
    if tri and not (stereo1 or stereo2):
        cmp("cosRays<0.9998", cos_rays, 0.9998)
        tri = float(cos_rays) < 0.9998
    stereo_point, sigma = 0, None
    if tri:
        A = build_A(xn1, T1, xn2, T2).astype(F)
        if not np.isfinite(A).all():
            return W_ZERO, 0, None, None
        _, sigma, Vt = np.linalg.svd(A)
        x3Dh = Vt[3]
        if x3Dh[3] == 0 or not np.isfinite(x3Dh[3]):
            return W_ZERO, 0, None, sigma
        X = (x3Dh[:3] / x3Dh[3]).astype(F)
    else:
        def unproject(k, depth, last, kf):
            z = F(depth)
            cmp("depth>0", z, 0.0, True)
            if not z > 0:
                return None
            x = (F(k[0]) - F(last["cx"])) * z * F(last["invfx"])
            y = (F(k[1]) - F(last["cy"])) * z * F(last["invfy"])
            return (g(kf, "Rwb").reshape(3, 3) @ np.array([x, y, z], F) + g(kf, "twb")).astype(F)

        if stereo1:
            cmp("cs1<cs2", cs1, cs2)
        if stereo1 and cs1 < cs2:
            stereo_point, X = 1, unproject(r["k1"], r["depth1"], last1, kf1)
        else:
            if stereo2:
                cmp("cs2<cs1", cs2, cs1)
            if stereo2 and cs2 < cs1:
                stereo_point, X = 1, unproject(r["k2"], r["depth2"], last2, kf2)
            else:
                return PARALLAX, 0, None, None
        if X is None:
            return NO_DEPTH, 1, None, None

    def cam_point(T):
        return [((T[i, 0] * X[0] + T[i, 1] * X[1]) + T[i, 2] * X[2]) + T[i, 3] for i in range(3)]

    x1, y1, d1 = cam_point(T1)
    cmp("z1<=0", d1, 0.0)
    if d1 <= 0:
        return BEHIND1, stereo_point, None, sigma
    x2, y2, d2 = cam_point(T2)
    cmp("z2<=0", d2, 0.0)
    if d2 <= 0:
        return BEHIND2, stereo_point, None, sigma

    def reproj_fails(side, c, kf, x, y, z, kp, ur, stereo, sigma2):
        fx, fy, cx, cy = F(c["fx"]), F(c["fy"]), F(c["cx"]), F(c["cy"])
        if not stereo:
            ex, ey = (fx * x / z + cx) - kp[0], (fy * y / z + cy) - kp[1]
            lhs, rhs = ex * ex + ey * ey, 5.991 * float(F(sigma2))      # float lhs against a double product
        else:
            invz = F(1) / z
            u, v = fx * x * invz + cx, fy * y * invz + cy
            ex, ey, er = u - kp[0], v - kp[1], (u - F(kf["bf"]) * invz) - ur
            lhs, rhs = ex * ex + ey * ey + er * er, 7.8 * float(F(sigma2))
        cmp(f"reproj{side}", lhs, rhs)
        return float(lhs) > rhs

    if reproj_fails(1, c1, kf1, x1, y1, d1, z1, ur1, stereo1, r["sigma2_1"]):
        return REPROJ1, stereo_point, None, sigma
    if reproj_fails(2, c2, kf2, x2, y2, d2, z2, ur2, stereo2, r["sigma2_2"]):
        return REPROJ2, stereo_point, None, sigma
    dist1, dist2 = _norm3(X - g(c1, "Ow")), _norm3(X - g(c2, "Ow"))
    cmp("dist1==0", dist1, 0.0)
    cmp("dist2==0", dist2, 0.0)
    if dist1 == 0 or dist2 == 0:
        return DIST_ZERO, stereo_point, None, sigma
    if far_points:
        cmp("dist1>=thFar", dist1, F(th_far))
        cmp("dist2>=thFar", dist2, F(th_far))
        if dist1 >= F(th_far) or dist2 >= F(th_far):
            return FAR, stereo_point, None, sigma
    ratio_dist, ratio_octave = dist2 / dist1, F(r["scale1"]) / F(r["scale2"])
    rf = F(ratio_factor)
    cmp("ratio*f<octave", ratio_dist * rf, ratio_octave)
    cmp("ratio>octave*f", ratio_dist, ratio_octave * rf)
    if ratio_dist * rf < ratio_octave or ratio_dist > ratio_octave * rf:
        return SCALE, stereo_point, None, sigma
    assert f64 or X.dtype == np.float32
    return OK, stereo_point, X, sigma


def run(pairs, rows, kfs, cams, n_cam, ratio_factor=1.5 * 1.2, far_points=0, th_far=0.0, precision="f64"):
    """Every row of every pair, in pair order (rows shared by two pairs carry the later pair's result)."""
    F = {"f64": np.float64, "f32": np.float32}[precision]
    res = Result(len(rows))
    res.n_new, res.n_stereo = np.zeros(len(pairs), np.int32), np.zeros(len(pairs), np.int32)
    with np.errstate(all="ignore"):
        for p, P in enumerate(pairs):
            kf1, kf2 = kfs[P["kf1"]], kfs[P["kf2"]]
            for i in range(int(P["row0"]), int(P["row0"] + P["n_rows"])):
                r = rows[i]
                c1, c2 = cams[kf1["cam0"] + r["cam1"]], cams[kf2["cam0"] + r["cam2"]]
                last1, last2 = cams[kf1["cam0"] + n_cam - 1], cams[kf2["cam0"] + n_cam - 1]
                cmps = []
                st, sp, X, sigma = _row(r, c1, c2, last1, last2, kf1, kf2, F, ratio_factor, far_points, th_far, cmps)
                res.status[i], res.stereo[i], res.cmp[i] = st, sp, cmps
                res.X[i] = X if X is not None else np.nan
                res.sigma[i] = sigma if sigma is not None else np.nan
                res.triangulated[i] = sigma is not None
                res.n_new[p] += st == OK
                res.n_stereo[p] += st == OK and sp
    return res


def margin(cmps):
    """the smallest relative distance of a row's computed comparisons from their gates (inf without any).  A comparison
    with a NaN side is false however it is evaluated, and one with an infinite side is as far from its gate as can
    be: neither counts."""
    m = np.inf
    for _, lhs, rhs, exact in cmps:
        scale = max(abs(lhs), abs(rhs))
        if exact or not np.isfinite(scale):
            continue
        m = min(m, abs(lhs - rhs) / scale if scale > 0 else 0.0)
    return m


def settled(res, tol=SETTLED):
    """per row: every computed comparison has |lhs - rhs| > tol max(|lhs|, |rhs|)"""
    return np.array([margin(c) > tol for c in res.cmp], bool)
