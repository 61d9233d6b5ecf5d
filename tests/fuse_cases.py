"""Named cases for lba_match_fuse: the smallest shapes at which k_fuse can go wrong.  case(name) returns a Case: its
targets, its shared points, its searches (target, point0, n_points) and `expect`, the property it is named for, per
mode: {mode: {field: flat list over the searches' rows}} (a field that is absent is not part of the property).

Unless a case says otherwise every camera of a target has the identity pose (q = (0, 0, 0, 1), t = 0, ow = 0) with
fx = fy = 256, c = (320, 240) and a 640 x 480 image: a point (X, Y, 4) then projects to u = 64 X + 320, v = 64 Y + 240
EXACTLY (every operation of the rotation adds or multiplies a zero or a one; 256 X / 4 is a scaling by a power of two),
so windows, ties and gate equalities are placed to the bit.  The cameras of one target see the same points and hold
different features.  max_distance = dist * 1.2^(level - 0.5) puts PredictScale's quotient half a level from an integer.

Settledness: PredictScale's quotient must keep M_LEVEL (tests/s3p_cases.py: the same function, the same bound) from an
integer; it is the only rounding-decided quantity, the float-versus-double literal comparisons are exact in the header
and in the restatement.  tests/test_fuse_cases.py checks it for every case and every GPU seed.
"""
import numpy as np

from amc_lba.abi import FUSE_CAM_DTYPE, MATCH_FEAT_DTYPE
from amc_lba.fuse import (FUSE_KF, FUSE_SIM3, FUSE_STATUS_NAMES, TH_KF, TH_SIM3, Target, make_fuse_problem)
from amc_lba.match import build_grid, flip_bits, match_cams, scale_factors
from amc_lba.sim3_project import S3P_POINT_DTYPE
from s3p_cases import M_LEVEL

F = np.float32
FX, CX, CY, W, H = 256.0, 320.0, 240.0, 640.0, 480.0
N_LEVELS, SCALE = 8, 1.2
LOG_SF = F(np.log(SCALE))
SF = scale_factors(N_LEVELS, SCALE)
SIGMA = (F(1.0) / (SF * SF)).astype(F)
BF = 40.0
MODES = (FUSE_KF, FUSE_SIM3)
TH = {FUSE_KF: TH_KF, FUSE_SIM3: TH_SIM3}
GPU_SEEDS = (0, 1, 2)
_cache = {}


class Case:
    def __init__(self, targets, points, searches, expect=None, note=""):
        self.targets, self.points, self.searches = targets, np.ascontiguousarray(points, S3P_POINT_DTYPE), searches
        self.expect, self.note = expect or {}, note

    def specs(self, mode):
        return [(t, p0, n, mode, TH[mode]) for t, p0, n in self.searches]


def D(seed):
    return np.random.default_rng([seed, 0xD35C]).integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)


def near(desc, bits, seed=0):
    return flip_bits(desc, bits, np.random.default_rng([seed, bits, 0xF11B]))


def feat(cam, x, y, octave, desc, u_right=-1.0):
    return (cam, x, y, octave, desc, u_right)


def target(n_cam, feats, gmin_x=0.0, bf=BF):
    """identity poses; feats: a list of feat(...) in index order"""
    fc = np.zeros(n_cam, FUSE_CAM_DTYPE)
    fc["q_cw"][:, 3] = 1.0
    fc["fx"], fc["fy"], fc["cx"], fc["cy"] = FX, FX, CX, CY
    fc["max_x"], fc["max_y"] = W, H
    ft = np.zeros(len(feats), MATCH_FEAT_DTYPE)
    for i, (cam, x, y, o, d, ur) in enumerate(feats):
        ft[i]["cam"], ft[i]["x"], ft[i]["y"], ft[i]["octave"], ft[i]["desc"], ft[i]["u_right"] = cam, x, y, o, d, ur
    gc = match_cams(n_cam, gmin_x, 0.0, W, H)
    cs, cf = build_grid(ft, gc)
    return Target(fc, gc, SF, SIGMA, cs, cf, ft, bf, LOG_SF)


def point(u, v, level, desc, z=4.0, skip=0, normal=None):
    """a point that projects to (u, v) exactly at depth z in an identity camera, predicted level `level`"""
    P = np.zeros(1, S3P_POINT_DTYPE)
    X, Y = F((u - CX) * z / FX), F((v - CY) * z / FX)
    P["pos"][0] = (X, Y, z)
    x, y, zz = P["pos"][0]
    dist = np.sqrt((x * x + y * y) + zz * zz)
    P["normal"][0] = (P["pos"][0] / dist) if normal is None else normal
    P["max_distance"] = F(float(dist) * SCALE ** (level - 0.5))
    P["min_dist"], P["max_dist"] = F(0.05) * dist, F(50.0) * dist
    P["desc"][0], P["skip"] = desc, skip
    return P


def cat(pts):
    return np.concatenate(pts) if pts else np.zeros(0, S3P_POINT_DTYPE)


def names(status):
    return [FUSE_STATUS_NAMES[int(s)] for s in np.asarray(status).ravel()]


def both(d):
    return {FUSE_KF: d, FUSE_SIM3: d}


# ---------------------------------------------------------------- sizes
def _n_jobs(n, n_cam=2):
    """n points, point i on its own feature i of camera 0, three bits off.  n_cam = 1: a search of exactly n JOBS (in
    LBA_FUSE_SIM3 its only camera is the last: every row NO_CAMERA).  n_cam = 2: the second camera is empty, so both
    modes have n LIVE jobs among the 2 n."""
    feats, pts = [], []
    for i in range(n):
        u, v = 20.0 + 9.0 * (i % 64), 30.0 + 40.0 * (i // 64)
        feats.append(feat(0, u + 0.5, v - 0.25, 2, near(D(i), 3, i)))
        pts.append(point(u, v, 2, D(i)))
    if n_cam == 1:
        return Case([target(1, feats)], cat(pts), [(0, 0, n)],
                    {FUSE_KF: dict(status=["OK"] * n, feat=list(range(n))),
                     FUSE_SIM3: dict(status=["NO_CAMERA"] * n, feat=[-1] * n)})
    return Case([target(2, feats)], cat(pts), [(0, 0, n)],
                {FUSE_KF: dict(status=["OK", "NO_CAND"] * n, feat=[v for i in range(n) for v in (i, -1)]),
                 FUSE_SIM3: dict(status=["OK", "NO_CAMERA"] * n, feat=[v for i in range(n) for v in (i, -1)])})


def _n_cam(n_cam):
    prob = make_fuse_problem(n_kf=2, n_cam=n_cam, n_feat=80, n_points=120, seed=10 + n_cam)
    ids = np.arange(prob.n_ids)
    exp = {FUSE_SIM3: dict(last_cam="NO_CAMERA")}
    return Case([prob.targets[1]], prob.points(ids), [(0, 0, len(ids))], exp)


def _straddle():
    """a wave's 64 jobs straddle two searches with different targets (1 and 2 cameras, 40 and 7 features): search 0 has
    40 jobs, search 1 starts at job 40 and runs into the second wave"""
    a = _n_jobs(40)
    t1 = target(1, [f for f in (feat(0, 20.0 + 9.0 * i + 0.5, 29.75, 2, near(D(i), 3, i)) for i in range(40))])
    fe = [feat(i % 2, 100.0 + 30.0 * i, 200.0, 2, near(D(100 + i), 4, i)) for i in range(7)]
    t2 = target(2, fe)
    pts = [a.points] + [point(100.0 + 30.0 * i, 200.0, 2, D(100 + i)) for i in range(7)] * 3
    return Case([t1, t2], cat(pts), [(0, 0, 40), (1, 40, 21)],
                {FUSE_KF: dict(n_ok=[40, 21])}, "KF: every point wins its feature in the camera that holds it")


# ---------------------------------------------------------------- windows
def _no_candidates():
    t = target(2, [feat(0, 500.0, 400.0, 2, D(1))])
    return Case([t], point(100.0, 100.0, 2, D(1)), [(0, 0, 1)],
                {FUSE_KF: dict(status=["NO_CAND", "NO_CAND"], n_cand=[0, 0]),
                 FUSE_SIM3: dict(status=["NO_CAND", "NO_CAMERA"], n_cand=[0, 0])})


def _span(n):
    """exactly n candidates in ONE span (one cell), the best the LAST of them: position n - 1"""
    d = D(7)
    feats = [feat(0, 320.0 + 0.01 * i, 240.5, 2, near(d, 3 if i == n - 1 else 10 + (i * 7) % 30, i)) for i in range(n)]
    return Case([target(2, feats)], point(320.0, 240.0, 2, d), [(0, 0, 1)],
                both(dict(feat=[n - 1, -1], best_dist=[3, 256], n_cand=[n, 0])))


def _clipped():
    """windows clipped at the left, right, top and bottom edge of the grid and at two corners, a feature inside each
    (AssignFeaturesToGrid rounds: a feature from x = 635 or y = 475 on is in no cell, so the right and bottom spots
    stay below)"""
    spots = [(1.0, 240.0), (632.0, 240.0), (320.0, 1.0), (320.0, 472.0), (1.0, 1.0), (632.0, 472.0)]
    feats = [feat(0, u + 0.5, v + 0.5, 2, near(D(i), 2, i)) for i, (u, v) in enumerate(spots)]
    pts = [point(u, v, 2, D(i)) for i, (u, v) in enumerate(spots)]
    return Case([target(2, feats)], cat(pts), [(0, 0, len(spots))],
                both(dict(feat=[v for i in range(len(spots)) for v in (i, -1)])))


def _outside_grid():
    """the grid starts at x = 200 (a caller's mvMinX there), the image at 0: a window at u = 50 lies wholly left of
    the grid and GetFeaturesInArea returns nothing"""
    t = target(2, [feat(0, 250.0, 100.0, 2, D(3))], gmin_x=200.0)
    return Case([t], point(50.0, 100.0, 2, D(3)), [(0, 0, 1)],
                {FUSE_KF: dict(status=["NO_CAND", "NO_CAND"]), FUSE_SIM3: dict(status=["NO_CAND", "NO_CAMERA"])})


# ---------------------------------------------------------------- ties
def _tie_one_stride():
    d = D(11)
    feats = [feat(0, 320.5, 240.5, 2, near(d, 9, 0)), feat(0, 320.6, 240.5, 2, near(d, 5, 1)),
             feat(0, 320.7, 240.5, 2, near(d, 5, 2)), feat(0, 320.8, 240.5, 2, near(d, 7, 3))]
    return Case([target(2, feats)], point(320.0, 240.0, 2, d), [(0, 0, 1)], both(dict(feat=[1, -1], best_dist=[5, 256])))


def _tie_two_strides():
    d = D(12)
    feats = [feat(0, 320.0 + 0.01 * i, 240.5, 2, near(d, 6 if i in (5, 64 + 2) else 20 + i % 9, i)) for i in range(80)]
    return Case([target(2, feats)], point(320.0, 240.0, 2, d), [(0, 0, 1)],
                both(dict(feat=[5, -1], best_dist=[6, 256], n_cand=[80, 0])))


def _tie_two_cells():
    """equal distances in three cells: the cell walked first (smaller ix, then smaller iy) wins although its feature
    index is larger.  Cells are 10 x 10 px: feature 0 is in (33, 24), feature 1 in (32, 24), feature 2 in (32, 25)."""
    d = D(13)
    feats = [feat(0, 325.2, 242.0, 3, near(d, 4, 0)), feat(0, 319.0, 242.0, 3, near(d, 4, 1)),
             feat(0, 322.0, 245.2, 3, near(d, 4, 2))]
    return Case([target(2, feats)], point(322.0, 242.0, 3, d), [(0, 0, 1)],
                both(dict(feat=[1, -1], best_dist=[4, 256], n_cand=[3, 0])))


# ---------------------------------------------------------------- distances and levels
def _complementary():
    d = D(14)
    t = target(2, [feat(0, 320.5, 240.5, 2, ~d)])
    return Case([t], point(320.0, 240.0, 2, d), [(0, 0, 1)],
                {FUSE_KF: dict(status=["TOO_FAR", "NO_CAND"], feat=[-1, -1], best_dist=[256, 256], n_cand=[1, 0]),
                 FUSE_SIM3: dict(status=["TOO_FAR", "NO_CAMERA"], feat=[0, -1], best_dist=[256, 256], n_cand=[1, 0])})


def _dist_50_51():
    d = D(15)
    t = target(2, [feat(0, 100.5, 100.5, 2, near(d, 50)), feat(0, 300.5, 100.5, 2, near(d, 51))])
    return Case([t], cat([point(100.0, 100.0, 2, d), point(300.0, 100.0, 2, d)]), [(0, 0, 2)],
                {FUSE_KF: dict(status=["OK", "NO_CAND", "TOO_FAR", "NO_CAND"], feat=[0, -1, 1, -1],
                               best_dist=[50, 256, 51, 256]),
                 FUSE_SIM3: dict(status=["OK", "NO_CAMERA", "TOO_FAR", "NO_CAMERA"], feat=[0, -1, 1, -1],
                                 best_dist=[50, 256, 51, 256])})


def _levels(level):
    """features at level - 2 .. level + 1, the out-of-gate ones the closest in Hamming distance"""
    d = D(16 + level)
    octs = [o for o in range(level - 2, level + 2) if o >= 0]
    bits = {level - 2: 1, level - 1: 9, level: 8, level + 1: 2}
    feats = [feat(0, 320.2 + 0.1 * i, 240.2, o, near(d, bits[o], i)) for i, o in enumerate(octs)]
    win = octs.index(level)
    n = 2 if level > 0 else 1
    return Case([target(2, feats)], point(320.0, 240.0, level, d), [(0, 0, 1)],
                {FUSE_KF: dict(feat=[win, -1], best_dist=[8, 256], level=[level, level], n_cand=[n, 0]),
                 FUSE_SIM3: dict(feat=[win, -1], best_dist=[8, 256], level=[level, -1], n_cand=[n, 0])})


# ---------------------------------------------------------------- stereo
def _edge(limit, centre, e0):
    """adjacent floats x below `centre` with e = centre - x (exact) and (double)(float(e * e) * 1.0f) <= limit for the
    first, > limit for the second: (inside, outside)"""
    c = F(centre)
    e2 = lambda x: np.float64((c - x) * (c - x))
    x = F(centre - e0)
    while e2(x) > limit:
        x = np.nextafter(x, c)
    while not e2(np.nextafter(x, F(-1e9))) > limit:
        x = np.nextafter(x, F(-1e9))
    return float(x), float(np.nextafter(x, F(-1e9)))


def _stereo_sign():
    """u_right negative, zero and positive in the LAST camera (1) and in another (0).  The points' ur is u - bf / z =
    u - 10.  Zero counts as stereo in the last camera only (quirk (c)): er = 190 there and the feature is dropped; the
    positive one (290.5 against ur 290) passes with the three-term e2."""
    d = D(20)
    feats = []
    for cam in (0, 1):
        for i, ur in enumerate((-1.0, 0.0, 290.5)):
            feats.append(feat(cam, 100.0 + 100.0 * i + 0.5, 100.0, 0, near(d, 3 + i, cam), ur))
    pts = [point(100.0 + 100.0 * i, 100.0, 0, d, z=4.0) for i in range(3)]
    return Case([target(2, feats)], cat(pts), [(0, 0, 3)],
                {FUSE_KF: dict(status=["OK", "OK", "OK", "NO_CAND", "OK", "OK"], feat=[0, 3, 1, -1, 2, 5]),
                 FUSE_SIM3: dict(status=["OK", "NO_CAMERA"] * 3, feat=[0, -1, 1, -1, 2, -1])})


def _chi2_edges():
    """e2 * invSigma2 just either side of 5.99 (camera 0, mono: ex = 320 - kpx) and of 7.8 (the last camera, stereo,
    ex = ey = 0, er = 90 - u_right), at level 0 where invSigma2 is 1: adjacent floats of kpx and of u_right"""
    d = D(21)
    m_in, m_out = _edge(5.99, 320.0, np.sqrt(5.99))
    s_in, s_out = _edge(7.8, 90.0, np.sqrt(7.8))
    feats = [feat(0, m_in, 100.0, 0, near(d, 2, 0)), feat(0, m_out, 300.0, 0, near(d, 2, 1)),
             feat(1, 100.0, 100.0, 0, near(d, 2, 2), s_in), feat(1, 100.0, 300.0, 0, near(d, 2, 3), s_out)]
    pts = [point(320.0, 100.0, 0, d), point(320.0, 300.0, 0, d), point(100.0, 100.0, 0, d), point(100.0, 300.0, 0, d)]
    return Case([target(2, feats)], cat(pts), [(0, 0, 4)],
                {FUSE_KF: dict(status=["OK", "NO_CAND", "NO_CAND", "NO_CAND", "NO_CAND", "OK", "NO_CAND", "NO_CAND"]),
                 FUSE_SIM3: dict(status=["OK", "NO_CAMERA", "OK", "NO_CAMERA", "NO_CAND", "NO_CAMERA", "NO_CAND",
                                         "NO_CAMERA"])})


# ---------------------------------------------------------------- geometric gates
def _gates():
    d = D(22)
    t = target(2, [feat(0, 320.5, 240.5, 2, near(d, 3))])
    behind = point(320.0, 240.0, 2, d)
    behind["pos"][0, 2] = -4.0
    z0 = point(320.0, 240.0, 2, d)
    z0["pos"][0] = (1.0, 0.0, 0.0)
    at_max = point(640.0, 240.0, 2, d)                     # u == max_x exactly
    below_max = point(640.0 - 1.0 / 64, 240.0, 2, d)
    base = point(320.0, 240.0, 2, d)                       # dist 4 exactly
    dmin, dmax = base.copy(), base.copy()
    dmin["min_dist"], dmax["max_dist"] = 4.0, 4.0
    dmin_out, dmax_out = base.copy(), base.copy()
    dmin_out["min_dist"], dmax_out["max_dist"] = np.nextafter(F(4.0), F(5)), np.nextafter(F(4.0), F(0))
    ang_eq = point(320.0, 240.0, 2, d, normal=(0.5, 0.0, 0.5))      # dot = 2 = 0.5 * 4
    ang_out = point(320.0, 240.0, 2, d, normal=(0.5, 0.0, np.nextafter(F(0.5), F(0))))
    skipped = point(320.0, 240.0, 2, d, skip=1)
    pts = [behind, z0, at_max, below_max, dmin, dmax, dmin_out, dmax_out, ang_eq, ang_out, skipped]
    cam0 = ["BEHIND", "OUT_OF_IMAGE", "OUT_OF_IMAGE", "NO_CAND", "OK", "OK", "DIST", "DIST", "OK", "ANGLE", "SKIPPED"]
    cam1 = ["BEHIND", "OUT_OF_IMAGE", "OUT_OF_IMAGE", "NO_CAND", "NO_CAND", "NO_CAND", "DIST", "DIST", "NO_CAND",
            "ANGLE", "SKIPPED"]
    return Case([t], cat(pts), [(0, 0, len(pts))],
                {FUSE_KF: dict(status=[s for pair in zip(cam0, cam1) for s in pair]),
                 FUSE_SIM3: dict(status=[s for a in cam0 for s in (a, "NO_CAMERA")])})


# ---------------------------------------------------------------- targets
def _empty_target():
    t = target(3, [])
    pts = [point(100.0 + i, 100.0, 2, D(i)) for i in range(5)]
    return Case([t], cat(pts), [(0, 0, 5)],
                {FUSE_KF: dict(status=["NO_CAND"] * 15), FUSE_SIM3: dict(status=["NO_CAND", "NO_CAND", "NO_CAMERA"] * 5)})


def _mixed_targets():
    """targets of 0, 3 and 200 features and of 1, 2 and 4 cameras in one call, searches that share a point range and
    one without points"""
    prob = make_fuse_problem(n_kf=2, n_cam=4, n_feat=50, n_points=90, seed=31)
    small = _tie_one_stride()
    ids = np.arange(prob.n_ids)
    pts = cat([prob.points(ids), small.points])
    n = len(ids)
    return Case([prob.targets[0], target(1, []), small.targets[0], prob.targets[1]], pts,
                [(0, 0, n), (1, 0, 17), (2, n, 1), (3, 0, n), (0, 5, 0), (3, 10, 60)], {})


_BUILD = dict(
    ncam_1=lambda: _n_cam(1), ncam_2=lambda: _n_cam(2), ncam_4=lambda: _n_cam(4),
    jobs_0=lambda: _n_jobs(0, 1), jobs_1=lambda: _n_jobs(1, 1), jobs_63=lambda: _n_jobs(63, 1),
    jobs_64=lambda: _n_jobs(64, 1), jobs_65=lambda: _n_jobs(65, 1), live_1=lambda: _n_jobs(1), live_63=lambda: _n_jobs(63),
    live_64=lambda: _n_jobs(64), live_65=lambda: _n_jobs(65), straddle=_straddle,
    no_candidates=_no_candidates, span_64=lambda: _span(64), span_65=lambda: _span(65), clipped=_clipped,
    outside_grid=_outside_grid,
    tie_one_stride=_tie_one_stride, tie_two_strides=_tie_two_strides, tie_two_cells=_tie_two_cells,
    complementary=_complementary, dist_50_51=_dist_50_51, levels_bottom=lambda: _levels(0),
    levels_top=lambda: _levels(N_LEVELS - 1),
    stereo_sign=_stereo_sign, chi2_edges=_chi2_edges, gates=_gates,
    empty_target=_empty_target, mixed_targets=_mixed_targets,
)
NAMES = list(_BUILD)


def case(name):
    if name not in _cache:
        _cache[name] = _BUILD[name]()
    return _cache[name]


def gpu_problem(seed):
    """a generated scene for the GPU tests: 21 searches as SearchInNeighbors has them"""
    key = ("gpu", seed)
    if key not in _cache:
        _cache[key] = make_fuse_problem(n_kf=21, n_cam=4, n_feat=120, n_points=260, seed=seed)
    return _cache[key]


def level_settled(quot):
    q = np.asarray(quot)[np.isfinite(quot)]
    return bool((np.abs(q - np.round(q)) > M_LEVEL).all())
