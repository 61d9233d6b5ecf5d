"""Named cases of the Sim3 SearchByProjection (lba_match_sim3_project): the smallest shapes at which each stage can go
wrong.  `case(name)` returns (Keyframe, [Hypothesis], expectations dict); every case is run at each of PARAMS.

The hand-made cases use an identity chain (Sbw, both poses and Tbc the identity, velocities 0), for which Tcw is exactly
the identity in any arithmetic, so a point's pixel, distance and viewing angle are exact float32 numbers and can sit ON a
gate.  The generated cases (amc_lba.sim3_project.make_s3p_problem) have a general pose chain, asynchronous cameras and
points that compete for features.

Settledness (tests/test_s3p_cases.py checks it on every case and seed below; nothing is ever dropped from a comparison):
a pose entry is settled if its fp64 value is further than M_POSE from the nearest midpoint between adjacent floats,
relative to the entry's scale (1 for a rotation entry, max(1, |t|_inf) for a translation entry: the scale of the fp64
chain's rounding error), a job if PredictScale's quotient is further than M_LEVEL from an integer (a quotient that is not
finite is settled by quirk (h)'s definition; an entry that is exactly 0 or +-1 is exact, see s3p_oracle.pose_margin).
The margins are max(1e-12, 64 x the largest difference measured between the host build of csrc/lba_s3p_math.hpp and
tests/s3p_oracle.py) over all cases, the 33-batch and make_s3p_problem's seeds 0 .. 39 (scripts/s3p_margins.py writes
profiles/sim3_project_margins.log): both measured differences are a few 1e-15, so M_POSE = M_LEVEL = 1e-12.
Seed search, recorded: at M_POSE = 1e-12 an entry is unsettled with probability of the order 1e-5, a search about one
time in a thousand.  For each generated shape the seeds 0, 1, 2, ... were tried in order and the first settled ones
taken: seed 0 for every named case, seeds 0, 1, 2 for GPU_SEEDS; of the 40 seeds measured, 32 and 33 are unsettled.  batch_33
generates 40 hypotheses on one keyframe (seed 3) and takes the first 33 settled ones: the rule is applied by `batch_33`
itself and the CPU test checks the outcome (hypotheses 3, 15, 31 and 34 of the 40 are unsettled and left out).
"""
import numpy as np

from amc_lba.abi import MATCH_FEAT_DTYPE
from amc_lba.match import build_grid, match_cams, scale_factors
from amc_lba.sim3_project import (CALL_SITES, S3P_CAM_DTYPE, S3P_KF_DTYPE, S3P_POINT_DTYPE, Hypothesis, Keyframe,
                                  make_s3p_problem, s3p_params)

F = np.float32
M_POSE = 1e-12
M_LEVEL = 1e-12
FX, CX, CY, W, H = 256.0, 320.0, 240.0, 640.0, 480.0
N_LEVELS, SCALE = 8, 1.2
LOG_SF = F(np.log(SCALE))
# (th, ratio) of the three call sites in both projection forms
PARAMS = [(th, ratio, form) for th, ratio in CALL_SITES for form in (0, 1)]
PARAM_IDS = ["th%d_r%.1f_form%d" % p for p in PARAMS]
GPU_SEEDS = (0, 1, 2)                       # make_s3p_problem(n_cam=4, n_feat=300, n_hyp=3, n_points=400): all settled
BATCH_SEED = 3                              # the 33-hypothesis batch


def params(p):
    return s3p_params(th=p[0], ratio_hamming=p[1], proj_form=p[2])


def desc_bits(*bits):
    d = np.zeros(8, np.uint32)
    for b in bits:
        d[b >> 5] |= np.uint32(1) << np.uint32(b & 31)
    return d


def identity_kf(n_cam=1, has_prev=1, feats=(), ow=None, stamps=None):
    """an identity chain; feats: (cam, x, y, octave, desc)"""
    kf = np.zeros(1, S3P_KF_DTYPE)
    kf["stamp"], kf["stamp_prev"] = 2.0, 1.0
    kf["q"], kf["q_prev"] = (0, 0, 0, 1), (0, 0, 0, 1)
    kf["log_scale_factor"], kf["has_prev"], kf["n_levels"], kf["n_cam"] = LOG_SF, has_prev, N_LEVELS, n_cam
    kc = np.zeros(n_cam, S3P_CAM_DTYPE)
    kc["stamp"] = 2.0 if stamps is None else stamps
    kc["q_bc"] = (0, 0, 0, 1)
    kc["fx"], kc["fy"], kc["cx"], kc["cy"] = FX, FX, CX, CY
    kc["max_x"], kc["max_y"] = W, H
    if ow is not None:
        kc["ow"] = ow
    gc = match_cams(n_cam, 0.0, 0.0, W, H)
    ft = np.zeros(len(feats), MATCH_FEAT_DTYPE)
    for i, (c, x, y, o, d) in enumerate(feats):
        ft[i]["cam"], ft[i]["x"], ft[i]["y"], ft[i]["octave"], ft[i]["desc"] = c, x, y, o, d
    ft["u_right"] = -1.0
    cs, cf = build_grid(ft, gc)
    return Keyframe(kf, kc, gc, scale_factors(N_LEVELS, SCALE), cs, cf, ft)


def point(pos, normal=(0, 0, 1), level=0.5, desc=None, skip=0, min_dist=None, max_dist=None, ow=(0, 0, 0)):
    """mfMaxDistance puts PredictScale's quotient at `level` (a half: ceil gives level + 0.5)"""
    p = np.zeros(1, S3P_POINT_DTYPE)
    dist = float(np.linalg.norm(np.asarray(pos, float) - np.asarray(ow, float)))
    p["pos"], p["normal"] = pos, normal
    p["max_distance"] = dist * SCALE ** level
    p["min_dist"] = 0.01 if min_dist is None else min_dist
    p["max_dist"] = 1e4 if max_dist is None else max_dist
    p["desc"] = desc_bits() if desc is None else desc
    p["skip"] = skip
    return p


def at_pixel(u, v, z=2.0):
    """the point that projects to (u, v) exactly under the identity pose (fx = 256: integer u, v and z = 2 give exact
    float32 coordinates and an exact projection in either form)"""
    return ((u - CX) * z / FX, (v - CY) * z / FX, z)


def identity_hyp(points, taken=None):
    pts = np.concatenate(points) if len(points) else np.zeros(0, S3P_POINT_DTYPE)
    return Hypothesis((0, 0, 0, 1), (0, 0, 0), 1.0, pts, taken)


def _row_of_points(n, with_feats=True, n_cam=1):
    """n points on a lattice 16 px apart, each with its own feature (its descriptor) in every camera"""
    feats, pts = [], []
    for i in range(n):
        u, v = 16.0 + 16.0 * (i % 38), 16.0 + 16.0 * (i // 38)
        d = desc_bits(*[(7 * i + k) % 256 for k in range(1 + i % 5)])
        if with_feats:
            feats += [(c, u, v, 1, d) for c in range(n_cam)]
        pts.append(point(at_pixel(u, v), level=0.5, desc=d))
    return feats, pts


def _chain(n):
    """n jobs that each want the feature the job before takes: job 0 sees f_1 only; job k sees f_k and f_k+1 and prefers
    f_k.  Features alternate between descriptors A (no bit) and B (bits 0 .. 14)."""
    B = list(range(15))
    feats = [(0, 40.0 + 4.0 * k, 100.0, 0, desc_bits(*B) if k & 1 else desc_bits()) for k in range(n + 1)]
    pts = [point(at_pixel(44.0, 100.0), level=-0.5, desc=desc_bits(*B))]
    for k in range(1, n):
        d = desc_bits(*B[5:]) if k & 1 else desc_bits(*B[:5])      # 5 from f_k, 10 from f_k+1
        pts.append(point(at_pixel(42.0 + 4.0 * k, 100.0), level=-0.5, desc=d))
    return feats, pts


NAMES = []
_BUILDERS = {}


def _case(fn):
    NAMES.append(fn.__name__)
    _BUILDERS[fn.__name__] = fn
    return fn


@_case
def live_0():
    return identity_kf(feats=[(0, 100.0, 100.0, 1, desc_bits())]), [identity_hyp([point((0, 0, -2.0))])], dict(live=[0])


def _live(n):
    def build():
        feats, pts = _row_of_points(n)
        return identity_kf(feats=feats), [identity_hyp(pts)], dict(live=[n], rounds=[1 if n else 0], n_matches=n)
    build.__name__ = "live_%d" % n
    return _case(build)


for _n in (1, 63, 64, 65, 255, 256, 257):
    _live(_n)


@_case
def four_cameras_identity():
    feats, pts = _row_of_points(70, n_cam=4)
    return identity_kf(n_cam=4, feats=feats), [identity_hyp(pts)], dict(live=[70] * 4, n_matches=280)


@_case
def camera_without_live_job():
    """camera 1 looks backwards (Tbc a half turn about y): every point is behind it"""
    feats, pts = _row_of_points(20, n_cam=2)
    k = identity_kf(n_cam=2, feats=feats)
    k.kcams[1]["q_bc"] = (0, 1, 0, 0)
    return k, [identity_hyp(pts)], dict(live=[20, 0], rounds=[1, 0])


@_case
def no_prev():
    feats, pts = _row_of_points(5)
    return identity_kf(has_prev=0, feats=feats), [identity_hyp(pts)], dict(all_status="NO_PREV", n_matches=0)


@_case
def all_skipped():
    feats, pts = _row_of_points(5)
    for p in pts:
        p["skip"] = 1
    return identity_kf(feats=feats), [identity_hyp(pts)], dict(all_status="SKIPPED", n_matches=0)


@_case
def z_zero_and_behind():
    """(d): z == 0 with X != 0 passes `z < 0` and ends OUT_OF_IMAGE at +-inf; the next float below zero is BEHIND"""
    pts = [point((1.0, 0.5, 0.0), ow=(9, 9, 9)), point((-1.0, 0.5, 0.0), ow=(9, 9, 9)),
           point((1.0, 0.5, -1e-30), ow=(9, 9, 9))]
    return identity_kf(), [identity_hyp(pts)], dict(status=["OUT_OF_IMAGE", "OUT_OF_IMAGE", "BEHIND"])


@_case
def image_bounds():
    """>= min and < max: ON each bound, and a hair (2^-18 relative) to its other side"""
    x0, y0 = at_pixel(0.0, 0.0)[:2]
    x1, y1 = at_pixel(W, H)[:2]
    xm, ym = at_pixel(100.0, 100.0)[:2]
    out, inn = 1.0 + 2.0 ** -18, 1.0 - 2.0 ** -18
    pts = [point((x0, ym, 2.0)), point((x0 * out, ym, 2.0)), point((x1, ym, 2.0)), point((x1 * inn, ym, 2.0)),
           point((xm, y0, 2.0)), point((xm, y0 * out, 2.0)), point((xm, y1, 2.0)), point((xm, y1 * inn, 2.0))]
    st = ["NO_CAND", "OUT_OF_IMAGE", "OUT_OF_IMAGE", "NO_CAND", "NO_CAND", "OUT_OF_IMAGE", "OUT_OF_IMAGE", "NO_CAND"]
    return identity_kf(), [identity_hyp(pts)], dict(status=st)


@_case
def distance_bounds():
    up = float(np.nextafter(F(2.0), F(np.inf)))
    dn = float(np.nextafter(F(2.0), F(0)))
    pts = [point((0, 0, 2.0), min_dist=2.0), point((0, 0, 2.0), min_dist=up),
           point((0, 0, 2.0), max_dist=2.0), point((0, 0, 2.0), max_dist=dn)]
    return identity_kf(), [identity_hyp(pts)], dict(status=["NO_CAND", "DIST", "NO_CAND", "DIST"])


@_case
def angle_60():
    """PO = (0, 0, 2), dist 2: PO . n = 1 = 0.5 * dist passes (`<`), the next float below fails"""
    dn = float(np.nextafter(F(0.5), F(0)))
    pts = [point((0, 0, 2.0), normal=(0.8, 0.3, 0.5)), point((0, 0, 2.0), normal=(0.8, 0.3, dn))]
    return identity_kf(), [identity_hyp(pts)], dict(status=["NO_CAND", "ANGLE"])


@_case
def levels():
    """the quotient at -3.5 (clamped to 0), -0.5 (0), 0.5 (1), 6.5 (7, the top), 9.5 (clamped to 7)"""
    pts = [point((0, 0, 2.0), level=q) for q in (-3.5, -0.5, 0.5, 6.5, 9.5)]
    return identity_kf(), [identity_hyp(pts)], dict(level=[0, 0, 1, 7, 7])


@_case
def keypoint_levels():
    """predicted level 3; keypoints at levels 1, 2, 3, 4 on the pixel: 1 and 4 (distance 0) are not candidates, 2 wins"""
    d = desc_bits(*range(40))
    feats = [(0, 100.0, 100.0, 1, d), (0, 100.0, 100.0, 2, desc_bits(*range(30))), (0, 100.0, 100.0, 3, desc_bits(*range(20))),
             (0, 100.0, 100.0, 4, d)]
    return identity_kf(feats=feats), [identity_hyp([point(at_pixel(100.0, 100.0), level=2.5, desc=d)])], \
        dict(status=["OK"], feat=[1], best_dist=[10], level=[3])


@_case
def camera_centre_quirk():
    """(a): the map's centre is 50 away from the corrected one (the origin): with it the first point is out of its
    distance range and the second one in; with the corrected centre it would be the other way round"""
    ow = (0.0, 0.0, -50.0)
    p0 = point((0, 0, 2.0), min_dist=1.0, max_dist=3.0, ow=ow)
    p1 = point((0, 0, 2.0), min_dist=40.0, max_dist=60.0, ow=ow)
    return identity_kf(ow=ow), [identity_hyp([p0, p1])], dict(status=["DIST", "NO_CAND"])


@_case
def two_cameras_match():
    """(b): the point matches in camera 0 and again in camera 1"""
    d = desc_bits(1, 2, 3)
    feats = [(0, 100.0, 100.0, 1, d), (1, 100.0, 100.0, 1, d)]
    return identity_kf(n_cam=2, feats=feats), [identity_hyp([point(at_pixel(100.0, 100.0), desc=d)])], \
        dict(status=["OK", "OK"], n_matches=2)


@_case
def taken_on_entry():
    d = desc_bits(1, 2, 3)
    feats = [(0, 100.0, 100.0, 1, d), (0, 101.0, 100.0, 1, desc_bits(1, 2))]
    return identity_kf(feats=feats), [identity_hyp([point(at_pixel(100.0, 100.0), desc=d)], taken=[1, 0])], \
        dict(status=["OK"], feat=[1], best_dist=[1])


@_case
def chain_64():
    feats, pts = _chain(64)
    return identity_kf(feats=feats), [identity_hyp(pts)], dict(rounds=[64], n_matches=64, only_th=3)


@_case
def disjoint_64():
    feats, pts = _row_of_points(64)
    return identity_kf(feats=feats), [identity_hyp(pts)], dict(rounds=[1], n_matches=64)


@_case
def tie_first():
    """two keypoints at the same distance: the first in (ix, iy, position in cell) order wins"""
    d = desc_bits(1, 2, 3)
    feats = [(0, 106.0, 100.0, 1, desc_bits(1, 2, 3, 4)), (0, 104.0, 100.0, 1, desc_bits(1, 2, 3, 5))]   # cells 11, 10
    return identity_kf(feats=feats), [identity_hyp([point(at_pixel(105.0, 100.0), desc=d)])], \
        dict(status=["OK"], best_dist=[1], feat=[1])


@_case
def dist_256():
    d = desc_bits(*range(256))
    return identity_kf(feats=[(0, 100.0, 100.0, 1, desc_bits())]), \
        [identity_hyp([point(at_pixel(100.0, 100.0), desc=d)])], dict(status=["TOO_FAR"], best_dist=[256], feat=[-1])


@_case
def quirk_h():
    """(h): dist == 0 (the point ON the map's camera centre): ratio +inf -> the top level; with mfMaxDistance 0 as well
    the ratio is NaN -> level 0"""
    ow = (0.0, 0.0, 2.0)
    p0 = point((0, 0, 2.0), ow=(0, 0, 0), min_dist=0.0)
    p1 = point((0, 0, 2.0), ow=(0, 0, 0), min_dist=0.0)
    p1["max_distance"] = 0.0
    return identity_kf(ow=ow), [identity_hyp([p0, p1])], dict(level=[N_LEVELS - 1, 0], unsettled_level_ok=True)


@_case
def generated_1cam():
    k, h = make_s3p_problem(n_cam=1, n_feat=200, n_hyp=2, n_points=150, seed=0)
    return k, h, dict()


@_case
def generated_4cam():
    k, h = make_s3p_problem(n_cam=4, n_feat=150, n_hyp=2, n_points=200, seed=0)
    return k, h, dict()


@_case
def shared_and_end_stamps():
    """cameras 0 and 1 share a stamp inside the interval; camera 3 is at the keyframe's own stamp (QueryPose's end point)"""
    k, h = make_s3p_problem(n_cam=4, n_feat=100, n_hyp=1, n_points=120, seed=0)
    k.kcams[1]["stamp"] = k.kcams[0]["stamp"]
    assert k.kcams[3]["stamp"] == k.kf[0]["stamp"]
    return k, h, dict()


@_case
def lds_limit():
    """exactly 8192 features in one camera"""
    k, h = make_s3p_problem(n_cam=1, n_feat=8192, n_hyp=1, n_points=200, seed=0)
    return k, h, dict(n_feat_cam=8192)


def gpu_problem(seed):
    return make_s3p_problem(n_cam=4, n_feat=300, n_hyp=3, n_points=400, seed=seed)


def pose_settled(kfm, hyp):
    import s3p_oracle as so
    return bool(so.pose_margin(so.pose_f64(kfm, hyp)).min() > M_POSE)


def level_settled(quot):
    q = np.asarray(quot, np.float64)
    q = q[np.isfinite(q)]
    return bool((np.abs(q - np.round(q)) > M_LEVEL).all())


def batch_33():
    """one keyframe, 33 hypotheses of 150 points: the first 33 pose-settled ones of 40 generated"""
    if "batch_33" not in _cache:
        k, hyps = make_s3p_problem(n_cam=4, n_feat=300, n_hyp=40, n_points=150, seed=BATCH_SEED)
        _cache["batch_33"] = (k, [h for h in hyps if pose_settled(k, h)][:33])
    return _cache["batch_33"]


_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    k, h, e = _cache[name]
    return k, h, e
