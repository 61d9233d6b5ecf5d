"""The named cases of lba_triangulate (tests/test_tri_cases.py on the CPU, tests/test_gpu_triangulate.py on the GPU).

A case is small (at most 3 pairs, at most 257 rows per pair) and has a property its builder asserts on the fp64
restatement (tests/tri_oracle.py).  `case(name)` returns (Case, fp64 result, float32-faithful result), computed once.
Exact-boundary inputs use values exactly representable in float, so both precisions decide alike.
"""
import functools

import numpy as np

import tri_oracle as to
from amc_lba.abi import TRI_PAIR_DTYPE, TRI_ROW_DTYPE
from amc_lba.triangulate import (LbaTriParams, make_tri_pairs, ratio_factor, scale_pyramid, tri_keyframes, tri_project)

U = 2.0 ** -53
SF, SIG2 = scale_pyramid(8)
# M_F32: 4 x the largest relative difference of a gate quantity between the float32 and the fp64 restatement, measured
# over the cases and six further seeds by scripts/triangulate_margins.py (profiles/triangulate_margins.log).  Over all
# gates that figure is 9.41e-4, set by the depth z of an ill-conditioned gross outlier; as ONE margin, 4 x 9.41e-4 on a
# cosine is 5 degrees of parallax around the 0.9998 gate and would put three quarters of all rows "near a gate".  So
# each gate quantity gets 4 x ITS OWN measured difference; every one of them is at most the single figure, so the rows
# held to equal status are a superset of those a single margin would hold.
M_F32_MEASURED = {"cos": 2.73e-7, "z": 9.41e-4, "reproj": 1.86e-4, "dist": 2.87e-5, "ratio": 4.11e-6}
M_F32 = {k: 4 * v for k, v in M_F32_MEASURED.items()}


class Case:
    def __init__(self, pairs, rows, kfs, cams, n_cam, ratio=None, far_points=0, th_far=0.0, check=None, note=""):
        self.pairs, self.rows, self.kfs, self.cams, self.n_cam = pairs, rows, kfs, cams, n_cam
        self.ratio = ratio_factor(1.2) if ratio is None else ratio
        self.far_points, self.th_far = far_points, th_far
        self.check, self.note = check, note
        self.reported = False    # a case whose results hinge on rounding noise: printed, not compared
        self.exact = False       # a case whose arithmetic is exact in binary: compared although it sits ON a gate

    def params(self):
        return LbaTriParams(self.ratio, self.th_far, self.far_points, 0)

    def in_pairs(self):
        """mask of the rows some pair covers"""
        m = np.zeros(len(self.rows), bool)
        for P in self.pairs:
            m[P["row0"]:P["row0"] + P["n_rows"]] = True
        return m


def _gen(**kw):
    pairs, rows, kfs, cams, truth = make_tri_pairs(**kw)
    return Case(pairs, rows, kfs, cams, kw.get("n_cam", 4)), truth


def _has(*statuses, stereo=None):
    def check(c, r):
        for s in statuses:
            assert (r.status[c.in_pairs()] == s).any(), (s, np.bincount(r.status[c.in_pairs()], minlength=11))
        if stereo is not None:
            assert ((r.status == to.OK) & (r.stereo == stereo))[c.in_pairs()].any()
    return check


def _sized(sizes, seed):
    """pairs of the given row counts, packed one behind the other"""
    def build():
        c, _ = _gen(n_pairs=len(sizes), n_rows=max(max(sizes), 1), seed=seed)
        rows, row0 = [], 0
        for p, n in enumerate(sizes):
            rows.append(c.rows[c.pairs[p]["row0"]:c.pairs[p]["row0"] + n])
            c.pairs[p]["row0"], c.pairs[p]["n_rows"] = row0, n
            row0 += n
        c.rows = np.concatenate(rows) if row0 else np.zeros(0, TRI_ROW_DTYPE)

        def check(c, r):
            assert [int(n) for n in c.pairs["n_rows"]] == list(sizes)
            if sum(sizes) >= 63:
                assert (r.status == to.OK).any() and (r.status != to.OK).any()
        c.check = check
        return c
    return build


# ---- hand-made geometry: two keyframes of the rig, the second `move` (body frame: x right, y down, z ahead) away
def _two(move, n_cam=4):
    return tri_keyframes([(np.eye(3), np.zeros(3)), (np.eye(3), np.asarray(move, float))], n_cam)


def _row(kfs, cams, n_cam, X, cam1, cam2, o1=0, o2=0, stereo1=False, stereo2=False, dz1=(0, 0), dz2=(0, 0)):
    """the match of world point X in camera cam1 of keyframe 0 and cam2 of keyframe 1: exact projections (rounded to
    float) plus the pixel offsets dz; a stereo side gets ur = u - bf / z and the depth of that disparity"""
    r = np.zeros(1, TRI_ROW_DTYPE)[0]
    for side, (k, c, o, st, dz) in enumerate(((0, cam1, o1, stereo1, dz1), (1, cam2, o2, stereo2, dz2)), start=1):
        u, v, z = tri_project(cams[k * n_cam + c], X)
        uv = np.float32([u + dz[0], v + dz[1]])
        r[f"cam{side}"], r[f"z{side}"], r[f"k{side}"] = c, uv, uv
        r[f"sigma2_{side}"], r[f"scale{side}"] = SIG2[o], SF[o]
        r[f"ur{side}"], r[f"depth{side}"] = -1.0, 0.0
        if st:
            ur = np.float32(u - kfs[k]["bf"] / z)
            r[f"ur{side}"], r[f"depth{side}"] = ur, np.float32(kfs[k]["bf"]) / (uv[0] - ur)
    return r


def _one_pair(rows, kfs, cams, n_cam=4, **kw):
    pairs = np.zeros(1, TRI_PAIR_DTYPE)
    pairs[0]["kf1"], pairs[0]["kf2"], pairs[0]["n_rows"] = 0, 1, len(rows)
    return Case(pairs, np.array(rows, TRI_ROW_DTYPE), kfs, cams, n_cam, **kw)


LAST = 3
FAR_X = (0.5, -0.3, 12.0)     # a point 12 m ahead of the last camera


def _expect(*want):
    """the statuses (and, where given as (status, stereo_point), the flag) of the case's rows, in order"""
    def check(c, r):
        got = [(int(s), int(p)) for s, p in zip(r.status, r.stereo)]
        for g, w in zip(got, want):
            assert (g == w) if isinstance(w, tuple) else (g[0] == w), (got, want)
        assert len(got) == len(want)
    return check


def _parallax():
    kfs, cams = _two((0.02, 0.0, 0.0))   # a 2 cm baseline: cosRays above 0.9998, no stereo
    rows = [_row(kfs, cams, 4, FAR_X, LAST, LAST), _row(kfs, cams, 4, (3.0, 1.0, 20.0), LAST, LAST)]
    return _one_pair(rows, kfs, cams, check=_expect(to.PARALLAX, to.PARALLAX))


def _no_depth():
    kfs, cams = _two((0.02, 0.0, 0.0))
    a = _row(kfs, cams, 4, FAR_X, LAST, LAST, stereo1=True)
    a["depth1"] = 0.0                       # depth == 0 exactly: cosStereo1 = cos(pi) = -1, the stereo branch, z <= 0
    b = _row(kfs, cams, 4, FAR_X, LAST, LAST, stereo2=True)
    b["depth2"] = -1.0
    return _one_pair([a, b], kfs, cams, check=_expect((to.NO_DEPTH, 1), (to.NO_DEPTH, 1)))


def _behind():
    # BEHIND1: rays that diverge (the keypoints swapped sideways) meet behind both cameras
    kfs, cams = _two((1.0, 0.0, 0.0))
    a = _row(kfs, cams, 4, FAR_X, LAST, LAST, dz1=(-60, 0), dz2=(60, 0))
    # BEHIND2: a stereo point 5 m ahead of KF1 back-projected (parallel rays), KF2 10 m further on
    kfs2, cams2 = _two((0.0, 0.0, 10.0))
    b = _row(kfs2, cams2, 4, (0.2, 0.1, 5.0), LAST, LAST, stereo1=True)
    b["z2"] = b["k2"] = b["z1"]
    pairs = np.zeros(2, TRI_PAIR_DTYPE)
    pairs["kf1"], pairs["kf2"], pairs["row0"], pairs["n_rows"] = (0, 2), (1, 3), (0, 1), (1, 1)
    kfs2 = kfs2.copy()
    kfs2["cam0"] += 8
    return Case(pairs, np.array([a, b], TRI_ROW_DTYPE), np.concatenate([kfs, kfs2]), np.concatenate([cams, cams2]), 4,
                check=_expect(to.BEHIND1, (to.BEHIND2, 1)))


def _reproj():
    kfs, cams = _two((1.0, 0.0, 0.3))
    good = _row(kfs, cams, 4, FAR_X, LAST, LAST)
    # an offset ACROSS the epipolar line cannot be triangulated away: it splits between the two views
    bad = _row(kfs, cams, 4, FAR_X, LAST, LAST, dz2=(0, 12))
    # a stereo side 1 holds the point to its own depth through u_r, so the whole offset lands in view 2
    bad2 = _row(kfs, cams, 4, FAR_X, LAST, LAST, o1=3, stereo1=True, dz1=(0, 3), dz2=(0, -3))
    s1 = _row(kfs, cams, 4, FAR_X, LAST, LAST, stereo1=True)
    s1["ur1"] = s1["ur1"] + np.float32(8.0)   # a wrong right coordinate: the 7.8 gate of KF1
    s2 = _row(kfs, cams, 4, FAR_X, LAST, LAST, stereo2=True)
    s2["ur2"] = s2["ur2"] + np.float32(8.0)

    def check(c, r):
        assert r.status[0] == to.OK and r.status[1] in (to.REPROJ1, to.REPROJ2)
        assert r.status[3] == to.REPROJ1 and r.status[4] == to.REPROJ2
        assert (r.status == to.REPROJ1).any() and (r.status == to.REPROJ2).any(), r.status
    return _one_pair([good, bad, bad2, s1, s2], kfs, cams, check=check)


def _dist_zero():
    """a deliberately inconsistent Ow: the centre of KF2's camera is put exactly ON a stereo back-projection whose
    arithmetic is exact in both precisions (focal length 512, small binary fractions)"""
    kfs, cams = tri_keyframes([(np.eye(3), np.zeros(3)), (np.eye(3), np.array([0.0, 0.0, -2.0]))], 4)
    cams["fx"] = cams["fy"] = 512.0
    cams["invfx"] = cams["invfy"] = 1.0 / 512.0
    a = _row(kfs, cams, 4, (0.0, 0.0, 4.0), LAST, LAST, stereo1=True)
    a["k1"] = (480.0 + 64.0, 300.0 - 128.0)          # x = 64 * 4 / 512 = 0.5, y = -1.0, exactly
    a["depth1"] = 4.0
    a["sigma2_1"] = a["sigma2_2"] = 2.0 ** 40         # the reprojection gates let everything through
    cams[4 + LAST]["Ow"] = (0.5, -1.0, 4.0)
    c = _one_pair([a], kfs, cams, check=_expect((to.DIST_ZERO, 1)))
    c.exact = True
    return c


def _far(on):
    def build():
        kfs, cams = _two((1.0, 0.0, 0.3))
        near, far = _row(kfs, cams, 4, (0.5, -0.3, 8.0), LAST, LAST), _row(kfs, cams, 4, (0.5, -0.3, 16.0), LAST, LAST)
        return _one_pair([near, far], kfs, cams, far_points=on, th_far=12.0, check=_expect(to.OK, to.FAR if on else to.OK))
    return build


def _scale():
    kfs, cams = _two((1.0, 0.0, 6.0))
    # ahead: dist2 / dist1 = 0.5 against octaves that claim 1.2^4 (the first condition); with octaves that agree, OK;
    # behind, in the camera that looks back: dist2 / dist1 = 2 against equal octaves (the second condition)
    rows = [_row(kfs, cams, 4, FAR_X, LAST, LAST, o1=4, o2=0), _row(kfs, cams, 4, FAR_X, LAST, LAST, o1=0, o2=3),
            _row(kfs, cams, 4, (3.0, 0.2, -6.0), 1, 1)]

    def check(c, r):
        _expect(to.SCALE, to.OK, to.SCALE)(c, r)
        first = dict((n, (lhs, rhs)) for n, lhs, rhs, _ in r.cmp[0])["ratio*f<octave"]
        second = dict((n, (lhs, rhs)) for n, lhs, rhs, _ in r.cmp[2])["ratio>octave*f"]
        assert first[0] < first[1] and second[0] > second[1]
    return _one_pair(rows, kfs, cams, check=check)


def _stereo_sides():
    """stereo on side 1, on side 2, on both: with both, only cosStereo1 is computed (the `else if`)"""
    kfs, cams = _two((0.02, 0.0, 0.0))    # no ray parallax: the stereo point is all there is
    X = (0.2, 0.1, 5.0)
    s1, s2, both = (_row(kfs, cams, 4, X, LAST, LAST, stereo1=a, stereo2=b) for a, b in ((1, 0), (0, 1), (1, 1)))
    # both, with side 1 too far for its stereo to beat the rays and side 2 close: the reference never looks at side 2
    # and triangulates over the 2 cm baseline (a stereo side also switches the 0.9998 gate off)
    quirk = _row(kfs, cams, 4, X, LAST, LAST, stereo1=True, stereo2=True)
    quirk["depth1"] = 4096.0

    def check(c, r):
        assert [int(s) for s in r.stereo[:3]] == [1, 1, 1] and (r.status[:3] == to.OK).all(), (r.status, r.stereo)
        # back-projected from KF1 when both are stereo: X = k1's ray at depth1
        assert (r.X[2] == r.X[0]).all() and not (r.X[1] == r.X[0]).all()
        assert r.status[3] == to.OK and r.stereo[3] == 0 and r.triangulated[3]
    return _one_pair([s1, s2, both, quirk], kfs, cams, check=check)


def _stereo_or_triangulation():
    """a stereo point preferred over the triangulation (little ray parallax), and the reverse (a wide baseline)"""
    kfs, cams = _two((0.05, 0.0, 0.0))
    a = _row(kfs, cams, 4, (0.2, 0.1, 5.0), LAST, LAST, stereo1=True)    # baseline 5 cm < stereo 12 cm
    kfs2, cams2 = _two((1.0, 0.0, 0.0))
    b = _row(kfs2, cams2, 4, (0.2, 0.1, 5.0), LAST, LAST, stereo1=True)
    pairs = np.zeros(2, TRI_PAIR_DTYPE)
    pairs["kf1"], pairs["kf2"], pairs["row0"], pairs["n_rows"] = (0, 2), (1, 3), (0, 1), (1, 1)
    kfs2 = kfs2.copy()
    kfs2["cam0"] += 8
    return Case(pairs, np.array([a, b], TRI_ROW_DTYPE), np.concatenate([kfs, kfs2]), np.concatenate([cams, cams2]), 4,
                check=_expect((to.OK, 1), (to.OK, 0)))


def _ur_zero():
    """ur == 0 exactly is stereo (ur >= 0): the depth is read"""
    kfs, cams = _two((1.0, 0.0, 0.3))
    a = _row(kfs, cams, 4, FAR_X, LAST, LAST)
    a["ur1"], a["depth1"] = 0.0, 12.0
    b = _row(kfs, cams, 4, FAR_X, LAST, LAST)
    b["ur1"], b["depth1"] = -0.0, 12.0          # -0 >= 0 too
    c = _row(kfs, cams, 4, FAR_X, LAST, LAST)

    def check(cs, r):
        # stereo with an absurd ur fails the 7.8 gate of KF1; the mono row passes
        assert r.status[0] == to.REPROJ1 and r.status[1] == to.REPROJ1 and r.status[2] == to.OK
        assert any(n == "ur1>=0" and lhs == 0.0 for n, lhs, _, _ in r.cmp[0])
    return _one_pair([a, b, c], kfs, cams, check=check)


def _nan_keypoint():
    kfs, cams = _two((0.05, 0.0, 0.0))
    a = _row(kfs, cams, 4, (0.2, 0.1, 5.0), LAST, LAST, stereo1=True)
    a["k1"] = (np.nan, a["k1"][1])          # the raw keypoint: a NaN point through every gate
    kfs2, cams2 = _two((1.0, 0.0, 0.3))
    b = _row(kfs2, cams2, 4, FAR_X, LAST, LAST)
    b["z1"] = (np.nan, b["z1"][1])          # the undistorted one: cosRays is NaN, nothing is attempted
    pairs = np.zeros(2, TRI_PAIR_DTYPE)
    pairs["kf1"], pairs["kf2"], pairs["row0"], pairs["n_rows"] = (0, 2), (1, 3), (0, 1), (1, 1)
    kfs2 = kfs2.copy()
    kfs2["cam0"] += 8

    def check(c, r):
        assert r.status[0] == to.OK and r.stereo[0] == 1 and np.isnan(r.X[0]).any()
        assert r.status[1] == to.PARALLAX
    return Case(pairs, np.array([a, b], TRI_ROW_DTYPE), np.concatenate([kfs, kfs2]), np.concatenate([cams, cams2]), 4,
                check=check)


def _rank_deficient():
    """identical cameras: A's four rows lie in the span of the three rows of Tcw, sigma4 vanishes and the null vector
    is the camera centre, where z is rounding noise around its gate 0: status and X are reported, not compared"""
    kfs, cams = _two((0.0, 0.0, 0.0))
    b = _row(kfs, cams, 4, FAR_X, LAST, LAST, dz2=(40, 0))

    def check(c, r):
        assert r.triangulated[0] and r.sigma[0][3] < 1e-12 * r.sigma[0][0] and r.sigma[0][2] > 1e-3 * r.sigma[0][0]
    c = _one_pair([b], kfs, cams, check=check)
    c.reported = True
    return c


def _shuffled():
    c, _ = _gen(n_pairs=1, n_rows=97, seed=21)
    c.rows = c.rows[np.random.default_rng(3).permutation(97)]

    def check(c, r):
        ref, _ = _gen(n_pairs=1, n_rows=97, seed=21)
        want = to.run(ref.pairs, ref.rows, ref.kfs, ref.cams, 4, c.ratio).status
        assert (r.status == want[np.random.default_rng(3).permutation(97)]).all()
    c.check = check
    return c


def _shared_rows():
    """two pairs over the same rows (the second with another neighbour): the rows carry the later pair's result"""
    c, _ = _gen(n_pairs=2, n_rows=70, seed=22)
    c.pairs["row0"][1], c.pairs["n_rows"][1] = 30, 70
    c.pairs["n_rows"][0] = 60

    def check(c, r):
        later = Case(c.pairs[1:], c.rows, c.kfs, c.cams, 4)
        want = to.run(later.pairs, later.rows, later.kfs, later.cams, 4, c.ratio)
        assert (r.status[30:100] == want.status[30:100]).all()
        assert r.n_new[0] + r.n_new[1] > (r.status[:100] == to.OK).sum()     # the counts are per pair
    c.check = check
    return c


def _n_cam_1():
    c, _ = _gen(n_pairs=1, n_rows=80, n_cam=1, seed=23, baselines=(0.6,))
    c.check = _has(to.OK, stereo=0)
    return c


def _generated(seed, **kw):
    def build():
        c, _ = _gen(n_pairs=2, n_rows=150, seed=seed, **kw)

        def check(c, r):
            assert (r.status != to.PARALLAX).mean() >= 1 / 3
            assert (r.status == to.OK).any()
        c.check = check
        return c
    return build


def _ends_inside_chunk():
    c = _sized((70, 5, 130), 24)()
    return c


BUILDERS = {
    "rows_0": _sized((0,), 10),
    "rows_1": _sized((1,), 11),
    "rows_63_64_65": _sized((63, 64, 65), 12),
    "rows_255_256_257": _sized((255, 256, 257), 13),
    "ends_inside_chunk": _ends_inside_chunk,
    "n_cam_1": _n_cam_1,
    "generated": _generated(30),
    "generated_short_baseline": _generated(31, baselines=(0.5, 0.8), stereo_frac=1.0, depth_range=(2.0, 12.0)),
    "parallax": _parallax,
    "no_depth": _no_depth,
    "behind": _behind,
    "reproj": _reproj,
    "dist_zero": _dist_zero,
    "far_on": _far(1),
    "far_off": _far(0),
    "scale": _scale,
    "stereo_sides": _stereo_sides,
    "stereo_or_triangulation": _stereo_or_triangulation,
    "ur_zero": _ur_zero,
    "nan_keypoint": _nan_keypoint,
    "rank_deficient": _rank_deficient,
    "shuffled": _shuffled,
    "shared_rows": _shared_rows,
}
NAMES = list(BUILDERS)
STATUS_CASES = {to.PARALLAX: "parallax", to.NO_DEPTH: "no_depth", to.BEHIND1: "behind", to.BEHIND2: "behind",
                to.REPROJ1: "reproj", to.REPROJ2: "reproj", to.DIST_ZERO: "dist_zero", to.FAR: "far_on",
                to.SCALE: "scale", to.OK: "generated"}


def run_oracle(c, precision="f64"):
    return to.run(c.pairs, c.rows, c.kfs, c.cams, c.n_cam, c.ratio, c.far_points, c.th_far, precision)


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert len(c.pairs) <= 3 and (c.pairs["n_rows"] <= 257).all()
    return c, run_oracle(c), run_oracle(c, "f32")


def settled_rows(c, r64):
    """the rows of a case the device is compared on: covered by a pair and settled (tri_oracle.settled)"""
    if c.reported:
        return np.zeros(len(c.rows), bool)
    return c.in_pairs() & (np.ones(len(c.rows), bool) if c.exact else to.settled(r64))


def run_device(tracker, c):
    """(pairs, rows) of the device on copies of the case's arrays"""
    return tracker.triangulate(c.pairs.copy(), c.rows.copy(), c.kfs, c.cams, c.n_cam, c.params())


def x_bound(X, sigma):
    """what a triangulated X may differ by from the restatement's: the null vector within 2 * 64 * 4 u s1 / (s3 - s4)
    (tests/test_tri_math_host.py), through X = v.head(3) / w: |dX| <= |dv| (1 + |X|) / |w| and 1 / |w| =
    sqrt(1 + |X|^2) for a unit v"""
    nX = np.linalg.norm(X)
    return 2 * 64 * 4 * U * sigma[0] / (sigma[2] - sigma[3]) * (1 + nX) * np.sqrt(1 + nX * nX)


def gate_group(name):
    """the gates of one quantity share a margin: the cosines, the depths, the reprojection errors, the distances, the
    distance ratios"""
    for key, group in (("cos", "cos"), ("cs", "cos"), ("z1", "z"), ("z2", "z"), ("reproj", "reproj"), ("dist", "dist"), ("ratio", "ratio")):
        if key in name:
            return group
    raise KeyError(name)


def gate_differences(r64, r32, groups=None):
    """per row the largest relative difference of a gate quantity between the two runs, over the comparisons both
    evaluated (the common prefix of the two sequences), relative to max(|lhs|, |rhs|) of the fp64 run.  `groups`
    (a dict) collects the largest per gate_group."""
    out = np.zeros(len(r64.cmp))
    for i, (a, b) in enumerate(zip(r64.cmp, r32.cmp)):
        for (na, la, ra, ea), (nb, lb, rb, _) in zip(a, b):
            if na != nb:
                break
            scale = max(abs(la), abs(ra))
            if ea or not np.isfinite([la, ra, lb, rb]).all() or scale == 0:
                continue
            d = max(abs(la - lb), abs(ra - rb)) / scale
            out[i] = max(out[i], d)
            if groups is not None:
                groups[gate_group(na)] = max(groups.get(gate_group(na), 0.0), d)
    return out


def inside_f32_margin(cmps):
    """a computed comparison of the row lies within its gate's M_F32 of the gate"""
    for name, lhs, rhs, exact in cmps:
        scale = max(abs(lhs), abs(rhs))
        if exact or not np.isfinite(scale):
            continue
        if abs(lhs - rhs) <= M_F32[gate_group(name)] * scale:
            return True
    return False
