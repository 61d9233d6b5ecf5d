"""Named cases of lba_match_epipolar at the smallest shapes where the kernel can go wrong, each with the property the
CPU test asserts on the restatement (tests/epi_oracle.py) and the GPU test thereby on the device.

`case(name)` -> (Case, [Result per pair] of `sequential` in fp64, [settled mask per pair]); computed once and shared.
A Case holds the arrays of the call; `prop(case, results)` asserts the case's property on a list of Results.

M_F32: the margin below which the reference's float evaluation may decide a job differently from fp64.  MEASURED
(tests/test_epi_cases.py::test_float32_agrees_outside_the_margin prints it) over the named cases and the 200 generator
seeds, both precisions run on each: no job of 22660 was decided differently, so there is no gate distance "at which they
disagree" to take; what is taken instead is the largest relative difference between the float and the fp64 value of a
gate quantity (the squared epipole distance, dsqr), measured against the larger side of its comparison: 7.97e-3 (F12
in float loses digits to the cancellation in [t12]x R12).  M_F32 is 4 x that."""
import functools
from collections import namedtuple

import numpy as np

import epi_oracle as eo
from amc_lba.abi import TRI_CAM_DTYPE, TRI_KF_DTYPE
from amc_lba.epipolar import EPI_FEAT_DTYPE, epi_pairs, make_epi_pairs, pack_epi_keyframes
from amc_lba.match import flip_bits
from amc_lba.synth import _rotz
from amc_lba.triangulate import _RBC0, TRI_K, scale_pyramid, tri_keyframes, tri_project

M_F32_FACTOR = 4
M_F32_SEEN = 7.97e-3
M_F32 = M_F32_FACTOR * M_F32_SEEN
MAX_UNSETTLED = 0.02

Case = namedtuple("Case", "pairs kfs ekfs cams n_cam feats node_id node_start node_feat prm prop")
SF, SIG2 = scale_pyramid(8)
FX, FY, CX, CY = TRI_K
SIDE = (_RBC0, _RBC0 @ np.array([0.8, 0.1, 0.3]))       # the neighbour mostly to the side of the current keyframe
ORIGIN = (_RBC0, np.zeros(3))


def kp(xy, cam=0, desc=None, node=0, has_point=0, u_right=-1.0, octave=0, angle=0.0):
    return dict(xy=xy, cam=cam, desc=desc, node=node, has_point=has_point, u_right=u_right, octave=octave, angle=angle)


def _feats(kps):
    f = np.zeros(len(kps), EPI_FEAT_DTYPE)
    for i, k in enumerate(kps):
        f[i]["x"], f[i]["y"] = k["xy"]
        f[i]["angle"], f[i]["u_right"], f[i]["cam"], f[i]["has_point"] = k["angle"], k["u_right"], k["cam"], k["has_point"]
        f[i]["scale"], f[i]["sigma2"], f[i]["desc"] = SF[k["octave"]], SIG2[k["octave"]], k["desc"]
    return f


def build(kf_kps, pair_idx, poses, n_cam, prop, prm=None, records=None):
    kfs, cams = records if records is not None else tri_keyframes(poses, n_cam)
    ekfs, feats, nid, nst, nf = pack_epi_keyframes([_feats(k) for k in kf_kps], [[k["node"] for k in ks] for ks in kf_kps])
    pairs = epi_pairs([p[0] for p in pair_idx], [p[1] for p in pair_idx], ekfs)
    return Case(pairs, kfs, ekfs, cams, n_cam, feats, nid, nst, nf, dict(prm or {}), prop)


class Geo:
    """two keyframes and true correspondences between them"""

    def __init__(self, n_cam=2, poses=(ORIGIN, SIDE), seed=0):
        self.n_cam, self.poses = n_cam, list(poses)
        self.kfs, self.cams = tri_keyframes(self.poses, n_cam)
        self.rng = np.random.default_rng([seed, 0xE7])

    def base(self):
        return self.rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)

    def near(self, base, d):
        return flip_bits(base, d, self.rng)

    def corr(self, c1=0, c2=0, uv=None, z=None):
        """a world point `z` metres in front of pixel `uv` of KF1's camera c1: its keypoints in (KF1 c1, KF2 c2)"""
        drawn = uv is None
        ep = eo.table(self.cams[c1], self.cams[self.n_cam + c2])[1]
        while True:
            uv = np.array([self.rng.uniform(200, 760), self.rng.uniform(150, 450)]) if drawn else np.asarray(uv, float)
            zz = self.rng.uniform(5.0, 15.0) if z is None else z
            T1 = self.cams[c1]["Tcw"].reshape(3, 4)
            Xw = T1[:, :3].T @ (np.array([(uv[0] - CX) / FX * zz, (uv[1] - CY) / FY * zz, zz]) - T1[:, 3])
            p1, p2 = tri_project(self.cams[c1], Xw), tri_project(self.cams[self.n_cam + c2], Xw)
            assert p1[2] > 0 and p2[2] > 0, "the point is behind a camera"
            if not drawn or not np.hypot(*(ep - p2[:2])) < 60.0:     # a drawn point keeps clear of the epipole test
                return np.float32(p1[:2]), np.float32(p2[:2])


def _status(res, *want):
    assert tuple(int(s) for s in res.status) == want, res.status


def _simple(kps1, kps2, prop, g, prm=None):
    return build([kps1, kps2], [(0, 1)], g.poses, g.n_cam, prop, prm)


# ------------------------------------------------------------------------------------------------ shapes, node structure

def _one_by_one():
    g = Geo()
    a, b = g.corr()
    B = g.base()

    def prop(c, r):
        assert r[0].idx2[0] == 0 and r[0].dist[0] == 10 and r[0].n_matches == 1
        _status(r[0], eo.OK)
    return _simple([kp(a, desc=B)], [kp(b, desc=g.near(B, 10))], prop, g)


def _chunk(n):
    def make():
        g = Geo(seed=n)
        k1, k2 = [], []
        for _ in range(n):
            a, b = g.corr()
            B = g.base()
            k1.append(kp(a, desc=B))
            k2.append(kp(b, desc=g.near(B, 5)))

        def prop(c, r):
            assert (r[0].idx2 == np.arange(n)).all() and (r[0].dist == 5).all() and r[0].n_matches == n
        return _simple(k1, k2, prop, g)
    return make


def _span2(n):
    def make():
        g = Geo(seed=100 + n)
        a, b = g.corr()
        B = g.base()
        k2 = [kp((g.rng.uniform(0, 960), g.rng.uniform(0, 600)), desc=g.base()) for _ in range(n - 1)] + [kp(b, desc=g.near(B, 7))]

        def prop(c, r):
            assert r[0].idx2[0] == n - 1 and r[0].dist[0] == 7 and r[0].n_matches == 1
        return _simple([kp(a, desc=B)], k2, prop, g)
    return make


def _node_all_ineligible():
    g = Geo()
    k1, k2 = [], []
    for _ in range(3):
        a, b = g.corr()
        B = g.base()
        k1.append(kp(a, desc=B, has_point=1))
        k2.append(kp(b, desc=B))

    def prop(c, r):
        _status(r[0], eo.HAS_POINT, eo.HAS_POINT, eo.HAS_POINT)
        assert r[0].n_matches == 0 and (r[0].idx2 == -1).all() and (r[0].dist == 50).all()
    return _simple(k1, k2, prop, g)


def _nodes(ids1, ids2, want):
    def make():
        g = Geo(seed=7)
        k1, k2 = [], []
        for n1, n2 in zip(ids1, ids2):
            a, b = g.corr()
            B = g.base()
            k1.append(kp(a, desc=B, node=n1))
            k2.append(kp(b, desc=g.near(B, 3), node=n2))

        def prop(c, r):
            _status(r[0], *want)
            assert r[0].n_matches == sum(w == eo.OK for w in want)
            assert all(r[0].idx2[i] == i for i, w in enumerate(want) if w == eo.OK)
        return _simple(k1, k2, prop, g)
    return make


def _empty_kf2():
    g = Geo()
    a, _ = g.corr()

    def prop(c, r):
        _status(r[0], eo.NO_NODE, eo.NO_NODE)
        assert r[0].n_matches == 0
    return _simple([kp(a, desc=g.base()), kp(a, desc=g.base(), node=2)], [], prop, g)


def _n_feat_0():
    g = Geo()
    _, b = g.corr()

    def prop(c, r):
        assert len(r[0].status) == 0 and r[0].n_matches == 0
    return _simple([], [kp(b, desc=g.base())], prop, g)


def _cross_camera():
    g = Geo(n_cam=3, poses=(ORIGIN, (_rotz(np.pi / 2) @ _RBC0, _RBC0 @ np.array([0.6, 0.1, 0.4]))))
    a, b = g.corr(c1=0, c2=2, uv=(430.0, 280.0), z=9.0)
    B = g.base()

    def prop(c, r):
        assert r[0].idx2[0] == 0 and r[0].n_matches == 1
    return _simple([kp(a, cam=0, desc=B)], [kp(b, cam=2, desc=g.near(B, 4))], prop, g)


# ------------------------------------------------------------------------------------------------------ distances and ties

def _two_candidates(d_first, d_second, second_off_line, want_idx2, want_dist, **kw):
    def make():
        g = Geo(seed=11)
        a, b = g.corr()
        B = g.base()
        b2 = np.float32(b + np.array([0.0, 40.0])) if second_off_line else b
        k2 = [kp(b, desc=g.near(B, d_first), **kw.get("first", {})), kp(b2, desc=g.near(B, d_second))]

        def prop(c, r):
            assert r[0].idx2[0] == want_idx2 and r[0].dist[0] == want_dist and r[0].n_matches == 1
        return _simple([kp(a, desc=B)], k2, prop, g)
    return make


def _dist_50_51():
    g = Geo(seed=12)
    k1, k2 = [], []
    for d in (50, 51):
        a, b = g.corr()
        B = g.base()
        k1.append(kp(a, desc=B))
        k2.append(kp(b, desc=g.near(B, d)))

    def prop(c, r):
        _status(r[0], eo.OK, eo.NO_MATCH)
        assert r[0].dist[0] == 50 and r[0].idx2[1] == -1 and r[0].dist[1] == 50
    return _simple(k1, k2, prop, g)


def _shared_idx2():
    g = Geo(seed=13)
    a, b = g.corr()
    B = g.base()

    def prop(c, r):
        assert (r[0].idx2 == 0).all() and r[0].n_matches == 2           # quirk (a): vbMatched2 is never set
    return _simple([kp(a, desc=B), kp(a, desc=g.near(B, 2))], [kp(b, desc=g.near(B, 6))], prop, g)


def _th_low_0():
    g = Geo(seed=14)
    k1, k2 = [], []
    for d in (0, 1):
        a, b = g.corr()
        B = g.base()
        k1.append(kp(a, desc=B))
        k2.append(kp(b, desc=g.near(B, d)))

    def prop(c, r):
        _status(r[0], eo.OK, eo.NO_MATCH)
        assert r[0].dist[0] == 0 and r[0].dist[1] == 0
    return _simple(k1, k2, prop, g, dict(th_low=0))


# ---------------------------------------------------------------------------------------------------------- skips and flags

def _has_point_kf1():
    g = Geo(seed=15)
    a, b = g.corr()
    B = g.base()

    def prop(c, r):
        _status(r[0], eo.HAS_POINT, eo.OK)
    return _simple([kp(a, desc=B, has_point=1), kp(a, desc=B)], [kp(b, desc=B)], prop, g)


def _only_stereo(u_right):
    def make():
        g = Geo(seed=16)
        a, b = g.corr(c1=1, c2=1)
        m, _ = g.corr(c1=0, c2=0)
        B = g.base()
        k1 = [kp(m, cam=0, desc=B), kp(a, cam=1, desc=B, u_right=u_right), kp(a, cam=1, desc=B, u_right=-1.0)]
        k2 = [kp(b, cam=1, desc=g.near(B, 5), u_right=-1.0), kp(b, cam=1, desc=g.near(B, 20), u_right=u_right),
              kp(b, cam=0, desc=g.near(B, 3), u_right=u_right)]      # u_right outside the last camera is not stereo

        def prop(c, r):
            _status(r[0], eo.NOT_STEREO, eo.OK, eo.NOT_STEREO)
            assert r[0].idx2[1] == 1 and r[0].dist[1] == 20
        return _simple(k1, k2, prop, g, dict(only_stereo=1))
    return make


def _coarse():
    g = Geo(seed=17)
    a, b = g.corr()
    B = g.base()

    def prop(c, r):
        assert r[0].idx2[0] == 0 and r[0].n_matches == 1
        assert eo.sequential(eo.jobs_of(c)[0]._replace(prm=dict(eo.PRM, coarse=0))).n_matches == 0
    return _simple([kp(a, desc=B)], [kp(np.float32(b + np.array([0.0, 60.0])), desc=g.near(B, 10))], prop, g, dict(coarse=1))


# ------------------------------------------------------------------------------------------------------- epipole and gate

BACK = (_RBC0, _RBC0 @ np.array([0.02, 0.01, -1.0]))     # the neighbour behind the current keyframe: the epipole ahead
AHEAD = (_RBC0, _RBC0 @ np.array([0.02, 0.01, 1.0]))     # the neighbour ahead: the current centre behind it (z < 0)


def _epipole(pose2, stereo2, want, z_sign, uv):
    def make():
        g = Geo(n_cam=2, poses=(ORIGIN, pose2), seed=18)
        a, b = g.corr(c1=1, c2=1, uv=uv, z=12.0)     # close to the baseline's direction
        B = g.base()
        ur = 0.5 if stereo2 else -1.0

        def prop(c, r):
            _status(r[0], want)
            j = eo.jobs_of(c)[0]
            F, ep = eo.table(j.cams1[1], j.cams2[1])
            T2 = j.cams2[1]["Tcw"].reshape(3, 4)
            assert np.sign((T2[:, :3] @ j.cams1[1]["Ow"] + T2[:, 3])[2]) == z_sign
            assert eo.near_epipole(ep, j.f2[0], np.float64)[0] and eo.epi_gate(F, j.f1[0], j.f2[0], np.float64)[0]
        return _simple([kp(a, cam=1, desc=B)], [kp(b, cam=1, desc=g.near(B, 8), u_right=ur)], prop, g)
    return make


def _plain_records(t1, t2):
    """one camera per keyframe with R = I and the integer translations t1, t2: exactly representable"""
    kfs, cams = np.zeros(2, TRI_KF_DTYPE), np.zeros(2, TRI_CAM_DTYPE)
    for k, t in enumerate((t1, t2)):
        kfs[k]["Rwb"], kfs[k]["twb"], kfs[k]["cam0"] = np.eye(3).ravel(), -np.asarray(t, float), k
        cams[k]["Tcw"] = np.hstack([np.eye(3), np.asarray(t, float)[:, None]]).ravel()
        cams[k]["Ow"] = -np.asarray(t, float)
        cams[k]["fx"], cams[k]["fy"], cams[k]["cx"], cams[k]["cy"] = FX, FY, CX, CY
        cams[k]["invfx"], cams[k]["invfy"] = 1.0 / FX, 1.0 / FY
    return kfs, cams


def _epipole_z_zero():
    rec = _plain_records((0, 0, 0), (-1, 0, 0))          # C1 in KF2's camera is (-1, 0, 0): z == 0
    X = np.array([0.5, 0.25, 8.0])
    a, b = tri_project(rec[1][0], X)[:2], tri_project(rec[1][1], X)[:2]
    rng = np.random.default_rng(19)
    B = rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)

    def prop(c, r):
        _, ep = eo.table(c.cams[0], c.cams[1])
        assert not np.isfinite(ep).all()
        assert r[0].idx2[0] == 0 and r[0].n_matches == 1             # quirk (e): nothing is skipped
    return build([[kp(np.float32(a), desc=B)], [kp(np.float32(b), desc=flip_bits(B, 9, rng))]], [(0, 1)], None, 1, prop,
                 records=rec)


def _den_zero():
    rec = _plain_records((2, 3, 4), (2, 3, 4))           # equal integer centres: t12 is exactly 0
    rng = np.random.default_rng(20)
    B = rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)
    ks = [kp((400.0, 300.0), desc=B), kp((500.0, 200.0), desc=flip_bits(B, 12, rng))]

    def prop(c, r):
        F, _ = eo.table(c.cams[0], c.cams[0])
        assert (F == 0).all()
        _status(r[0], eo.NO_MATCH, eo.NO_MATCH)                       # quirk (f)
        _status(r[1], eo.NO_MATCH, eo.NO_MATCH)
        for j in eo.jobs_of(c):
            assert eo.sequential(j._replace(prm=dict(eo.PRM, coarse=1))).n_matches == 2
    return build([ks, ks], [(0, 0), (0, 1)], None, 1, prop, records=rec)     # kf1 == kf2, and a twin of it


def _unc_is_kf2_level():
    g = Geo(seed=21)
    a, b = g.corr()
    B = g.base()

    def prop(c, r):
        assert r[0].idx2[0] == 0 and r[0].n_matches == 1
        assert eo.sequential(eo.jobs_of(c)[0], kp1_sigma=True).n_matches == 0      # quirk (d)
    return _simple([kp(a, desc=B, octave=0)], [kp(np.float32(b + np.array([0.0, 3.0])), desc=g.near(B, 10), octave=4)], prop, g)


# ------------------------------------------------------------------------------------------ rotation, batch, generated

def _rotation(diffs, want_rot, want_n):
    def make():
        g = Geo(seed=22)
        k1, k2 = [], []
        for d in diffs:
            a, b = g.corr()
            B = g.base()
            k1.append(kp(a, desc=B, angle=d))
            k2.append(kp(b, desc=g.near(B, 5), angle=0.0))

        def prop(c, r):
            assert (r[0].status == eo.ROT).sum() == want_rot and r[0].n_matches == want_n
            assert (r[0].idx2 == np.arange(len(diffs))).all()                        # idx2 is kept under LBA_EPI_ROT
        return _simple(k1, k2, prop, g, dict(check_orientation=1))
    return make


def generated(n_pairs, n_cam, n_feat, n_nodes, seed, prm=None, **kw):
    a = make_epi_pairs(n_pairs, n_cam, n_feat, n_nodes, seed, **kw)

    def prop(c, r):
        assert all(x.n_matches > 0 for x in r) and any((x.status == eo.NO_MATCH).any() for x in r)
    return Case(a[0], a[1], a[2], a[3], n_cam, a[4], a[5], a[6], a[7], dict(prm or {}), prop)


CASES = {
    "one_by_one": _one_by_one,
    "chunk_63": _chunk(63), "chunk_64": _chunk(64), "chunk_65": _chunk(65),
    "span2_1": _span2(1), "span2_64": _span2(64), "span2_65": _span2(65), "span2_257": _span2(257),
    "node_all_ineligible": _node_all_ineligible,
    "nodes_disjoint": _nodes((1, 3), (2, 4), (eo.NO_NODE, eo.NO_NODE)),
    "nodes_interleaved": _nodes((1, 3, 5, 7, 9, 11), (2, 3, 6, 7, 10, 11), (eo.NO_NODE, eo.OK) * 3),
    "node_only_in_kf1": _nodes((0, 1), (0, 0), (eo.OK, eo.NO_NODE)),
    "keypoint_in_no_node": _nodes((0, -1, 0), (0, 0, 0), (eo.OK, eo.NO_NODE, eo.OK)),
    "empty_kf2": _empty_kf2, "n_feat_0": _n_feat_0,
    "cross_camera": _cross_camera,
    "tie_last_wins": _two_candidates(20, 20, False, 1, 20),
    "tie_later_fails_gate": _two_candidates(20, 20, True, 0, 20),
    "dist_50_51": _dist_50_51,
    "dist_shrinks": _two_candidates(10, 30, False, 0, 10),
    "shared_idx2": _shared_idx2,
    "th_low_0": _th_low_0,
    "has_point_kf1": _has_point_kf1,
    "has_point_kf2": _two_candidates(5, 20, False, 1, 20, first=dict(has_point=1)),
    "only_stereo": _only_stereo(37.5),
    "stereo_u_right_0": _only_stereo(0.0),
    "coarse": _coarse,
    "epipole_gate_mono": _epipole(BACK, False, eo.NO_MATCH, 1.0, (CX - 8.0, CY - 3.5)),
    "epipole_gate_stereo_exempt": _epipole(BACK, True, eo.OK, 1.0, (CX - 8.0, CY - 3.5)),
    "epipole_behind": _epipole(AHEAD, False, eo.NO_MATCH, -1.0, (CX + 12.0, CY + 6.5)),
    "epipole_z_zero": _epipole_z_zero,
    "den_zero": _den_zero,
    "unc_is_kf2_level": _unc_is_kf2_level,
    "rotation_maxima_removed": _rotation((30.0,) * 11 + (300.0,), 11, 1),
    "rotation_single_bin": _rotation((60.0,) * 4, 4, 0),
    "kf1_in_20_pairs": lambda: generated(20, 2, 40, 6, 31),
    "generated_4x400": lambda: generated(1, 4, 400, 40, 32),
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    jobs = eo.jobs_of(c)
    return c, [eo.sequential(j) for j in jobs], [eo.settled(j) for j in jobs]


def run_device(tracker, c, junk=True):
    """the case on the device: (pairs, out); n_matches pre-filled with junk, `out` is the binding's own"""
    from amc_lba.epipolar import epi_params
    pairs = c.pairs.copy()
    if junk:
        pairs["n_matches"] = -77
    return tracker.match_epipolar(pairs, c.kfs, c.ekfs, c.cams, c.n_cam, c.feats, c.node_id, c.node_start, c.node_feat,
                                  epi_params(**dict(eo.PRM, **c.prm)))
