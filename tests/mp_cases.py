"""The named cases of lba_mappoint_refresh: each a small batch with the property it is there for (`check`, applied to the
refreshed points by tests/test_mp_cases.py on the restatements, and the same batch goes to the host build and the GPU).
`world` is a synthetic set of keyframes (amc_lba.mappoint.synthetic_keyframes) whose descriptors the cases overwrite.
`problems` are the generated batches the restatements, the host build and the mistake counts run on."""
import numpy as np

from amc_lba.abi import LBA_E_LIMIT, MP_OBS_DTYPE
from amc_lba.mappoint import MP_BAD, MP_EMPTY, MP_OK, make_mp_problem, pack_points, synthetic_keyframes
import mp_oracle as mo

F = np.float32
N_FEAT = 4            # keypoints per camera of a world
SEEDS = range(200)
GPU_SEEDS = (0, 1, 2)


class Case:
    def __init__(self, K, points, obs, kf_bad=None, check=None, refused=0):
        self.K, self.points, self.obs, self.kf_bad, self.check, self.refused = K, points, obs, kf_bad, check, refused


def world(n_kf=6, n_cam=4, seed=0, spread=2.0):
    return synthetic_keyframes(n_kf, n_cam, N_FEAT, np.random.default_rng([seed, 0xCA5E]), spread=spread)


def lst(*kcj):
    """an observation list from (keyframe, camera, j): the j-th keypoint of that camera"""
    out = np.zeros(len(kcj), MP_OBS_DTYPE)
    for i, (k, c, j) in enumerate(kcj):
        out[i] = (k, c * N_FEAT + j)
    return out


def bits(*ranges):
    """a descriptor with the bits of the given (lo, hi) ranges set"""
    d = np.zeros(8, np.uint32)
    for lo, hi in ranges:
        for b in range(lo, hi):
            d[b >> 5] |= np.uint32(1) << np.uint32(b & 31)
    return d


def set_desc(K, L, descs):
    for o, d in zip(L, descs):
        K.feats["desc"][int(K.ekfs["feat0"][o["kf"]]) + int(o["feat"])] = d


def one(K, L, pos=(0.5, -0.25, 4.0), ref=None, **kw):
    ref = int(L["kf"][0]) if ref is None and len(L) else (-1 if ref is None else ref)
    P, obs = pack_points([L], [pos], ref, **kw)
    P["normal"], P["min_distance"], P["max_distance"], P["desc"] = (7.0, 8.0, 9.0), 0.125, 77.0, np.arange(8) + 100
    return P, obs


def _best(i, med, st=MP_OK):
    def check(R):
        assert (int(R[0]["status"]), int(R[0]["best_obs"]), int(R[0]["best_median"])) == (st, i, med), R[0]
    return check


def _small_n(n):
    K = world()
    L = lst(*[(k, 1, 0) for k in range(n)])
    set_desc(K, L, [bits(), bits((0, 30)), bits((0, 40)), bits((0, 45))][:n])
    # D01 = 30, D02 = 40, D03 = 45, D12 = 10, D13 = 15, D23 = 5; positions 0, 0, 1, 1
    want = {1: (0, 0), 2: (0, 0), 3: (1, 10), 4: (2, 5)}[n]
    P, obs = one(K, L)
    return Case(K, P, obs, check=_best(*want))


def _all_equal():
    K = world()
    L = lst(*[(k, 0, 1) for k in range(5)])
    set_desc(K, L, [bits((3, 99))] * 5)
    P, obs = one(K, L)
    return Case(K, P, obs, check=_best(0, 0))


def _tie_first():
    K = world()
    L = lst(*[(k, 2, 0) for k in range(5)])
    # nested prefixes of lengths 100, 25, 25, 40, 41: D = |a - b|.  Sorted rows: [0,59,60,75,75] [0,0,15,16,75]
    # [0,0,15,16,75] [0,1,15,15,60] [0,1,16,16,59]; position 2: rows 1, 2 and 3 share the least median, row 1 wins
    set_desc(K, L, [bits((0, n)) for n in (100, 25, 25, 40, 41)])
    P, obs = one(K, L)
    return Case(K, P, obs, check=_best(1, 15))


def _tie_first_two_rows():
    K = world()
    L = lst(*[(k, 2, 1) for k in range(4)])
    set_desc(K, L, [bits((0, 50)), bits((0, 10)), bits((0, 20)), bits((10, 30))])
    # D01 = 40, D02 = 30, D03 = 30, D12 = 10, D13 = 30, D23 = 20: medians (position 1) 30, 10, 10, 20: row 1
    P, obs = one(K, L)
    return Case(K, P, obs, check=_best(1, 10))


def _complementary():
    K = world()
    L = lst((0, 0, 0), (1, 0, 0), (2, 0, 0))
    x = np.random.default_rng(5).integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)
    set_desc(K, L, [x, ~x, ~x])
    P, obs = one(K, L)       # row 0: [0, 256, 256] -> 256; rows 1, 2: [0, 0, 256] -> 0
    return Case(K, P, obs, check=_best(1, 0))


def _bad_kf_among():
    K = world()
    L = lst((0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0))
    set_desc(K, L, [bits(), bits((0, 200)), bits((0, 2)), bits((0, 4))])
    P, obs = one(K, L, ref=2)
    bad = np.array([1, 0, 0, 0, 0, 0], np.int32)     # keyframe 0 is skipped for the descriptor, counted in the normal

    def check(R):
        assert int(R[0]["n"]) == 4 and int(R[0]["best_obs"]) == 2 and int(R[0]["best_median"]) == 2, R[0]
    return Case(K, P, obs, bad, check)


def _all_kf_bad():
    K = world()
    L = lst((0, 0, 0), (1, 1, 0), (1, 2, 0))
    P, obs = one(K, L)

    def check(R):
        assert int(R[0]["best_obs"]) == -1 and R[0]["desc"].tolist() == P[0]["desc"].tolist()
        assert int(R[0]["n"]) == 3 and R[0]["normal"].tolist() != P[0]["normal"].tolist()
    return Case(K, P, obs, np.ones(6, np.int32), check)


def _untouched(status):
    def check(R):
        assert int(R[0]["status"]) == status and int(R[0]["n"]) == 0 and int(R[0]["best_obs"]) == -1
    return check


def _bad_point():
    K = world()
    P, obs = one(K, lst((0, 0, 0), (1, 0, 0)), bad=1)
    return Case(K, P, obs, check=_untouched(MP_BAD))


def _empty_list():
    K = world()
    P, obs = one(K, lst())
    return Case(K, P, obs, check=_untouched(MP_EMPTY))


def _ref_minus1():
    K = world()
    P, obs = one(K, lst((0, 0, 0), (2, 1, 0)), ref=-1)

    def check(R):
        assert R[0]["max_distance"] == mo.FLT_MIN and R[0]["min_distance"] == mo.FLT_MAX and int(R[0]["n"]) == 2
        assert np.isfinite(R[0]["normal"]).all()
    return Case(K, P, obs, check=check)


def _ref_cams(cams):
    K = world()
    L = lst((0, 1, 0), *[(3, c, 1) for c in cams], (5, 0, 0))
    P, obs = one(K, L, ref=3)

    def check(R):
        f = K.feats[K.ekfs["feat0"][3] + L["feat"][1:-1]]
        r = np.linalg.norm(P[0]["pos"].astype(float) - K.cams["Ow"][K.kfs["cam0"][3] + f["cam"]], axis=1)
        assert np.isclose(R[0]["max_distance"], (r * f["scale"]).max(), rtol=1e-5)
        assert np.isclose(R[0]["min_distance"], (r * f["scale"]).min() / K.scale_top, rtol=1e-5)
    return Case(K, P, obs, check=check)


def _multi_cam_midlist():
    K = world()
    P, obs = one(K, lst((0, 2, 0), (2, 0, 1), (2, 1, 1), (2, 3, 1), (4, 1, 0), (5, 3, 3)), ref=0)

    def check(R):
        assert int(R[0]["n"]) == 6 and int(R[0]["status"]) == MP_OK
    return Case(K, P, obs, check=check)


def _top_octave():
    K = world()
    L = lst((1, 0, 0), (2, 0, 0))
    K.feats["scale"][int(K.ekfs["feat0"][1]) + int(L["feat"][0])] = K.scale_top
    P, obs = one(K, L, ref=1)

    def check(R):
        r = np.linalg.norm(P[0]["pos"].astype(float) - K.cams["Ow"][K.kfs["cam0"][1]])
        assert np.isclose(R[0]["min_distance"], r, rtol=1e-6) and np.isclose(R[0]["max_distance"], r * K.scale_top, rtol=1e-6)
    return Case(K, P, obs, check=check)


def _coords(mag):
    K = world(spread=mag)
    P, obs = one(K, lst((0, 0, 0), (1, 1, 1), (3, 2, 2), (4, 3, 3)), pos=(1.5 * mag, -0.7 * mag, 2.2 * mag))

    def check(R):
        assert 0.0 < np.linalg.norm(R[0]["normal"].astype(float)) <= 1.0 + 1e-6
    return Case(K, P, obs, check=check)


def _on_centre():
    K = world()
    L = lst((0, 0, 0), (1, 1, 0), (2, 0, 0))
    P, obs = one(K, L, pos=K.centre(1, 1), ref=1)

    def check(R):
        assert np.isnan(R[0]["normal"]).all() and int(R[0]["n"]) == 3
        assert R[0]["max_distance"] == mo.FLT_MIN and R[0]["min_distance"] == 0.0     # max(FLT_MIN, 0), min(FLT_MAX, 0)
    return Case(K, P, obs, check=check)


def _ops(ops):
    K = world()
    P, obs = one(K, lst((0, 0, 0), (1, 1, 0), (2, 0, 0)), ops=ops)

    def check(R):
        same_geom = all(R[0][f].tobytes() == P[0][f].tobytes() for f in ("normal", "min_distance", "max_distance"))
        assert same_geom == (not ops & 1) and (int(R[0]["n"]) == 3) == bool(ops & 1)
        assert (int(R[0]["best_obs"]) >= 0) == bool(ops & 2)
        if not ops & 2:
            assert R[0]["desc"].tobytes() == P[0]["desc"].tobytes()
    return Case(K, P, obs, check=check)


def big_world():
    return synthetic_keyframes(70, 4, N_FEAT, np.random.default_rng([7, 0xCA5E]))


def long_list(K, n, rng):
    """n observations over the (keyframe, camera) slots in order, round after round"""
    slots = [(k, c) for k in range(len(K.kfs)) for c in range(K.n_cam)]
    rows = [(k, c, int(rng.integers(0, N_FEAT))) for i in range(n) for k, c in [slots[i % len(slots)]]]
    return lst(*sorted(rows[:n], key=lambda r: (r[0], r[1])))


def _big_n(n, refused=0, bad_share=0.0):
    K = big_world()
    rng = np.random.default_rng(n)
    P, obs = one(K, long_list(K, n, rng), pos=(0.3, 0.2, 9.0))
    bad = (rng.random(len(K.kfs)) < bad_share).astype(np.int32) if bad_share else None

    def check(R):
        assert int(R[0]["n"]) == n and 0 <= int(R[0]["best_obs"]) < n and 90 < int(R[0]["best_median"]) < 140
    return Case(K, P, obs, bad, None if refused else check, refused)


def _shuffled_shared():
    """points in an order unrelated to their lists, with shared and overlapping ranges of `obs`"""
    K = world(n_kf=12)
    rng = np.random.default_rng(11)
    obs = long_list(K, 48, rng)
    spans = [(0, 48), (0, 48), (5, 7), (40, 8), (10, 30), (11, 30), (47, 1), (3, 0), (20, 3), (0, 1)]
    spans = [spans[i] for i in rng.permutation(len(spans))]
    P, _ = pack_points([obs[a:a + n] for a, n in spans], rng.normal(0, 5, (len(spans), 3)), [int(obs["kf"][a]) for a, _ in spans])
    P["obs0"] = [a for a, _ in spans]
    P["desc"] = 5

    def check(R):
        n = [s[1] for s in spans]
        assert R["n"].tolist() == n and (R["status"] == np.where(np.array(n) > 0, MP_OK, MP_EMPTY)).all()
        same = [i for i, s in enumerate(spans) if s == (0, 48)]
        assert int(R[same[0]]["best_obs"]) == int(R[same[1]]["best_obs"])
    return Case(K, P, obs, check=check)


CASES = {
    "n1": lambda: _small_n(1), "n2": lambda: _small_n(2), "n3": lambda: _small_n(3), "n4": lambda: _small_n(4),
    "all_equal": _all_equal, "tie_first": _tie_first, "tie_first_two_rows": _tie_first_two_rows,
    "complementary": _complementary, "bad_kf_among": _bad_kf_among, "all_kf_bad": _all_kf_bad, "bad_point": _bad_point,
    "empty_list": _empty_list, "ref_minus1": _ref_minus1, "ref_two_cams": lambda: _ref_cams((1, 3)),
    "ref_all_cams": lambda: _ref_cams((0, 1, 2, 3)), "multi_cam_midlist": _multi_cam_midlist, "top_octave": _top_octave,
    "coords_1e4": lambda: _coords(1e4), "coords_1e-3": lambda: _coords(1e-3), "on_centre": _on_centre,
    "ops_1": lambda: _ops(1), "ops_2": lambda: _ops(2), "ops_3": lambda: _ops(3),
    "n63": lambda: _big_n(63), "n64": lambda: _big_n(64), "n65": lambda: _big_n(65),
    "n200_some_bad": lambda: _big_n(200, bad_share=0.3), "n1024": lambda: _big_n(1024),
    "n1025_refused": lambda: _big_n(1025, refused=LBA_E_LIMIT), "shuffled_shared": _shuffled_shared,
}
NAMES = tuple(CASES)
_made = {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


_ref = {}


def reference(name):
    """the vectorised restatement of a case, computed once and shared"""
    if name not in _ref:
        c = case(name)
        _ref[name] = mo.refresh_batch(c.points, c.obs, c.K, c.kf_bad)
    return _ref[name]


def problem(seed):
    """the generated batch of a seed: both scenes in turn, every fourth with long tracks"""
    return make_mp_problem(seed, scene="epipolar" if seed % 5 == 4 else "fuse", n_kf=5, n_cam=3 + seed % 2, n_feat=24,
                           n_points=40, long_tracks=1 if seed % 4 == 0 else 0, long_obs=(65, 90))


def gpu_problem(seed):
    """about 2000 points with both size classes"""
    return make_mp_problem(1000 + seed, n_kf=10, n_cam=4, n_feat=500, n_points=1900, long_tracks=6, long_obs=(65, 300))


def order_matters():
    """a list and a permutation of it whose normals differ in their bits (the sum is pinned to list order)"""
    K = world(n_kf=8, seed=3)
    rng = np.random.default_rng(3)
    for _ in range(100):
        L = long_list(K, 12, rng)
        perm = L[::-1].copy()
        P, obs = one(K, L, pos=rng.normal(0, 4, 3))
        P2, obs2 = one(K, perm, pos=P[0]["pos"], ref=int(L["kf"][0]))
        a, b = mo.refresh_vec(P[0], obs, K), mo.refresh_vec(P2[0], obs2, K)
        if a["normal"].tobytes() != b["normal"].tobytes():
            return (K, P, obs), (K, P2, obs2), a, b
    raise AssertionError("no permutation changed the normal's bits")
