"""Named cases of lba_match_bow at the smallest shapes where the kernel can go wrong, each with the property the CPU
test asserts on the restatement (tests/bow_oracle.py) and the GPU test thereby on the device.

`case(name, mode)` -> (Case, [Result per pair] of `sequential`); computed once and shared.  A Case holds the arrays of
the call; `prop(case, results)` asserts the case's property on a list of Results.  Every case exists in both overloads
(mode bo.KF / bo.FRAME); where the overloads differ the property says how.

Descriptors with chosen distances: L(n) has its first n bits set, so dist(L(a), L(b)) = |a - b|; `far(rng)` is a random
descriptor, about 128 from everything."""
import functools
from collections import namedtuple

import numpy as np

import bow_oracle as bo
from amc_lba.abi import EPI_FEAT_DTYPE, EPI_KF_DTYPE
from amc_lba.bow import BOW_LDS_CAP, BOW_MAX_NODE, bow_pairs, make_bow_pairs
from amc_lba.epipolar import pack_epi_keyframes
from amc_lba.match import flip_bits

Case = namedtuple("Case", "pairs ekfs feats node_id node_start node_feat prm prop")
MODES = (bo.KF, bo.FRAME)
MODE_NAMES = {bo.KF: "kf", bo.FRAME: "frame"}


def L(n):
    bits = np.zeros(256, np.uint8)
    bits[:n] = 1
    return np.packbits(bits, bitorder="little").view("<u4").copy()


def far(rng):
    return rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)


def kp(desc, node=0, has_point=1, angle=0.0):
    return dict(desc=desc, node=node, has_point=has_point, angle=angle)


def _feats(kps):
    f = np.zeros(len(kps), EPI_FEAT_DTYPE)
    f["u_right"], f["scale"], f["sigma2"] = -1.0, 1.0, 1.0
    for i, k in enumerate(kps):
        f[i]["desc"], f[i]["has_point"], f[i]["angle"] = k["desc"], k["has_point"], k["angle"]
    return f


def build(kf_kps, pair_idx, prop, mode, **prm):
    ekfs, feats, nid, nst, nf = pack_epi_keyframes([_feats(k) for k in kf_kps], [[k["node"] for k in ks] for ks in kf_kps])
    pairs = bow_pairs([p[0] for p in pair_idx], [p[1] for p in pair_idx], ekfs)
    return Case(pairs, ekfs, feats, nid, nst, nf, dict(dict(check_orientation=0, mode=mode), **prm), prop)


def _status(res, *want):
    assert tuple(int(s) for s in res.status) == want, res.status


def _row(res, i, idx2, dist, dist2, status):
    got = (int(res.idx2[i]), int(res.dist[i]), int(res.dist2[i]), int(res.status[i]))
    assert got == (idx2, dist, dist2, status), (i, got, (idx2, dist, dist2, status))


# ------------------------------------------------------------------------------------------------ shapes

def _list2(n2):
    """side 2's list of n2 entries: the partner of keypoint 0 is its LAST entry, of keypoint 1 its first, of keypoint 2
    the one in the middle; keypoint 3 has no partner"""
    def make(mode):
        rng = np.random.default_rng([n2, 0xB1])
        B = [far(rng) for _ in range(4)]
        k2 = [kp(far(rng)) for _ in range(n2)]
        want = {0: n2 - 1, 1: 0, 2: n2 // 2}
        want = {i: p for i, p in want.items() if n2 > 0 and list(want.values()).index(p) == i}     # a position once
        for i, p in want.items():
            k2[p] = kp(flip_bits(B[i], 7 + i, rng))
        k1 = [kp(b) for b in B]

        def prop(c, r):
            for i in range(4):
                if n2 == 0:
                    _row(r[0], i, -1, 256, 256, bo.NO_NODE)
                elif i in want:
                    assert (r[0].idx2[i], r[0].dist[i], r[0].status[i]) == (want[i], 7 + i, bo.OK), (i, r[0])
                    # (256 where the other candidates are all matched by then)
                    assert r[0].dist2[i] == 256 if n2 == 1 else 50 < r[0].dist2[i] <= 256
                else:
                    assert r[0].status[i] == bo.NO_CAND and (n2 <= len(want) or r[0].dist[i] > 50)
            assert r[0].n_matches == len(want)
        return build([k1, k2], [(0, 1)], prop, mode)
    return make


def _empty_list2(mode):
    """the node is in both sides' vectors, side 2's list of it is empty (a hand-made CSR): the inner loop runs over
    nothing, the threshold fails"""
    f = _feats([kp(L(3), node=5), kp(L(3), node=-1)])
    ekfs = np.zeros(2, EPI_KF_DTYPE)
    ekfs[0], ekfs[1] = (0, 1, 0, 1, 0, 0), (1, 1, 2, 1, 1, 0)
    nid, nst, nf = np.array([5, -1, 5, -1], np.int32), np.array([0, 1, 0, 0], np.int32), np.array([0], np.int32)

    def prop(c, r):
        _row(r[0], 0, -1, 256, 256, bo.NO_CAND)
        assert r[0].n_matches == 0
    return Case(bow_pairs(0, [1], ekfs), ekfs, f, nid, nst, nf, dict(check_orientation=0, mode=mode), prop)


def _list1(n1):
    """side 1's list of n1 entries against n1 + 5 candidates, every keypoint with its own partner, in reverse order"""
    def make(mode):
        rng = np.random.default_rng([n1, 0xB2])
        B = [far(rng) for _ in range(n1)]
        k2 = [kp(far(rng)) for _ in range(5)] + [kp(flip_bits(b, 6, rng)) for b in B[::-1]]

        def prop(c, r):
            assert (r[0].idx2 == 5 + np.arange(n1)[::-1]).all() and (r[0].dist == 6).all() and r[0].n_matches == n1
            assert (r[0].status == bo.OK).all()
        return build([[kp(b) for b in B], k2], [(0, 1)], prop, mode)
    return make


# ------------------------------------------------------------------------------------------------ ties

def _tie_position_not_lane(mode):
    """130 candidates.  Keypoint 0 (at L(100)) has its minimum twice: position 65 (chunk 1, lane 1) and position 40
    (chunk 0, lane 40); keypoint 1 (at L(200)) at positions 5 and 69 (both lane 5).  The first POSITION wins.  With
    nn_ratio 1.5 the tie is accepted and sets the flag of the right one: keypoint 2, a copy of keypoint 0, then gets
    position 65."""
    rng = np.random.default_rng(0xB3)
    k2 = [kp(far(rng)) for _ in range(130)]
    k2[40], k2[65] = kp(L(110)), kp(L(90))
    k2[5], k2[69] = kp(L(204)), kp(L(196))

    def prop(c, r):
        _row(r[0], 0, 40, 10, 10, bo.OK)
        _row(r[0], 1, 5, 4, 4, bo.OK)
        assert (r[0].idx2[2], r[0].dist[2], r[0].status[2]) == (65, 10, bo.OK) and r[0].dist2[2] > 50
    return build([[kp(L(100)), kp(L(200)), kp(L(100))], k2], [(0, 1)], prop, mode, nn_ratio=1.5)


def _best_tied_with_second(mode):
    """b1 == b2 fails the ratio test at 0.9, and so does (0, 0): 0 < 0.9 * 0 is false"""
    k1 = [kp(L(100), node=0), kp(L(30), node=1)]
    k2 = [kp(L(108), node=0), kp(L(92), node=0), kp(L(30), node=1), kp(L(30), node=1)]

    def prop(c, r):
        _row(r[0], 0, 0, 8, 8, bo.RATIO)
        _row(r[0], 1, 2, 0, 0, bo.RATIO)
        assert r[0].n_matches == 0
    return build([k1, k2], [(0, 1)], prop, mode)


def _b1_zero(mode):
    def prop(c, r):
        _row(r[0], 0, 1, 0, 5, bo.OK)
    return build([[kp(L(60))], [kp(L(65)), kp(L(60))]], [(0, 1)], prop, mode)


def _complement(mode):
    """a candidate at distance 256 never becomes best: bestIdx2 stays -1"""
    def prop(c, r):
        _row(r[0], 0, -1, 256, 256, bo.NO_CAND)
        _row(r[0], 1, 1, 0, 256, bo.OK)       # (and is no second best either)
    return build([[kp(L(0), node=0), kp(L(256), node=1)], [kp(L(256), node=0), kp(L(256), node=1), kp(L(0), node=1)]],
                 [(0, 1)], prop, mode)


def _threshold(mode):
    """distances 49 / 50 / 51 at th_low 50: `<` in the keyframe overload, `<=` in the frame overload"""
    k1 = [kp(L(100), node=n) for n in range(3)]
    k2 = [kp(L(100 + d), node=n) for n, d in enumerate((49, 50, 51))]

    def prop(c, r):
        _status(r[0], bo.OK, bo.OK if mode == bo.FRAME else bo.NO_CAND, bo.NO_CAND)
        assert r[0].dist.tolist() == [49, 50, 51] and r[0].idx2.tolist() == [0, 1, 2]      # bestIdx2 as the loop left it
        assert r[0].n_matches == (2 if mode == bo.FRAME else 1)
    return build([k1, k2], [(0, 1)], prop, mode)


# ------------------------------------------------------------------------------------------------ the matched flag

def _steal_chain(mode):
    """a takes X; b's best was X too, so b gets its next candidate"""
    def prop(c, r):
        _row(r[0], 0, 0, 2, 20, bo.OK)
        _row(r[0], 1, 1, 17, 256, bo.OK)
    return build([[kp(L(0)), kp(L(3))], [kp(L(2)), kp(L(20))]], [(0, 1)], prop, mode)


def _matched_not_second(mode):
    """b (at 12) has Y at 10 and X at 11: 10 < 0.9 * 11 fails.  a took X before, so b's second is 256 and b passes."""
    def prop(c, r):
        _row(r[0], 0, 0, 1, 22, bo.OK)
        _row(r[0], 1, 1, 10, 256, bo.OK)
    return build([[kp(L(0)), kp(L(12))], [kp(L(1)), kp(L(22))]], [(0, 1)], prop, mode)


def _rot_removed_stays_matched(mode):
    """a takes X and is alone in its rotation bin, so the rotation pass removes it; X stays matched all the same (the
    pass runs after the loops): b, whose best was X, has Y.  Twelve more matches fill three larger bins."""
    k1, k2 = [kp(L(0), angle=180.0), kp(L(3), angle=0.0)], [kp(L(2)), kp(L(20))]
    for i, rot in enumerate([0.0] * 5 + [60.0] * 4 + [120.0] * 3):
        k1.append(kp(L(40 + i), node=1 + i, angle=rot))
        k2.append(kp(L(41 + i), node=1 + i))

    def prop(c, r):
        _row(r[0], 0, 0, 2, 20, bo.ROT)
        _row(r[0], 1, 1, 17, 256, bo.OK)
        assert (r[0].status[2:] == bo.OK).all() and r[0].n_matches == 13
    return build([k1, k2], [(0, 1)], prop, mode, check_orientation=1)


def _has_point2(mode):
    """the nearest candidate has no point: skipped by the keyframe overload, taken by the frame overload"""
    def prop(c, r):
        if mode == bo.KF:
            _row(r[0], 0, 1, 9, 256, bo.OK)
        else:
            _row(r[0], 0, 0, 2, 9, bo.OK)
        _row(r[0], 1, -1, 256, 256, bo.NO_POINT)
    return build([[kp(L(50)), kp(L(50), has_point=0)], [kp(L(52), has_point=0), kp(L(59))]], [(0, 1)], prop, mode)


def _all_equal(mode):
    """all descriptors of the node equal: (0, 0) every time, nobody matches, nothing gets matched"""
    def prop(c, r):
        for i in range(3):
            _row(r[0], i, 0, 0, 0, bo.RATIO)
    return build([[kp(L(77))] * 3, [kp(L(77))] * 3], [(0, 1)], prop, mode)


def _nodes_one_side(mode):
    """node 1 only in side 1, node 2 only in side 2, a keypoint in no node; node 3 in both"""
    k1 = [kp(L(10), node=1), kp(L(10), node=-1), kp(L(10), node=3), kp(L(10), node=1, has_point=0)]
    k2 = [kp(L(10), node=2), kp(L(11), node=3), kp(L(10), node=-1)]

    def prop(c, r):
        _status(r[0], bo.NO_NODE, bo.NO_NODE, bo.OK, bo.NO_NODE)
        _row(r[0], 2, 1, 1, 256, bo.OK)
    return build([k1, k2], [(0, 1)], prop, mode)


def _kf1_is_kf2(mode):
    """a keyframe against itself: every keypoint with a point finds itself at distance 0"""
    rng = np.random.default_rng(0xB4)
    k = [kp(far(rng), node=i % 3, has_point=int(i % 5 != 0)) for i in range(40)]

    def prop(c, r):
        has = np.array([x["has_point"] for x in k], bool)
        assert (r[0].idx2[has] == np.flatnonzero(has)).all() and (r[0].dist[has] == 0).all()
        assert (r[0].status[has] == bo.OK).all() and (r[0].status[~has] == bo.NO_POINT).all()
    return build([k], [(0, 0)], prop, mode)


def _ratio_float(nn_ratio, b1, b2):
    """nn_ratio * (float)b2 rounds to b1 in float, so b1 < it is false; the product in double accepts"""
    def make(mode):
        def prop(c, r):
            _row(r[0], 0, 0, b1, b2, bo.RATIO)
        return build([[kp(L(100))], [kp(L(100 + b1)), kp(L(100 - b2))]], [(0, 1)], prop, mode, nn_ratio=nn_ratio)
    return make


def _empty_side1(mode):
    def prop(c, r):
        assert len(r[0].status) == 0 and r[0].n_matches == 0 and r[1].n_matches == 1
    return build([[], [kp(L(5))], [kp(L(6))]], [(0, 1), (2, 1)], prop, mode)


# ------------------------------------------------------------------------------------------------ generated

GEN = dict(n_feat=300, n_nodes=12, cluster=4)
VARIANT_PAIRS = (6, 77)     # (n_pairs, seed) of the generated pairs on which the variants are counted
# ... and their knobs, tuned on the CPU (tests/test_bow_cases.py prints the counts): tight clusters and little bit noise
# keep (bestDist1, bestDist2) small, where ties and the 3 : 5 ratios that separate the float product from the double
# one are common
VARIANT_GEN = dict(cluster_bits=(1, 8), bits=(0, 8), cluster=5)


def generated(n_pairs, seed, mode, prm=None, **over):
    pairs, ekfs, feats, nid, nst, nf, _ = make_bow_pairs(n_pairs, seed=seed, **dict(GEN, **over))
    return Case(pairs, ekfs, feats, nid, nst, nf, dict(dict(mode=mode), **(prm or {})), None)


def _generated(n_pairs, seed, **over):
    def make(mode):
        def prop(c, r):
            for x in r:
                assert x.n_matches > 20 and (x.status == bo.RATIO).any() and (x.status == bo.ROT).any()
        return generated(n_pairs, seed, mode, **over)._replace(prop=prop)
    return make


CASES = {
    **{f"list2_{n}": _list2(n) for n in (0, 1, 2, 63, 64, 65, 128, 129, BOW_LDS_CAP - 1, BOW_LDS_CAP, BOW_LDS_CAP + 1,
                                         BOW_MAX_NODE)},
    "empty_list2": _empty_list2,
    "empty_side1": _empty_side1,
    "list1_1": _list1(1),
    "list1_65": _list1(65),
    "tie_position_not_lane": _tie_position_not_lane,
    "best_tied_with_second": _best_tied_with_second,
    "b1_zero": _b1_zero,
    "complement": _complement,
    "threshold_49_50_51": _threshold,
    "steal_chain": _steal_chain,
    "matched_not_second": _matched_not_second,
    "rot_removed_stays_matched": _rot_removed_stays_matched,
    "has_point2": _has_point2,
    "all_equal": _all_equal,
    "nodes_one_side": _nodes_one_side,
    "kf1_is_kf2": _kf1_is_kf2,
    "ratio_float_0.6_3_5": _ratio_float(0.6, 3, 5),
    "ratio_float_0.8_4_5": _ratio_float(0.8, 4, 5),
    "generated_3x300": _generated(3, 1),
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name, mode):
    c = CASES[name](mode)
    return c, [bo.sequential(j) for j in bo.jobs_of(c)]
