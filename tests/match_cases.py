"""The named cases of lba_match_project (tests/test_match_cases.py on the CPU, tests/test_match_host.py against the
host-built header, tests/test_gpu_match.py on the GPU).

A case is the smallest shape at which its hazard exists and has a property its `check` asserts on the sequential
restatement (tests/match_oracle.py).  `case(name, mode)` returns (Search, params, sequential result, round-based
result, check, candidate lists), computed once.  The image is 640 x 480 with the grid's 64 x 48 cells of 10 x 10
pixels, so every float expression of a hand-made case is exact unless the case says otherwise.
"""
import functools

import numpy as np

import match_oracle as mo
from amc_lba.abi import MATCH_FEAT_DTYPE, MATCH_JOB_DTYPE
from amc_lba.match import (MATCH_BEST, MATCH_MAX_FEAT, MATCH_NO_CAND, MATCH_OK, MATCH_RATIO, MATCH_RATIO_FAIL,
                           MATCH_ROT, MATCH_TOO_FAR, Search, build_grid, make_match_search, match_cams, match_params)

BOTH = (MATCH_RATIO, MATCH_BEST)
MODE_NAME = {MATCH_RATIO: "ratio", MATCH_BEST: "best"}


def D(n):
    """a descriptor with the n lowest bits set: D(a) and D(b) are |a - b| apart"""
    v = (1 << n) - 1
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)], np.uint32)


def feat(x, y, dist=0, octave=0, cam=0, taken=0, u_right=-1.0, angle=0.0):
    return dict(x=x, y=y, desc=D(dist), octave=octave, cam=cam, taken=taken, u_right=u_right, angle=angle)


def job(x, y, radius, cam=0, lo=-1, hi=-1, blocks=1, ur=0.0, angle=0.0, dist=0):
    return dict(x=x, y=y, radius=radius, cam=cam, min_level=lo, max_level=hi, blocks=blocks, ur=ur, angle=angle, desc=D(dist))


def search(feats, jobs, n_cam=1):
    f = np.zeros(len(feats), MATCH_FEAT_DTYPE)
    j = np.zeros(len(jobs), MATCH_JOB_DTYPE)
    for arr, rows in ((f, feats), (j, jobs)):
        for i, r in enumerate(rows):
            for k, v in r.items():
                arr[i][k] = v
    j["point"] = 1000 + np.arange(len(j))
    cams = match_cams(n_cam)
    cs, cf = build_grid(f, cams)
    return Search(cams, cs, cf, f, j)


def prm(mode, n_cam=1, **kw):
    kw.setdefault("stereo_cam", -1)
    kw.setdefault("check_orientation", 0)
    return match_params(mode, n_cam, **kw)


# ---- the builders: mode -> (Search, params, check(search, sequential, by_rounds, candidates))
def _empty(mode):
    def check(s, r, rr, cands):
        assert r.n_matches == 0 and len(r.status) == 0 and rr.rounds.tolist() == [0]
    return search([], []), prm(mode), check


def _n_cand(n):
    def build(mode):
        # one cell's worth of features around (105, 105); the best is the first, later ones tie with it in pairs
        # (one column of the grid, so the wave walks ONE span of n slots)
        fs = [feat(104.0 + (i % 5) * 0.2, 104.0 + (i // 5) * 0.125, dist=10 + (i // 2) % 60) for i in range(n)]

        def check(s, r, rr, cands):
            assert len(cands[0]) == n and mo.capacity(s, 0) >= n
            assert r.status[0] == (MATCH_OK if n else MATCH_NO_CAND)
            if n:
                assert r.best_dist[0] == 10 and r.feat[0] == next(f for f, d, _ in cands[0] if d == 10)
            if n > 1 and mode == MATCH_RATIO:
                assert r.best_dist2[0] == 10          # the tie partner: equal levels, accepted only as nn_ratio is 1
        return search(fs, [job(105.0, 105.0, 3.0)]), prm(mode, nn_ratio=1.0), check
    return build


def _two_jobs(blocks):
    def build(mode):
        fs = [feat(105.0, 105.0, dist=5), feat(106.0, 105.0, dist=40, octave=1)]
        js = [job(105.0, 105.0, 3.0, blocks=blocks), job(105.5, 105.0, 3.0, blocks=1)]

        def check(s, r, rr, cands):
            assert r.status.tolist() == [MATCH_OK, MATCH_OK] and r.n_matches == 2
            assert r.feat.tolist() == ([0, 1] if blocks else [0, 0])
            assert r.job.tolist() == ([0, 1] if blocks else [1, -1])
            assert rr.rounds.tolist() == [2]
        return search(fs, js), prm(mode), check
    return build


def _taken(mode):
    fs = [feat(105.0, 105.0, dist=5, taken=1), feat(106.0, 105.0, dist=40), feat(305.0, 105.0, dist=5, taken=1)]
    js = [job(105.0, 105.0, 3.0), job(305.0, 105.0, 3.0)]

    def check(s, r, rr, cands):
        assert r.feat.tolist() == [1, -1] and r.status.tolist() == [MATCH_OK, MATCH_NO_CAND]
        assert len(cands[1]) == 1 and r.job.tolist() == [-1, 0, -1]
    return search(fs, js), prm(mode), check


def _chain(mode):
    # job k sees features k and k + 1 only: every job waits for the one before it
    fs = [feat(20.0 + 2.0 * k, 100.0, dist=(7 * k) % 50) for k in range(257)]
    js = [job(21.0 + 2.0 * k, 100.0, 1.5, blocks=k % 3 != 0) for k in range(256)]

    def check(s, r, rr, cands):
        assert all([f for f, _, _ in cands[k]] == [k, k + 1] for k in range(256))
        assert rr.rounds.tolist() == [256]
    return search(fs, js), prm(mode), check


def _disjoint(mode):
    fs = [feat(25.0 + 30.0 * (k % 16), 15.0 + 30.0 * (k // 16), dist=k % 50) for k in range(256)]
    js = [job(25.0 + 30.0 * (k % 16), 15.0 + 30.0 * (k // 16), 3.0) for k in range(256)]

    def check(s, r, rr, cands):
        assert rr.rounds.tolist() == [1] and r.feat.tolist() == list(range(256))
    return search(fs, js), prm(mode), check


def _ties(mode):
    # across two cells: feature 0 lies in the LATER cell (ix 11), feature 1 in the earlier one (ix 10): 1 wins.
    # within one cell: features 2 and 3, the first inserted wins.
    fs = [feat(106.0, 105.0, dist=9), feat(104.0, 105.0, dist=9), feat(304.0, 105.0, dist=9), feat(304.25, 105.0, dist=9)]
    js = [job(105.0, 105.0, 3.0), job(304.0, 105.0, 3.0)]

    def check(s, r, rr, cands):
        assert [f for f, _, _ in cands[0]] == [1, 0] and [f for f, _, _ in cands[1]] == [2, 3]
        if mode == MATCH_BEST:
            assert r.feat.tolist() == [1, 2]
        else:            # equal levels and 9 > 0.8 * 9: the ratio rule drops both
            assert r.status.tolist() == [MATCH_RATIO_FAIL] * 2 and r.best_dist2.tolist() == [9, 9]
    return search(fs, js), prm(mode), check


def _ratio(mode):
    # nn_ratio 0.5 and bestDist2 80: the product is 40 exactly.  best 39 / 40 / 41 with equal and unequal levels
    fs, js = [], []
    for g, (best, lvl2) in enumerate([(39, 0), (40, 0), (41, 0), (39, 1), (40, 1), (41, 1)]):
        x = 55.0 + 50.0 * g
        fs += [feat(x, 105.0, dist=best), feat(x + 1.0, 105.0, dist=80, octave=lvl2)]
        js.append(job(x, 105.0, 3.0))
    fs.append(feat(55.0, 305.0, dist=99))      # a single candidate: bestLevel2 stays -1
    js.append(job(55.0, 305.0, 3.0))

    def check(s, r, rr, cands):
        F_ = MATCH_RATIO_FAIL
        assert r.status.tolist() == [MATCH_OK, MATCH_OK, F_, MATCH_OK, MATCH_OK, MATCH_OK, MATCH_OK]
        assert r.best_dist2.tolist() == [80] * 6 + [256]
    return search(fs, js), prm(mode, nn_ratio=0.5), check


def _th_high(mode):
    fs = [feat(105.0, 105.0, dist=100), feat(305.0, 105.0, dist=101)]
    js = [job(105.0, 105.0, 3.0), job(305.0, 105.0, 3.0)]

    def check(s, r, rr, cands):
        assert r.status.tolist() == [MATCH_OK, MATCH_TOO_FAR] and r.best_dist.tolist() == [100, 101]
    return search(fs, js), prm(mode), check


def _edges(mode):
    fs = [feat(1.0, 240.0), feat(634.0, 240.0), feat(320.0, 1.0), feat(320.0, 474.0)]
    js = [job(2.0, 240.0, 5.0), job(636.0, 240.0, 5.0), job(320.0, 2.0, 5.0), job(320.0, 476.0, 5.0),   # clipped
          job(-20.0, 240.0, 5.0), job(660.0, 240.0, 5.0), job(320.0, -20.0, 5.0), job(320.0, 500.0, 5.0)]   # outside

    def check(s, r, rr, cands):
        assert r.feat.tolist() == [0, 1, 2, 3, -1, -1, -1, -1]
        assert r.status[4:].tolist() == [MATCH_NO_CAND] * 4
        rects = [mo.cell_rect(j["x"], j["y"], j["radius"], s.cams[0]) for j in s.jobs]
        assert rects[0][0] == 0 and rects[1][1] == 63 and rects[2][2] == 0 and rects[3][3] == 47
        assert rects[4:] == [None] * 4
    return search(fs, js), prm(mode), check


def _ceil_cell(mode):
    # the window ends at x = 106: floor gives cell 10, ceil cell 11, and PosInGrid's round puts 105.5 into cell 11
    def check(s, r, rr, cands):
        assert mo.cell_rect(103.0, 105.0, 3.0, s.cams[0])[:2] == (10, 11)
        assert int(np.floor(np.float32(106.0) * s.cams[0]["grid_w_inv"])) == 10
        assert s.cell_start[12 * 48] - s.cell_start[11 * 48] == 1 and r.feat.tolist() == [0]
    return search([feat(105.5, 105.0)], [job(103.0, 105.0, 3.0)]), prm(mode), check


def _levels(mode):
    fs = [feat(104.0 + 0.5 * o, 105.0, dist=10 + o, octave=o) for o in range(4)]
    ranges = [(0, -1), (-1, -1), (2, -1), (1, 2), (3, 3), (4, -1), (0, 0)]
    js = [job(105.0, 105.0, 3.0, lo=lo, hi=hi, blocks=0) for lo, hi in ranges]

    def check(s, r, rr, cands):
        assert [[o for _, _, o in c] for c in cands] == [[0, 1, 2, 3], [0, 1, 2, 3], [2, 3], [1, 2], [3], [], [0]]
    return search(fs, js, n_cam=1), prm(mode), check


def _stereo(truncate):
    def build(mode):
        fs, js = [], []
        # (u_right, ur) per group, radius 5, on the stereo camera 1; the last group on camera 0
        groups = [(-1.0, 100.0, 1), (0.6, 100.0, 1), (50.0, 55.0, 1), (50.0, 55.5, 1), (50.9, 45.5, 1), (50.0, 100.0, 0)]
        for g, (u, ur, cam) in enumerate(groups):
            fs.append(feat(55.0 + 50.0 * g, 105.0, cam=cam, u_right=u))
            js.append(job(55.0 + 50.0 * g, 105.0, 5.0, cam=cam, ur=ur))
        want = [1, int(truncate), 1, 0, int(truncate), 1]

        def check(s, r, rr, cands):
            assert [len(c) for c in cands] == want
            assert r.status.tolist() == [MATCH_OK if w else MATCH_NO_CAND for w in want]
        return search(fs, js, n_cam=2), prm(mode, 2, stereo_cam=1, ur_truncate=int(truncate)), check
    return build


def _not_finite(mode):
    bad = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    fs = [feat(105.0, 105.0)]
    js = [job(v, 105.0, 3.0) for v in bad] + [job(105.0, v, 3.0) for v in bad] + [job(105.0, 105.0, v) for v in bad[:4]]
    js.append(job(105.0, 105.0, 3.0))

    def check(s, r, rr, cands):
        assert r.status[:-1].tolist() == [MATCH_NO_CAND] * 14 and r.status[-1] == MATCH_OK
    return search(fs, js), prm(mode), check


def _rot(sizes, extra=()):
    """bins 1, 2, 3, ... with `sizes` jobs each (rot = 30 bin), every job with a feature of its own"""
    def build(mode):
        fs, js, k = [], [], 0
        rots = [30.0 * (b + 1) for b, n in enumerate(sizes) for _ in range(n)] + list(extra)
        for rot in rots:
            x, y = 15.0 + 20.0 * (k % 30), 15.0 + 20.0 * (k // 30)
            fs.append(feat(x, y, angle=10.0))
            js.append(job(x, y, 3.0, angle=10.0 + rot))
            k += 1

        def check(s, r, rr, cands):
            bins = [mo.rot_bin(j["angle"], 10.0) for j in s.jobs]
            keep = mo.three_maxima(np.bincount(bins, minlength=30))
            assert (r.status == np.where(np.isin(bins, keep), MATCH_OK, MATCH_ROT)).all()
            assert (r.status == MATCH_ROT).any() and r.n_matches == (r.status == MATCH_OK).sum()
            assert (r.job[r.feat[r.status == MATCH_ROT]] == -1).all()
            check.bins, check.keep = bins, keep
        return search(fs, js), prm(mode, check_orientation=1), check
    return build


def _limit(mode):
    # LBA_MATCH_MAX_FEAT features in ONE camera (a 128 x 64 lattice), the last of them wanted by two jobs
    n = MATCH_MAX_FEAT
    f = np.zeros(n, MATCH_FEAT_DTYPE)
    f["x"], f["y"] = 2.5 + 4.9 * (np.arange(n) % 128), 3.5 + 7.0 * (np.arange(n) // 128)
    f["desc"][:, 0] = 0xFFFF
    f["desc"][n - 1] = D(3)
    s = search([], [job(f["x"][n - 1], f["y"][n - 1], 3.0), job(f["x"][n - 1], f["y"][n - 1], 9.0), job(2.5, 3.5, 3.0)])
    cams = match_cams(1)
    cs, cf = build_grid(f, cams)

    def check(s, r, rr, cands):
        assert r.feat[0] == n - 1 and r.feat[1] not in (-1, n - 1) and r.feat[2] == 0 and rr.rounds.tolist() == [2]
    return Search(cams, cs, cf, f, s.jobs), prm(mode, nn_ratio=1.0), check


def over_limit():
    """one feature more than the resolve kernel's LDS holds: refused with LBA_E_LIMIT"""
    s = _limit(MATCH_BEST)[0]
    f = np.concatenate([s.feats, s.feats[:1]])
    cs, cf = build_grid(f, s.cams)
    return Search(s.cams, cs, cf, f, s.jobs)


def _generated(**kw):
    def build(mode):
        s = make_match_search(mode=mode, **kw)

        def check(s, r, rr, cands):
            st = np.bincount(r.status, minlength=5)
            assert st[MATCH_OK] > 0.2 * len(s.jobs) and st[MATCH_TOO_FAR] > 0 and st[MATCH_NO_CAND] > 0
            assert st[MATCH_RATIO_FAIL if mode == MATCH_RATIO else MATCH_ROT] > 0
        return s, match_params(mode, s.n_cam), check
    return build


BUILDERS = {
    "empty": (_empty, BOTH),
    "cand_0": (_n_cand(0), BOTH), "cand_1": (_n_cand(1), BOTH), "cand_63": (_n_cand(63), BOTH),
    "cand_64": (_n_cand(64), BOTH), "cand_65": (_n_cand(65), BOTH),
    "same_feature_blocks": (_two_jobs(1), BOTH), "same_feature_overwrite": (_two_jobs(0), BOTH),
    "taken_on_entry": (_taken, BOTH),
    "chain_256": (_chain, BOTH), "disjoint_256": (_disjoint, BOTH),
    "ties": (_ties, BOTH),
    "ratio_rule": (_ratio, (MATCH_RATIO,)),
    "th_high": (_th_high, BOTH),
    "grid_edges": (_edges, BOTH),
    "ceil_cell": (_ceil_cell, BOTH),
    "levels": (_levels, BOTH),
    "stereo_float": (_stereo(False), BOTH), "stereo_truncate": (_stereo(True), BOTH),
    "not_finite": (_not_finite, BOTH),
    # two surviving bins, the 0.1f rule AT equality (2 < 0.1f * 20 is false: kept) and below it (1: dropped)
    "rot_two_bins": (_rot([20, 2, 1]), (MATCH_BEST,)),
    "rot_three_bins": (_rot([10, 5, 3, 2]), (MATCH_BEST,)),
    # rot exactly 0 and 899.9 (bin 30 -> 0; with factor 1 / 30 a rot below 360 ends in bin 12 at most) share bin 0
    "rot_bin_wrap": (_rot([3, 2], extra=[0.0, 0.0, 899.9, 899.9, 359.9, 90.0]), (MATCH_BEST,)),
    "lds_limit": (_limit, BOTH),
    "generated": (_generated(n_cam=4, n_feat=400, n_points=600, seed=1), BOTH),
}
NAMES = [(n, m) for n, (_, modes) in BUILDERS.items() for m in modes]
IDS = [f"{n}-{MODE_NAME[m]}" for n, m in NAMES]


@functools.lru_cache(maxsize=None)
def case(name, mode):
    s, p, check = BUILDERS[name][0](mode)
    cands = mo.candidates(s, p)
    return s, p, mo.sequential(s, p, cands), mo.by_rounds(s, p, cands), check, cands


BATCH_SIZES = [(1 + k % 4, 40 + 23 * (k % 7), 30 + 41 * (k % 5)) for k in range(40)]   # n_cam, n_feat, n_points


@functools.lru_cache(maxsize=None)
def batch(mode):
    """40 generated searches of different sizes (1 .. 4 cameras), one of them without jobs"""
    out = [make_match_search(mode=mode, n_cam=c, n_feat=f, n_points=p, seed=100 + k) for k, (c, f, p) in enumerate(BATCH_SIZES)]
    out[7] = Search(out[7].cams, out[7].cell_start, out[7].cell_feat, out[7].feats, out[7].jobs[:0])
    return out


@functools.lru_cache(maxsize=None)
def small_batch(mode, n=300):
    """300 small searches: more (search, camera) workgroups than an MI355X has CUs"""
    return [make_match_search(mode=mode, n_cam=1 + k % 3, n_feat=30 + k % 11, n_points=25 + k % 13, seed=500 + k)
            for k in range(n)]
