"""The split of ORBmatcher::Fuse is exact: device-free rows (the restatement on the uploaded snapshot), amc_lba.fuse's
fuse_walk on a ToyMap and `redo` from the restatement on the LIVE point leave the map IDENTICAL to fuse_sequential, the
whole Fuse run directly on a copy: every observation, occupant, bad flag, nObs, descriptor, n_fused and replace_out.
For LocalMapping::SearchInNeighbors' two phases over 20 targets and for LoopClosing::SearchAndFuse with its replace
loop, on generated maps and on the named map cases.  Without the redo rule this file fails
(test_without_the_redo_rule_the_map_differs shows it).

Cap, a condition on the generator and not a measurement: on every GENERATED problem the redone jobs are at most 10 % of
the rows with status OK or TOO_FAR.  The named map cases are exempt: they are built so that the redo matters.
scripts/fuse_margins.py writes the measured shares to profiles/fuse_margins.log."""
import numpy as np
import pytest

import fuse_cases as fc
import fuse_oracle as fo
from amc_lba.fuse import (FUSE_KF, FUSE_OK, FUSE_SIM3, FUSE_TOO_FAR, TH_KF, TH_SIM3, FuseProblem, fuse_walk,
                          make_fuse_problem, pack_searches, pack_targets, search_and_fuse_replaces)

CAP = 0.10


def snapshot(prob, m, ids):
    """the points array a caller uploads for the list `ids` at this moment: live descriptors, skip = isBad()"""
    bad = np.array([p.bad for p in m.pts], bool)
    desc = np.stack([p.desc for p in m.pts])
    return prob.points(ids, skip=bad, desc=desc)


class Tally:
    def __init__(self):
        self.redone = self.decided = self.in_kf_rows_used = 0


def batch_walk(prob, m, kfs, ids, mode, th, tally, redo_rule=True, replaces=False, rows_fn=None):
    """one device call's worth: the rows of every keyframe of `kfs` against the list from ONE snapshot, then the walk.
    rows_fn(targets, points, mode, th) -> rows per target: the device in tests/test_gpu_fuse.py, the restatement here.
    Returns (n_fused per search, replace_out per search)."""
    ids = np.asarray(ids, np.int64)
    targets = [prob.targets[k] for k in kfs]
    points = snapshot(prob, m, ids)
    rows = [fo.sequential(tg, points, mode, th)[0] for tg in targets] if rows_fn is None else rows_fn(targets, points, mode, th)
    S = pack_searches(pack_targets(targets).T, [(i, 0, len(ids), mode, th) for i in range(len(kfs))])
    was_in = {(s, int(pid), c) for s, k in enumerate(kfs) for pid in ids for c in range(targets[s].n_cam)
              if pid >= 0 and m.in_camera(int(pid), k, c)}
    tally.decided += sum(int(np.isin(r["status"], (FUSE_OK, FUSE_TOO_FAR)).sum()) for r in rows)
    n_fused, rep_out = [], []
    for s in range(len(kfs)):                 # search by search, so that SearchAndFuse's replaces can go in between
        if redo_rule:
            redo = lambda _s, i, c, s=s: fo.one_job(targets[s], c, fo.live_point(prob, m, int(ids[i])), mode, th)[0]
        else:
            redo = lambda _s, i, c, s=s: rows[s][i, c]
        used = _Spy(m, s, was_in)
        nf, rep, redone = fuse_walk(rows[s:s + 1], S[s:s + 1], ids, points["desc"], used, redo, kf_ids={s: kfs[s]})
        tally.redone += len(redone)
        tally.in_kf_rows_used += used.count
        n_fused.append(nf[0])
        rep_out.append(rep[0])
        if replaces:
            search_and_fuse_replaces(m, ids, rep[0])
    return n_fused, rep_out


class _Spy:
    """the map, counting the jobs the walk goes on to search although the UPLOADED map observed them: the rows an
    IsInKFCamera applied on the device would not have"""

    def __init__(self, m, s, was_in):
        self.m, self.s, self.was_in, self.count = m, s, was_in, 0

    def __getattr__(self, name):
        return getattr(self.m, name)

    def in_camera(self, pid, kf, c):
        live = self.m.in_camera(pid, kf, c)
        self.count += (not live) and (self.s, pid, c) in self.was_in
        return live


def batch_sequential(prob, m, kfs, ids, mode, th, replaces=False):
    n_fused, rep_out = [], []
    for k in kfs:
        nf, rep = fo.fuse_sequential(m, prob, k, prob.targets[k], ids, mode, th)
        n_fused.append(nf)
        rep_out.append(rep)
        if replaces:
            search_and_fuse_replaces(m, ids, rep)
    return n_fused, rep_out


def fuse_candidates(m, kfs):
    """SearchInNeighbors :655-674: the targets' points, each once, in order"""
    seen, out = set(), []
    for k in kfs:
        for pid in m.mp[k]:
            pid = int(pid)
            if pid < 0 or m.is_bad(pid) or pid in seen:
                continue
            seen.add(pid)
            out.append(pid)
    return out


def same(a, b):
    return a.state() == b.state()


def search_in_neighbors(prob, cur, kfs, tally, redo_rule=True, rows_fn=None):
    """both phases on two maps; returns (walked map, sequential map)"""
    mw = fo.ToyMap.from_problem(prob)
    ms = mw.copy()
    lst = mw.mp[cur].copy()                                   # vpMapPointMatches, NULLs included
    a = batch_walk(prob, mw, kfs, lst, FUSE_KF, TH_KF, tally, redo_rule, rows_fn=rows_fn)
    b = batch_sequential(prob, ms, kfs, lst, FUSE_KF, TH_KF)
    assert not redo_rule or (a[0] == b[0] and same(mw, ms)), "phase one"
    cw, cs = fuse_candidates(mw, kfs), fuse_candidates(ms, kfs)
    assert not redo_rule or cw == cs
    a = batch_walk(prob, mw, [cur], cw, FUSE_KF, TH_KF, tally, redo_rule, rows_fn=rows_fn)
    b = batch_sequential(prob, ms, [cur], cs, FUSE_KF, TH_KF)
    assert not redo_rule or (a[0] == b[0] and same(mw, ms)), "phase two"
    return mw, ms


def search_and_fuse(prob, kfs, lst, tally, redo_rule=True, rows_fn=None):
    mw = fo.ToyMap.from_problem(prob)
    ms = mw.copy()
    a = batch_walk(prob, mw, kfs, lst, FUSE_SIM3, TH_SIM3, tally, redo_rule, replaces=True, rows_fn=rows_fn)
    b = batch_sequential(prob, ms, kfs, lst, FUSE_SIM3, TH_SIM3, replaces=True)
    if redo_rule:
        assert a[0] == b[0] and all((x == y).all() for x, y in zip(a[1], b[1])) and same(mw, ms)
    return mw, ms


@pytest.mark.parametrize("seed", (0, 1))
def test_search_in_neighbors_over_20_targets(seed):
    prob = make_fuse_problem(n_kf=21, n_cam=4, n_feat=100, n_points=220, seed=seed)
    tally = Tally()
    search_in_neighbors(prob, 0, list(range(1, 21)), tally)
    share = tally.redone / max(1, tally.decided)
    print("seed %d: %d redone of %d OK / TOO_FAR rows (%.2f %%); %d used rows an up-front IsInKFCamera would drop"
          % (seed, tally.redone, tally.decided, 100 * share, tally.in_kf_rows_used))
    assert tally.decided > 500 and share <= CAP


def loop_list(prob, m, kfs):
    """the loop side's points (mvpLoopMapPoints): those of the given keyframes, each once"""
    return fuse_candidates(m, kfs)


@pytest.mark.parametrize("seed", (0, 1))
def test_search_and_fuse_with_its_replace_loop(seed):
    prob = make_fuse_problem(n_kf=12, n_cam=4, n_feat=100, n_points=220, seed=100 + seed, duplicates=0.08)
    lst = loop_list(prob, fo.ToyMap.from_problem(prob), [0, 1, 2])
    tally = Tally()
    search_and_fuse(prob, list(range(3, 12)), lst, tally)
    share = tally.redone / max(1, tally.decided)
    print("seed %d: %d redone of %d OK / TOO_FAR rows (%.2f %%)" % (seed, tally.redone, tally.decided, 100 * share))
    assert tally.decided > 500 and share <= CAP


# ---------------------------------------------------------------- the named map cases (exempt from the cap)
def mini(feats_per_kf, pts, obs, bad=()):
    """identity-pose keyframes of two cameras (tests/fuse_cases.py); pts: (u, v, desc) at level 2"""
    targets = [fc.target(2, f) for f in feats_per_kf]
    P = fc.cat([fc.point(u, v, 2, d) for u, v, d in pts])
    b = np.zeros(len(pts), bool)
    b[list(bad)] = True
    return FuseProblem(targets, P["pos"].copy(), P["normal"].copy(), P["max_distance"].copy(), P["desc"].copy(), b,
                       np.array(obs, np.int64).reshape(-1, 3), None, fc.N_LEVELS, fc.SCALE)


def case_wins_and_is_seen_again():
    """A (two observations in keyframes 3 and 4) meets B (one) on feature 0 of (keyframe 1, camera 0): B.Replace(A), and
    ComputeDistinctiveDescriptors moves A's descriptor some 60 bits away.  The feature A would have taken in camera 1 and
    the one in keyframe 2 are 20 bits from the UPLOADED descriptor and beyond TH_LOW from the live one."""
    d = fc.D(1)
    e = fc.near(d, 60, 1)
    g1, g2 = fc.near(e, 3, 1), fc.near(e, 3, 2)
    kf0 = []
    kf1 = [fc.feat(0, 100.5, 100.0, 2, fc.near(d, 10, 3)), fc.feat(1, 100.5, 100.0, 2, fc.near(d, 20, 4))]
    kf2 = [fc.feat(0, 100.5, 100.0, 2, fc.near(d, 20, 5))]
    kf3, kf4 = [fc.feat(0, 300.0, 300.0, 2, g1)], [fc.feat(0, 300.0, 300.0, 2, g2)]
    prob = mini([kf0, kf1, kf2, kf3, kf4], [(100.0, 100.0, d), (100.0, 100.25, fc.near(d, 12, 6))],
                [(0, 3, 0), (0, 4, 0), (1, 1, 0)])
    return prob, [1, 2], [0]


def case_loses_and_goes_on():
    """A (one observation: camera 1 of keyframe 1) meets B (three) in camera 0: A.Replace(B) clears A's observations, so
    the reference goes on to search camera 1, which IsInKFCamera would have skipped at upload time"""
    d = fc.D(2)
    kf1 = [fc.feat(0, 100.5, 100.0, 2, fc.near(d, 5, 1)), fc.feat(1, 100.5, 100.0, 2, fc.near(d, 9, 2)),
           fc.feat(1, 99.5, 100.0, 2, fc.near(d, 4, 3))]
    kf2, kf3 = [fc.feat(0, 300.0, 300.0, 2, fc.near(d, 6, 4))], [fc.feat(0, 300.0, 300.0, 2, fc.near(d, 7, 5))]
    prob = mini([[], kf1, kf2, kf3], [(100.0, 100.0, d), (100.0, 100.25, fc.near(d, 3, 6))],
                [(0, 1, 1), (1, 1, 0), (1, 2, 0), (1, 3, 0)])
    return prob, [1], [0]


def case_later_element_made_bad():
    """the list is [A, B]; A (two observations) takes B's (one) feature: B is bad when its turn comes, though its
    uploaded skip is 0 and its row is OK"""
    d = fc.D(3)
    kf1 = [fc.feat(0, 100.5, 100.0, 2, fc.near(d, 5, 1)), fc.feat(0, 400.5, 100.0, 2, fc.near(d, 6, 2))]
    kf2, kf3 = [fc.feat(0, 300.0, 300.0, 2, fc.near(d, 6, 4))], [fc.feat(0, 300.0, 300.0, 2, fc.near(d, 7, 5))]
    prob = mini([[], kf1, kf2, kf3], [(100.0, 100.0, d), (400.0, 100.0, d)], [(0, 2, 0), (0, 3, 0), (1, 1, 0)])
    return prob, [1], [0, 1]


def case_bad_occupant():
    """the feature's occupant is a bad point: nFused counts it, nothing is replaced or added"""
    d = fc.D(4)
    kf1 = [fc.feat(0, 100.5, 100.0, 2, fc.near(d, 5, 1))]
    prob = mini([[], kf1], [(100.0, 100.0, d), (100.0, 100.25, d)], [(1, 1, 0)], bad=[1])
    return prob, [1], [0]


def case_two_points_one_feature():
    """A and C both project onto one free feature: A adds it, C then meets A as its occupant"""
    d = fc.D(5)
    kf1 = [fc.feat(0, 100.5, 100.0, 2, fc.near(d, 5, 1))]
    kf2 = [fc.feat(0, 300.0, 300.0, 2, fc.near(d, 6, 4)), fc.feat(1, 300.0, 300.0, 2, fc.near(d, 8, 4))]
    prob = mini([[], kf1, kf2], [(100.0, 100.0, d), (100.25, 100.0, fc.near(d, 2, 7))], [(1, 2, 0), (1, 2, 1)])
    return prob, [1], [0, 1, -1, 0]


KF_CASES = dict(wins_and_is_seen_again=case_wins_and_is_seen_again, loses_and_goes_on=case_loses_and_goes_on,
                later_element_made_bad=case_later_element_made_bad, bad_occupant=case_bad_occupant,
                two_points_one_feature=case_two_points_one_feature)


def run_kf_case(name, redo_rule=True):
    prob, kfs, lst = KF_CASES[name]()
    mw = fo.ToyMap.from_problem(prob)
    ms = mw.copy()
    tally = Tally()
    a = batch_walk(prob, mw, kfs, lst, FUSE_KF, TH_KF, tally, redo_rule)
    b = batch_sequential(prob, ms, kfs, lst, FUSE_KF, TH_KF)
    return mw, ms, a, b, tally


@pytest.mark.parametrize("name", list(KF_CASES))
def test_named_map_case(name):
    mw, ms, a, b, tally = run_kf_case(name)
    assert a[0] == b[0] and same(mw, ms)
    if name == "wins_and_is_seen_again":
        assert mw.pts[1].bad and mw.pts[0].obs == {1: [0, -1], 3: [0, -1], 4: [0, -1]} and tally.redone == 2
    if name == "loses_and_goes_on":
        assert mw.pts[0].bad and tally.in_kf_rows_used == 1 and 1 in mw.pts[0].obs      # searched, and added again
    if name == "later_element_made_bad":
        assert mw.pts[1].bad and a[0] == [1] and mw.mp[1].tolist() == [0, -1]
    if name == "bad_occupant":
        assert a[0] == [1] and mw.mp[1].tolist() == [1] and not mw.pts[0].obs
    if name == "two_points_one_feature":
        assert a[0] == [2] and mw.pts[0].bad and mw.mp[1].tolist() == [1]


def case_found_through_replaces():
    """SearchAndFuse: the loop point L meets R on keyframe 1; R also holds a feature of keyframe 2.  After keyframe 1's
    replace loop L has R's observations, so keyframe 2's spAlreadyFound holds L and its (OK) rows are not used."""
    d = fc.D(6)
    kf1 = [fc.feat(0, 100.5, 100.0, 2, fc.near(d, 5, 1)), fc.feat(1, 0.0, 0.0, 2, fc.D(99))]
    kf2 = [fc.feat(0, 100.5, 100.0, 2, fc.near(d, 6, 2)), fc.feat(0, 99.5, 100.0, 2, fc.near(d, 4, 3)),
           fc.feat(1, 0.0, 0.0, 2, fc.D(98))]
    kf3 = [fc.feat(0, 300.0, 300.0, 2, fc.near(d, 6, 4))]
    prob = mini([[], kf1, kf2, kf3], [(100.0, 100.0, d), (100.0, 100.25, fc.near(d, 3, 6))],
                [(0, 3, 0), (1, 1, 0), (1, 2, 0)])
    return prob, [1, 2], [0]


def test_loop_point_becomes_already_found_through_the_replaces():
    prob, kfs, lst = case_found_through_replaces()
    mw, ms = search_and_fuse(prob, kfs, lst, Tally())
    assert mw.pts[1].bad and mw.mp[2].tolist() == [0, -1, -1]       # L holds R's feature; the closer one stays free


def test_without_the_redo_rule_the_map_differs():
    mw, ms, a, b, _ = run_kf_case("wins_and_is_seen_again", redo_rule=False)
    assert not same(mw, ms)
    differs = 0
    for seed in (0, 1):
        prob = make_fuse_problem(n_kf=21, n_cam=4, n_feat=100, n_points=220, seed=seed)
        mw, ms = search_in_neighbors(prob, 0, list(range(1, 21)), Tally(), redo_rule=False)
        differs += not same(mw, ms)
    print("generated maps that differ without the redo rule: %d of 2" % differs)
