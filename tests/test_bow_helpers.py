"""The caller's side of lba_match_bow on plain arrays (amc_lba.bow): bow_merge against a direct restatement of
LoopClosing.cc:499-516 on hand-made inputs (a shared point, a bad point, an empty pair, a skipped keyframe), the frame
overload's scatter, bow_pairs, and the chain bow_merge -> sim3_ransac_rows.  No GPU."""
import numpy as np

import bow_cases as bc
import bow_oracle as bo
from amc_lba.abi import BOW_ROW_DTYPE
from amc_lba.bow import (BOW_NO_CAND, BOW_NO_POINT, BOW_OK, BOW_RATIO, BOW_ROT, bow_matches, bow_merge, bow_pairs,
                         frame_matches, make_bow_pairs)
from amc_lba.sim3_ransac import sim3_ransac_rows


def rows_of(status, idx2):
    r = np.zeros(len(status), BOW_ROW_DTYPE)
    r["status"], r["idx2"], r["dist"], r["dist2"] = status, idx2, 9, 99
    return r


def merge_direct(vvp_matched, bad, n1):
    """LoopClosing.cc:499-516 with vvpMatchedMPs[j][k] as a point id or None"""
    seen, num = set(), 0
    points, kfs = [None] * n1, [None] * n1
    for j in range(len(vvp_matched)):
        for k in range(len(vvp_matched[j])):
            mp = vvp_matched[j][k]
            if mp is None or mp in bad:
                continue
            if mp not in seen:
                seen.add(mp)
                num += 1
                points[k] = mp
                kfs[k] = j
    return points, kfs, num


def test_bow_merge_on_hand_made_inputs():
    # three covisible keyframes and one the reference skipped (bad, :487: its vector stays empty)
    ids = [np.array([100, 101, 102, -1]), np.array([101, 200, 201]), np.array([300]), np.array([400, 401])]
    rows = [rows_of([BOW_OK, BOW_OK, BOW_NO_POINT, BOW_RATIO, BOW_OK], [0, 1, -1, 2, 2]),      # k0->100, k1->101, k4->102
            rows_of([BOW_OK, BOW_OK, BOW_OK, BOW_ROT, BOW_NO_CAND], [1, 0, 2, 1, 0]),           # k0->200, k1->101 (seen), k2->201 (bad)
            None,
            rows_of([BOW_NO_CAND] * 5, [-1] * 5)]                                               # an empty pair
    bad = {201}
    point, pair, n = bow_merge(rows, ids, bad)
    vvp = [[100, 101, None, None, 102], [200, 101, 201, None, None], [], [None] * 5]
    want_p, want_k, want_n = merge_direct(vvp, bad, 5)
    assert n == want_n == 4
    assert point.tolist() == [-1 if p is None else p for p in want_p] == [200, 101, -1, -1, 102]      # k0 overwritten by pair 1
    assert pair.tolist() == [-1 if k is None else k for k in want_k] == [1, 0, -1, -1, 0]
    # a matched keypoint of side 2 without a point id (the frame overload has those) brings nothing
    point, pair, n = bow_merge([rows_of([BOW_OK], [3])], [ids[0]])
    assert (point.tolist(), pair.tolist(), n) == ([-1], [-1], 0)
    assert bow_merge([], []) [2] == 0


def test_bow_merge_on_generated_pairs():
    for mode in bc.MODES:
        pairs, ekfs, feats, nid, nst, nf, truth = make_bow_pairs(5, n_feat=120, n_nodes=6, seed=3)
        c = bc.Case(pairs, ekfs, feats, nid, nst, nf, dict(mode=mode), None)
        res = [bo.sequential(j) for j in bo.jobs_of(c)]
        rows, vvp = [], []
        bad = set(int(i) for i in truth["point_id"][0][::7] if i >= 0)
        for p, r in enumerate(res):
            rr = rows_of(r.status, r.idx2)
            rows.append(rr)
            pid = truth["point_id"][p + 1]
            vvp.append([int(pid[r.idx2[k]]) if r.status[k] == bo.OK and pid[r.idx2[k]] >= 0 else None for k in range(len(rr))])
        point, pair, n = bow_merge(rows, truth["point_id"][1:], bad)
        want_p, want_k, want_n = merge_direct(vvp, bad, 120)
        assert n == want_n > 50 and len(set(point[point >= 0].tolist())) <= n
        assert point.tolist() == [-1 if x is None else x for x in want_p]
        assert pair.tolist() == [-1 if x is None else x for x in want_k]
        assert len(np.unique(pair[pair >= 0])) > 1          # the points come from several keyframes


def test_frame_matches_scatters_by_idx2():
    rows = rows_of([BOW_OK, BOW_NO_POINT, BOW_OK, BOW_ROT, BOW_RATIO, BOW_OK], [4, -1, 0, 2, 3, 5])
    pair = bow_pairs(0, [1], np.array([(0, 6, 0, 0, 0, 0), (6, 7, 0, 0, 0, 0)], bc.EPI_KF_DTYPE))[0]
    assert bow_matches(pair, rows).tolist() == [[0, 4], [2, 0], [5, 5]]
    assert frame_matches(pair, rows, 7).tolist() == [2, -1, -1, -1, 0, 5, -1]
    out = np.concatenate([rows_of([BOW_NO_CAND] * 3, [-1] * 3), rows])
    pair["out0"] = 3
    ekfs = np.array([(0, 6, 0, 0, 0, 0), (6, 7, 0, 0, 0, 0)], bc.EPI_KF_DTYPE)
    assert frame_matches(pair, out, 7, ekfs).tolist() == [2, -1, -1, -1, 0, 5, -1]


def test_bow_pairs_lays_the_out_ranges_one_behind_the_other():
    ekfs = np.zeros(4, bc.EPI_KF_DTYPE)
    ekfs["n_feat"] = (10, 20, 30, 40)
    p = bow_pairs(2, [0, 1, 3], ekfs)
    assert p["kf1"].tolist() == [2, 2, 2] and p["kf2"].tolist() == [0, 1, 3] and p["out0"].tolist() == [0, 30, 60]
    q = bow_pairs([0, 1], [3, 3], ekfs)
    assert q["out0"].tolist() == [0, 10] and len(bow_pairs(0, [], ekfs)) == 0


def test_merge_chains_into_sim3_ransac_rows():
    """vpMatchedPoints from bow_merge is the `match` of Sim3Solver's constructor loop"""
    ids = [np.array([100, 101, 102]), np.array([200, 102, 201])]
    rows = [rows_of([BOW_OK, BOW_NO_POINT, BOW_OK, BOW_RATIO], [0, -1, 2, 1]), rows_of([BOW_RATIO, BOW_OK, BOW_OK, BOW_OK], [0, 0, 1, 2])]
    point, pair, n = bow_merge(rows, ids)
    assert point.tolist() == [100, 200, 102, 201] and pair.tolist() == [0, 1, 0, 1] and n == 4
    n1 = 4
    X = np.arange(n1 * 3, dtype=np.float32).reshape(n1, 3)
    corr, idx = sim3_ransac_rows(point >= 0, np.array([1, 1, 0, 1], bool), np.zeros(n1, bool), np.zeros(n1, bool),
                                 np.arange(n1), np.array([5, 6, 7, -1]), np.zeros(n1, int), np.zeros(n1, int), X, X + 1,
                                 np.ones(n1, np.float32), np.full(n1, 1.44, np.float32))
    assert idx.tolist() == [0, 1]          # keypoint 2 has no point of its own, keypoint 3's point no index in its keyframe
    assert corr["X1b"].tolist() == X[:2].tolist() and corr["X2b"].tolist() == (X[:2] + 1).tolist()
    assert corr["max_err1"].tolist() == [9, 9] and corr["max_err2"].tolist() == [13, 13]
