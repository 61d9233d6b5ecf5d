"""lba_match_bow on the GPU: every named case (tests/bow_cases.py) in both overloads IDENTICAL to the restatement
(tests/bow_oracle.py: `sequential`) in idx2, dist, dist2, status and n_matches, with no tolerance and no filter; the
flag, tie and ratio variants on generated pairs; and, without an oracle, bitwise: a 33-pair batch sharing its KF1
against each pair alone, two runs, a fresh tracker against one that ran lba_match_epipolar on the same arrays; the
chain into lba_sim3_ransac; refused calls write nothing and leave a message.

Outputs are pre-filled with junk, so every row must be written; inputs come back as passed."""
import ctypes

import numpy as np
import pytest

import bow_cases as bc
import bow_oracle as bo
from amc_lba.abi import BOW_PAIR_DTYPE, BOW_ROW_DTYPE, EPI_FEAT_DTYPE, LBA_E_ARG, LBA_E_LIMIT, TRI_CAM_DTYPE, TRI_KF_DTYPE, ptr
from amc_lba.bow import (BOW_FRAME, BOW_KF, BOW_MAX_NODE, BOW_NO_NODE, LbaBowParams, _bind, bow_merge, bow_pairs, bow_params,
                         bow_rows, frame_matches, make_bow_pairs)
from amc_lba.epipolar import epi_pairs, pack_epi_keyframes
from amc_lba.sim3_ransac import draw_triples, make_sim3_ransac_pairs, sim3_ransac_rows
from amc_lba.track import Tracker, track_config

pytestmark = pytest.mark.gpu

JUNK = -77
ARRAYS = ("ekfs", "feats", "node_id", "node_start", "node_feat")


@pytest.fixture(scope="module")
def tracker():
    t = Tracker(track_config())
    yield t
    t.close()


def device(tracker, c, prm=None):
    """(pairs, out) with every output pre-filled with junk; the inputs are checked to come back as passed"""
    pairs = c.pairs.copy()
    pairs["n_matches"] = JUNK
    n_out = int((c.pairs["out0"] + c.ekfs["n_feat"][c.pairs["kf1"]]).max()) if len(c.pairs) else 0
    out = np.full(4 * (n_out + 3), JUNK, np.int32).view(BOW_ROW_DTYPE)
    ins = [getattr(c, a).copy() for a in ARRAYS]
    p = bow_params(**dict(bo.PRM, **(c.prm if prm is None else prm)))
    pairs, out = tracker.match_bow(pairs, *ins, p, out=out)
    for a, name in zip(ins, ARRAYS):
        assert a.tobytes() == getattr(c, name).tobytes()
    for f in ("kf1", "kf2", "out0"):
        assert (pairs[f] == c.pairs[f]).all()
    assert (out[n_out:].view(np.int32) == JUNK).all()       # nothing behind the last pair's rows
    return pairs, out[:n_out]


def results(c, pairs, out):
    res = []
    for P in pairs:
        r = bow_rows(P, out, c.ekfs)
        res.append(bo.Result(*(r[f].astype(np.int64) for f in ("idx2", "dist", "dist2", "status")), int(P["n_matches"])))
    return res


def identical(res, want, label):
    assert len(res) == len(want)
    for p, (r, w) in enumerate(zip(res, want)):
        for f in ("idx2", "dist", "dist2", "status"):
            assert (getattr(r, f) == getattr(w, f)).all(), (label, p, f, np.flatnonzero(getattr(r, f) != getattr(w, f))[:10])
        assert r.n_matches == w.n_matches, (label, p)
        took = r.idx2[(r.status == bo.OK) | (r.status == bo.ROT)]
        assert len(np.unique(took)) == len(took), (label, p, "idx2 is not unique among the accepted rows")


@pytest.mark.parametrize("mode", bc.MODES, ids=bc.MODE_NAMES.get)
@pytest.mark.parametrize("name", bc.NAMES)
def test_case_identical_to_restatement(tracker, name, mode):
    c, seq = bc.case(name, mode)
    pairs, out = device(tracker, c)
    res = results(c, pairs, out)
    print(f"{name}/{bc.MODE_NAMES[mode]}: statuses {np.bincount(out['status'], minlength=6).tolist()}; n_matches {pairs['n_matches'][:4].tolist()}")
    identical(res, seq, name)
    c.prop(c, res)


@pytest.mark.parametrize("mode", bc.MODES, ids=bc.MODE_NAMES.get)
def test_variants_on_generated_pairs(tracker, mode):
    """the pairs on which tests/test_bow_cases.py counts what a device without the flag, with ties to the last position
    or with the ratio product in double would change (at least 20 rows each), at nn_ratio 0.6f; then other flags"""
    c = bc.generated(*bc.VARIANT_PAIRS, mode, dict(nn_ratio=0.6), **bc.VARIANT_GEN)
    jobs = bo.jobs_of(c)
    seq = [bo.sequential(j) for j in jobs]
    res = results(c, *device(tracker, c))
    identical(res, seq, "nn_ratio 0.6")
    for wrong in (dict(flag=False), dict(tie="last"), dict(ratio_double=True)):
        n = sum(bo.rows_differing(r, bo.sequential(j, **wrong)) for r, j in zip(res, jobs))
        print(f"{bc.MODE_NAMES[mode]}: the device differs from {wrong} in {n} rows")
        assert n >= 20
    for prm in (dict(nn_ratio=0.8), dict(check_orientation=0), dict(th_low=30), dict(th_low=0), dict(th_low=255, nn_ratio=0.75)):
        prm = dict(prm, mode=mode)
        identical(results(c, *device(tracker, c, prm)), [bo.sequential(j) for j in bo.jobs_of(c, prm)], str(prm))


def _batch():
    """33 pairs sharing KF1 (DetectCommonRegionsFromBoW: 3 candidates x 11 covisible keyframes)"""
    pairs, ekfs, feats, nid, nst, nf, truth = make_bow_pairs(33, n_feat=200, n_nodes=10, seed=21, cluster=4)
    return bc.Case(pairs, ekfs, feats, nid, nst, nf, {}, None), truth


def test_batch_equals_each_pair_alone_two_runs(tracker):
    c, _ = _batch()
    bp, bo_ = device(tracker, c)
    again = device(tracker, c)
    assert again[0].tobytes() == bp.tobytes() and again[1].tobytes() == bo_.tobytes()
    assert (bp["n_matches"] > 0).all() and (bo_["status"] == BOW_NO_NODE).any()
    for k in range(len(c.pairs)):
        one = c._replace(pairs=c.pairs[k:k + 1].copy())
        one.pairs["out0"] = 0
        sp, so = device(tracker, one)
        assert so.tobytes() == bow_rows(bp[k], bo_, c.ekfs).tobytes(), k
        assert sp[0]["n_matches"] == bp[k]["n_matches"]
    # ... and against the restatement, on a few of them
    seq = [bo.sequential(j) for j in bo.jobs_of(c._replace(pairs=c.pairs[::8]))]
    identical(results(c, bp[::8], bo_), seq, "batch")


def test_fresh_tracker_and_epipolar_between(tracker):
    """a tracker that ran lba_match_epipolar on the same keyframe arrays before gives what a fresh one gives"""
    c, _ = _batch()
    other = Tracker(track_config())
    fresh = device(other, c)
    other.close()
    kfs, cams = np.zeros(len(c.ekfs), TRI_KF_DTYPE), np.zeros(len(c.ekfs), TRI_CAM_DTYPE)
    kfs["cam0"] = np.arange(len(c.ekfs))
    for C in cams:
        C["Tcw"] = np.eye(3, 4).ravel()
        C["fx"], C["fy"], C["cx"], C["cy"], C["invfx"], C["invfy"] = 500.0, 500.0, 480.0, 300.0, 1 / 500.0, 1 / 500.0
    ep, eo_ = tracker.match_epipolar(epi_pairs(c.pairs["kf1"], c.pairs["kf2"], c.ekfs), kfs, c.ekfs, cams, 1, c.feats, c.node_id,
                                     c.node_start, c.node_feat)
    assert len(eo_) == len(fresh[1])
    after = device(tracker, c)
    assert after[0].tobytes() == fresh[0].tobytes() and after[1].tobytes() == fresh[1].tobytes()


def test_default_parameters_and_profile(tracker):
    c, _ = _batch()
    args = [getattr(c, a) for a in ARRAYS]
    a = tracker.match_bow(c.pairs.copy(), *args, None)
    b = tracker.match_bow(c.pairs.copy(), *args, LbaBowParams(BOW_KF, 50, 0.9, 1))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    tracker.match_bow_kernel_ms(True)
    device(tracker, c)
    ms = tracker.match_bow_kernel_ms(False)
    print(f"33 pairs x 200 keypoints: k_bow_match {ms * 1e3:.1f} us")
    assert 0.0 < ms < 1000.0


def test_frame_mode_scatter(tracker):
    c, seq = bc.case("generated_3x300", BOW_FRAME)
    pairs, out = device(tracker, c)
    for P, s in zip(pairs, seq):
        got = frame_matches(P, out, int(c.ekfs[P["kf2"]]["n_feat"]), c.ekfs)
        ok = np.flatnonzero(s.status == bo.OK)
        assert (got >= 0).sum() == len(ok) == P["n_matches"] and (got[s.idx2[ok]] == ok).all()


def test_matches_chain_into_sim3_ransac(tracker):
    """match_bow -> bow_merge -> sim3_ransac_rows -> Tracker.sim3_ransac on the tracker handle: the keypoints of KF1 get
    the body points of a synthetic Sim3 candidate, a correct match the true partner's, any other a point metres off"""
    n1, n_cam, n_hyp = 300, 2, 300
    pairs, ekfs, feats, nid, nst, nf, truth = make_bow_pairs(5, n_feat=n1, n_nodes=12, seed=31)
    pairs, out = tracker.match_bow(pairs, ekfs, feats, nid, nst, nf)
    point, kf_of, n = bow_merge([bow_rows(P, out, ekfs) for P in pairs], truth["point_id"][1:])
    assert n >= (point >= 0).sum() >= 60          # (numBoWMatches also counts the points a later keyframe overwrote)
    rp, corr, _, cams, _ = make_sim3_ransac_pairs(1, n_corr=n1, n_cam=n_cam, outlier_frac=0.0, seed=4, n_hyp=n_hyp)
    X2b = corr["X2b"].copy()
    rng = np.random.default_rng(8)
    for k in np.flatnonzero(point >= 0):
        j = int(kf_of[k])
        idx2 = int(bow_rows(pairs[j], out, ekfs)["idx2"][k])
        if truth["member"][j][idx2] != k:
            X2b[k] += rng.uniform(1.0, 5.0, 3).astype(np.float32)
    yes, no = np.ones(n1, bool), np.zeros(n1, bool)
    rows, idx = sim3_ransac_rows(point >= 0, feats["has_point"][:n1] != 0, no, no, np.arange(n1), np.arange(n1), corr["cam1"],
                                 corr["cam2"], corr["X1b"], X2b, np.ones(n1, np.float32), np.ones(n1, np.float32))
    assert (idx == np.flatnonzero(point >= 0)).all()
    rp["corr0"], rp["n_corr"], rp["hyp0"], rp["n_hyp"] = 0, len(rows), 0, n_hyp
    rp, rows = tracker.sim3_ransac(rp, rows, draw_triples(len(rows), n_hyp, rng), cams, n_cam, per_hyp=False)
    assert rp[0]["best_hyp"] >= 0 and rp[0]["n_inliers"] >= 15 and rows["inlier"].sum() == rp[0]["n_inliers"]


def _args(tracker, c, p_arr, o_arr, **over):
    a = dict(pairs=ptr(p_arr), n_pairs=len(p_arr), out=ptr(o_arr), n_out=len(o_arr), ekfs=ptr(c.ekfs), n_kf=len(c.ekfs),
             feats=ptr(c.feats), n_feats=len(c.feats), node_id=ptr(c.node_id), node_start=ptr(c.node_start),
             n_node_rows=len(c.node_id), node_feat=ptr(c.node_feat), n_node_feat=len(c.node_feat), prm=None)
    a.update(over)
    return [tracker.h] + list(a.values())


def _refused(tracker, c, code=LBA_E_ARG, **over):
    """the call with some arguments or arrays replaced is refused, writes nothing and leaves a message"""
    repl = {k: np.ascontiguousarray(v) for k, v in over.items() if isinstance(v, np.ndarray)}
    c2 = c._replace(**{k: v for k, v in repl.items() if k in c._fields})
    pairs, out = c2.pairs.copy(), np.full(len(c.feats) * 4 * max(1, len(c.pairs)), JUNK, np.int32).view(BOW_ROW_DTYPE)
    pairs["n_matches"] = JUNK
    before = pairs.copy()
    raw = {k: v for k, v in over.items() if not isinstance(v, np.ndarray)}
    rc = _bind().lba_match_bow(*_args(tracker, c2, pairs, out, **raw))
    assert rc == code, (list(over.keys()), rc)
    assert pairs.tobytes() == before.tobytes() and (out.view(np.int32) == JUNK).all()
    assert len(tracker.last_error()) > 0


def _mod(arr, k, field, value):
    out = arr.copy()
    if field is None:
        out[k] = value
    else:
        out[field][k] = value
    return out


def _small():
    pairs, ekfs, feats, nid, nst, nf, _ = make_bow_pairs(4, n_feat=80, n_nodes=6, seed=11)
    return bc.Case(pairs, ekfs, feats, nid, nst, nf, {}, None)


def test_refused_calls_write_nothing_and_the_next_call_succeeds(tracker):
    c = _small()
    L = _bind()
    pairs, out = c.pairs.copy(), np.zeros(len(c.feats), BOW_ROW_DTYPE)
    assert L.lba_match_bow(None, *_args(tracker, c, pairs, out)[1:]) == LBA_E_ARG
    for null in ("pairs", "out", "ekfs", "feats", "node_id", "node_start", "node_feat"):
        _refused(tracker, c, **{null: None})
    for neg in ("n_pairs", "n_out", "n_kf", "n_feats", "n_node_rows", "n_node_feat"):
        _refused(tracker, c, **{neg: -1})
    _refused(tracker, c, pairs=_mod(c.pairs, 1, "kf1", -1))
    _refused(tracker, c, pairs=_mod(c.pairs, 1, "kf2", len(c.ekfs)))
    _refused(tracker, c, n_kf=len(c.ekfs) - 1)
    _refused(tracker, c, pairs=_mod(c.pairs, 1, "out0", -1))
    _refused(tracker, c, pairs=_mod(c.pairs, 3, "out0", c.pairs["out0"][2] + 1))           # overlaps its neighbour
    _refused(tracker, c, n_out=int(c.pairs["out0"][-1]) + int(c.ekfs["n_feat"][0]) - 1)     # the last range is cut short
    _refused(tracker, c, ekfs=_mod(c.ekfs, 1, "feat0", -1))
    _refused(tracker, c, ekfs=_mod(c.ekfs, 4, "n_feat", c.ekfs["n_feat"][4] + 1))
    _refused(tracker, c, n_feats=len(c.feats) - 1)
    _refused(tracker, c, ekfs=_mod(c.ekfs, 4, "n_node", c.ekfs["n_node"][4] + 1))           # past node_id / node_start
    _refused(tracker, c, ekfs=_mod(c.ekfs, 1, "node0", -1))
    _refused(tracker, c, ekfs=_mod(c.ekfs, 4, "nf0", c.ekfs["nf0"][4] + 1))                 # past node_feat
    n0 = int(c.ekfs["node0"][3])
    _refused(tracker, c, node_id=_mod(c.node_id, n0 + 1, None, c.node_id[n0]))              # not strictly ascending
    _refused(tracker, c, node_start=_mod(c.node_start, n0, None, 1))                        # does not start at 0
    _refused(tracker, c, node_start=_mod(c.node_start, n0 + 1, None, c.node_start[n0 + 2] + 1))    # decreases behind it
    f0 = int(c.ekfs["nf0"][3])
    _refused(tracker, c, node_feat=_mod(c.node_feat, f0, None, -1))
    _refused(tracker, c, node_feat=_mod(c.node_feat, f0, None, c.ekfs["n_feat"][3]))
    _refused(tracker, c, node_feat=_mod(c.node_feat, f0, None, c.node_feat[f0 + 1]))        # listed twice
    for bad in (LbaBowParams(BOW_KF, -1, 0.9, 1), LbaBowParams(BOW_KF, 256, 0.9, 1), LbaBowParams(2, 50, 0.9, 1),
                LbaBowParams(-1, 50, 0.9, 1), LbaBowParams(BOW_FRAME, 50, float("nan"), 1), LbaBowParams(BOW_KF, 50, float("inf"), 1)):
        _refused(tracker, c, prm=ctypes.byref(bad))
    # the next valid call runs clean and gives what the restatement gives
    identical(results(c, *device(tracker, c)), [bo.sequential(j) for j in bo.jobs_of(c)], "after the refusals")


def test_node_list_limit(tracker):
    """a side-2 list of exactly LBA_BOW_MAX_NODE entries runs (the case list2_2048 holds it against the restatement);
    one entry more is refused with LBA_E_LIMIT, in either overload, and only where the long list is on side 2"""
    n = BOW_MAX_NODE + 1
    rng = np.random.default_rng(3)
    f = np.zeros(n, EPI_FEAT_DTYPE)
    f["desc"], f["has_point"] = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32), 1
    ekfs, feats, nid, nst, nf = pack_epi_keyframes([f[:3], f], [np.zeros(3, int), np.zeros(n, int)])
    c = bc.Case(bow_pairs(0, [1], ekfs), ekfs, feats, nid, nst, nf, {}, None)
    for mode in bc.MODES:
        prm = LbaBowParams(mode, 50, 0.9, 1)
        _refused(tracker, c, code=LBA_E_LIMIT, prm=ctypes.byref(prm))
    assert "LBA_BOW_MAX_NODE" in tracker.last_error()
    back = c._replace(pairs=bow_pairs(1, [0], ekfs))         # the long list on side 1: no limit
    identical(results(back, *device(tracker, back)), [bo.sequential(j) for j in bo.jobs_of(back)], "long side 1")


def test_empty_calls(tracker):
    c = _small()
    L = _bind()
    none = np.zeros(0, BOW_PAIR_DTYPE)
    assert L.lba_match_bow(*_args(tracker, c, none, np.zeros(0, BOW_ROW_DTYPE), pairs=None, out=None)) == 0
    # keyframes without features, without nodes, and a pair of a keyframe with itself
    e = c.ekfs.copy()
    e["n_feat"][1], e["n_node"][1], e["n_node"][2] = 0, 0, 0
    pairs = c.pairs.copy()
    pairs["kf1"], pairs["kf2"] = (0, 1, 0, 3), (1, 0, 2, 3)
    pairs["out0"] = (0, 80, 80, 160)
    c2 = c._replace(ekfs=e, pairs=pairs)
    p, o = device(tracker, c2)
    assert p["n_matches"].tolist()[:3] == [0, 0, 0]
    assert (o["status"][:160] == BOW_NO_NODE).all()
    identical(results(c2, p, o), [bo.sequential(j) for j in bo.jobs_of(c2)], "empty keyframes")
    assert p["n_matches"][3] > 0
