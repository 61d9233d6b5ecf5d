"""lba_match_fuse on the GPU: every named case (tests/fuse_cases.py) in both modes IDENTICAL to the restatement
(tests/fuse_oracle.py) in every row (status, feat, best_dist, level, n_cand, the bits of x, y, radius) and in n_ok, with
no tolerance; and, without an oracle, bitwise: a 21-search batch against each search alone, two runs, a fresh tracker
against one that ran lba_match_project and lba_match_sim3_project before; the two chains on one handle
(match_epipolar -> triangulate -> match_fuse -> fuse_walk on a ToyMap equals fuse_sequential; sim3_project ->
match_fuse (SIM3) -> fuse_walk + search_and_fuse_replaces likewise); refused calls write nothing and leave a message.

Outputs are pre-filled with junk, so every row must be written; inputs come back byte for byte; nothing is written
behind the last row.  Every case and seed used here is settled (tests/test_fuse_cases.py checks that on the CPU)."""
import numpy as np
import pytest

import fuse_cases as fc
import fuse_oracle as fo
from amc_lba.abi import FUSE_ROW_DTYPE, LBA_E_ARG, LBA_E_LIMIT
from amc_lba.fuse import (FUSE_KF, FUSE_MAX_CAM, FUSE_OK, FUSE_SIM3, TH_KF, TH_LOW, TH_SIM3, FusePack, fuse_raw,
                          pack_searches, pack_targets, split_rows)
from amc_lba.match import MATCH_MAX_FEAT, build_grid, tracker_last_error
from amc_lba.track import Tracker, track_config

pytestmark = pytest.mark.gpu

JUNK = -77
EXTRA = 3
_ref = {}


@pytest.fixture(scope="module")
def tracker():
    t = Tracker(track_config())
    yield t
    t.close()


def reference(key, targets, points, specs):
    """the restatement of a batch, computed once and shared"""
    if key not in _ref:
        _ref[key] = [fo.sequential(targets[t], points[p0:p0 + n], mode, th)[0] for t, p0, n, mode, th in specs]
    return _ref[key]


def device(tracker, targets, points, specs, expect=0, th_low=TH_LOW, pk=None, S=None, n_rows=None):
    """per search its rows [n_points, n_cam] and the search records, after the junk, input and overrun checks"""
    pk = pack_targets(targets) if pk is None else pk
    S = pack_searches(pk.T, specs) if S is None else S
    S["n_ok"] = JUNK
    points = np.ascontiguousarray(points)
    pk0, S0, points0 = pk.copy(), S.copy(), points.copy()
    if n_rows is None:
        n_rows = sum(int(s["n_points"]) * int(pk.T[s["target"]]["n_cam"]) for s in S)
    rows = np.full(8 * (n_rows + EXTRA), JUNK, np.int32).view(FUSE_ROW_DTYPE)
    rc = fuse_raw(tracker, pk, S, points, rows[:n_rows], th_low)
    assert rc == expect, (rc, tracker_last_error(tracker))
    for a in FusePack.ARRAYS:
        assert getattr(pk, a).tobytes() == getattr(pk0, a).tobytes(), a
    assert points.tobytes() == points0.tobytes()
    for f in S.dtype.names:
        if f != "n_ok":
            assert S[f].tobytes() == S0[f].tobytes(), f
    assert (rows[n_rows:].view(np.int32) == JUNK).all()
    if expect != 0:
        assert (rows.view(np.int32) == JUNK).all() and (S["n_ok"] == JUNK).all()
        assert tracker_last_error(tracker).startswith("lba_match_fuse: ")
        return None, S
    return split_rows(pk.T, S, rows), S


def identical(got, S, want, label):
    for i, (g, w) in enumerate(zip(got, want)):
        for f in ("status", "feat", "best_dist", "level", "n_cand"):
            assert (g[f] == w[f]).all(), (label, i, f, np.argwhere(g[f] != w[f])[:5])
        for f in ("x", "y", "radius"):
            assert (g[f].view(np.uint32) == w[f].view(np.uint32)).all(), (label, i, f)
        assert int(S[i]["n_ok"]) == int((w["status"] == FUSE_OK).sum()), (label, i)


@pytest.mark.parametrize("mode", fc.MODES, ids=("kf", "sim3"))
@pytest.mark.parametrize("name", fc.NAMES)
def test_case_identical_to_restatement(tracker, name, mode):
    c = fc.case(name)
    got, S = device(tracker, c.targets, c.points, c.specs(mode))
    identical(got, S, reference((name, mode), c.targets, c.points, c.specs(mode)), (name, mode))


def neighbours_batch(seed, mode):
    """SearchInNeighbors' shape: 20 searches that share keyframe 0's points, then one search with a long list into
    keyframe 0 (mode SIM3: 21 searches that share the list)"""
    prob = fc.gpu_problem(seed)
    ids = prob.kf_points(0)
    cand = np.unique(np.concatenate([prob.kf_points(k) for k in range(1, 21)]))
    cand = cand[cand >= 0]
    points = np.concatenate([prob.points(ids), prob.points(cand)])
    th = TH_KF if mode == FUSE_KF else TH_SIM3
    specs = [(k, 0, len(ids), mode, th) for k in range(1, 21)] + [(0, len(ids), len(cand), mode, th)]
    return prob, points, specs


@pytest.mark.parametrize("seed", fc.GPU_SEEDS)
def test_generated_batch_identical_to_restatement(tracker, seed):
    mode = fc.MODES[seed % 2]
    prob, points, specs = neighbours_batch(seed, mode)
    got, S = device(tracker, prob.targets, points, specs)
    identical(got, S, reference(("gen", seed, mode), prob.targets, points, specs), ("gen", seed))


def bitwise(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("mode", fc.MODES, ids=("kf", "sim3"))
def test_batch_of_21_equals_each_search_alone_and_a_second_run(tracker, mode):
    prob, points, specs = neighbours_batch(0, mode)
    batch, S = device(tracker, prob.targets, points, specs)
    again, S2 = device(tracker, prob.targets, points, specs)
    assert bitwise(batch, again) and S.tobytes() == S2.tobytes()
    for k, (t, p0, n, m, th) in enumerate(specs):
        alone, S1 = device(tracker, [prob.targets[t]], points[p0:p0 + n], [(0, 0, n, m, th)])
        assert alone[0].tobytes() == batch[k].tobytes(), k
        assert int(S1[0]["n_ok"]) == int(S[k]["n_ok"])


def test_fresh_tracker_equals_one_that_ran_other_searches_before(tracker):
    import s3p_cases as sc
    from amc_lba.match import MATCH_RATIO, make_match_search, match_params, match_searches
    from amc_lba.sim3_project import sim3_project
    prob, points, specs = neighbours_batch(1, FUSE_KF)
    s = make_match_search(mode=MATCH_RATIO, seed=3)
    match_searches(tracker, [s], match_params(MATCH_RATIO, s.n_cam))
    kfm, hyps = sc.gpu_problem(sc.GPU_SEEDS[0])
    sim3_project(tracker, kfm, hyps, sc.params(sc.PARAMS[0]))
    used, S = device(tracker, prob.targets, points, specs)
    fresh = Tracker(track_config())
    try:
        new, Sn = device(fresh, prob.targets, points, specs)
    finally:
        fresh.close()
    assert bitwise(used, new) and S.tobytes() == Sn.tobytes()


def test_profile_reports_the_kernel(tracker):
    prob, points, specs = neighbours_batch(0, FUSE_KF)
    assert tracker.fuse_kernel_ms(True) is not None
    device(tracker, prob.targets, points, specs)
    ms = tracker.fuse_kernel_ms(False)
    assert ms > 0.0


# ---------------------------------------------------------------- the chains on one handle
def _device_rows(tracker):
    def rows_fn(targets, points, mode, th):
        got, _ = device(tracker, targets, points, [(i, 0, len(points), mode, th) for i in range(len(targets))])
        return got
    return rows_fn


def test_local_mapping_chain_on_one_handle(tracker):
    """match_epipolar -> triangulate on the handle (their own generated pair: no generator ties triangulated points to
    a fuse scene), then SearchInNeighbors on the same handle: match_fuse for the neighbours, fuse_walk on a ToyMap,
    match_fuse for the candidates into the current keyframe, fuse_walk; the map equals fuse_sequential's"""
    import test_fuse_walk as tw
    from amc_lba.abi import TRI_PAIR_DTYPE
    from amc_lba.epipolar import epi_matches, make_epi_pairs
    from amc_lba.fuse import make_fuse_problem
    from amc_lba.triangulate import tri_params, tri_rows
    pairs, kfs, ekfs, cams, feats, nid, nst, nf, truth = make_epi_pairs(1, 4, 150, 30, seed=9)
    pairs, out = tracker.match_epipolar(pairs, kfs, ekfs, cams, 4, feats, nid, nst, nf)
    m = epi_matches(pairs[0], out, ekfs)
    tp = np.zeros(1, TRI_PAIR_DTYPE)
    tp[0]["kf1"], tp[0]["kf2"], tp[0]["n_rows"] = pairs[0]["kf1"], pairs[0]["kf2"], len(m)
    tp, _ = tracker.triangulate(tp, tri_rows(m, truth["kf"][pairs[0]["kf1"]], truth["kf"][pairs[0]["kf2"]], 4), kfs, cams, 4,
                                tri_params(1.2))
    assert tp[0]["n_new"] > 0
    prob = make_fuse_problem(n_kf=7, n_cam=4, n_feat=100, n_points=220, seed=2, duplicates=0.1)
    tally = tw.Tally()
    mw, ms = tw.search_in_neighbors(prob, 0, list(range(1, 7)), tally, rows_fn=_device_rows(tracker))
    assert tw.same(mw, ms) and tally.decided > 200
    print("local mapping chain: %d redone of %d OK / TOO_FAR rows" % (tally.redone, tally.decided))


def test_loop_closing_chain_on_one_handle(tracker):
    """sim3_project on the handle (its own generated keyframe), then SearchAndFuse on the same handle: match_fuse
    (SIM3) for every corrected keyframe, fuse_walk and search_and_fuse_replaces keyframe after keyframe"""
    import s3p_cases as sc
    import test_fuse_walk as tw
    from amc_lba.fuse import make_fuse_problem
    from amc_lba.sim3_project import sim3_project
    kfm, hyps = sc.gpu_problem(sc.GPU_SEEDS[0])
    assert sum(r.n_matches for r in sim3_project(tracker, kfm, hyps, sc.params(sc.PARAMS[0]))) > 0
    prob = make_fuse_problem(n_kf=8, n_cam=4, n_feat=100, n_points=220, seed=103, duplicates=0.1)
    lst = tw.loop_list(prob, fo.ToyMap.from_problem(prob), [0, 1])
    tally = tw.Tally()
    mw, ms = tw.search_and_fuse(prob, list(range(2, 8)), lst, tally, rows_fn=_device_rows(tracker))
    assert tw.same(mw, ms) and tally.decided > 200
    print("loop closing chain: %d redone of %d OK / TOO_FAR rows" % (tally.redone, tally.decided))


# ---------------------------------------------------------------- refusals
def _refusal_base():
    c = fc.case("mixed_targets")
    return c, pack_targets(c.targets), c.specs(FUSE_KF)


def _refuse(tracker, code, pk=None, S=None, th_low=TH_LOW, points=None):
    c, pk0, specs = _refusal_base()
    pk = pk0 if pk is None else pk
    S0 = pack_searches(pk0.T, specs)
    n_rows = int(S0[-1]["row0"]) + int(S0[-1]["n_points"]) * int(pk0.T[S0[-1]["target"]]["n_cam"])
    device(tracker, None, c.points if points is None else points, None, expect=code, th_low=th_low, pk=pk,
           S=S0 if S is None else S, n_rows=n_rows)


def test_refusals_write_nothing_and_leave_a_message(tracker):
    c, pk0, specs = _refusal_base()
    S0 = pack_searches(pk0.T, specs)

    def with_T(field, k, value):
        pk = pk0.copy()
        pk.T[k][field] = value
        return pk

    def with_S(field, k, value):
        S = S0.copy()
        S[k][field] = value
        return S

    arg, lim = LBA_E_ARG, LBA_E_LIMIT
    # malformed grids
    pk = pk0.copy(); pk.cell_start[int(pk.T[0]["cell0"])] = 1
    _refuse(tracker, arg, pk=pk)
    pk = pk0.copy(); pk.cell_start[int(pk.T[0]["cell0"]) + 100] += 5000
    _refuse(tracker, arg, pk=pk)
    pk = pk0.copy(); pk.cell_feat[0] = int(pk.T[0]["n_feat"])
    _refuse(tracker, arg, pk=pk)
    pk = pk0.copy(); pk.cell_feat[0] = -1
    _refuse(tracker, arg, pk=pk)
    pk = pk0.copy(); f = int(pk.cell_feat[0]); pk.feats["cam"][f] = (pk.feats["cam"][f] + 1) % 4
    _refuse(tracker, arg, pk=pk)
    pk = pk0.copy(); pk.feats["octave"][0] = 256
    _refuse(tracker, arg, pk=pk)
    pk = pk0.copy(); pk.feats["cam"][0] = 4
    _refuse(tracker, arg, pk=pk)
    # ranges outside their arrays
    _refuse(tracker, arg, pk=with_T("cam0", 3, len(pk0.fcams) - 3))
    _refuse(tracker, arg, pk=with_T("feat0", 3, len(pk0.feats)))
    _refuse(tracker, arg, pk=with_T("cell0", 3, len(pk0.cell_start) - 10))
    _refuse(tracker, arg, pk=with_T("cf0", 3, len(pk0.cell_feat)))
    _refuse(tracker, arg, pk=with_T("sf0", 0, len(pk0.sf) - 2))
    _refuse(tracker, arg, pk=with_T("sigma0", 0, -1))
    _refuse(tracker, arg, S=with_S("target", 0, len(pk0.T)))
    _refuse(tracker, arg, S=with_S("point0", 0, len(c.points)))
    _refuse(tracker, arg, S=with_S("n_points", 2, -1))
    _refuse(tracker, arg, S=with_S("row0", 1, 0))                     # overlaps search 0
    _refuse(tracker, arg, S=with_S("row0", 5, 10 ** 6))               # past the end of rows
    # n_cam, n_levels, th, mode, th_low
    _refuse(tracker, arg, pk=with_T("n_cam", 1, 0))
    _refuse(tracker, arg, pk=with_T("n_levels", 0, 0))
    _refuse(tracker, arg, S=with_S("th", 0, -1.0))
    _refuse(tracker, arg, S=with_S("th", 0, np.nan))
    _refuse(tracker, arg, S=with_S("th", 0, np.inf))
    _refuse(tracker, arg, S=with_S("mode", 0, 2))
    _refuse(tracker, arg, th_low=-1)


def test_limits_are_refused(tracker):
    # n_cam > 64
    t = fc.target(FUSE_MAX_CAM + 1, [])
    pts = fc.point(100.0, 100.0, 2, fc.D(1))
    device(tracker, [t], pts, [(0, 0, 1, FUSE_KF, TH_KF)], expect=LBA_E_LIMIT)
    # more than LBA_MATCH_MAX_FEAT features in one camera
    big = fc.target(1, [])
    n = MATCH_MAX_FEAT + 1
    big.feats = np.zeros(n, big.feats.dtype)
    big.feats["x"], big.feats["y"] = np.linspace(5, 600, n), 100.0
    big.cell_start, big.cell_feat = build_grid(big.feats, big.gcams)
    device(tracker, [big], pts, [(0, 0, 1, FUSE_KF, TH_KF)], expect=LBA_E_LIMIT)
    # (an arena above 2 GB needs two gigabytes of rows on the host: not exercised here, as for the sibling calls)
    # the tracker is as usable as before
    c = fc.case("span_65")
    got, S = device(tracker, c.targets, c.points, c.specs(FUSE_KF))
    identical(got, S, reference(("span_65", FUSE_KF), c.targets, c.points, c.specs(FUSE_KF)), "after refusals")


def test_valid_edge_shapes(tracker):
    c = fc.case("empty_target")
    got, S = device(tracker, c.targets, c.points, [])                       # n_searches == 0
    assert got == []
    got, S = device(tracker, c.targets, c.points, [(0, 0, 0, FUSE_KF, TH_KF), (0, 2, 0, FUSE_SIM3, TH_SIM3)])
    assert [g.shape for g in got] == [(0, 3), (0, 3)] and (S["n_ok"] == 0).all()
    one = fc.target(1, [fc.feat(0, 100.5, 100.5, 2, fc.D(1))])
    got, S = device(tracker, [one], fc.point(100.0, 100.0, 2, fc.D(1)), [(0, 0, 1, FUSE_SIM3, TH_SIM3)])
    assert fc.names(got[0]["status"]) == ["NO_CAMERA"] and int(S[0]["n_ok"]) == 0
