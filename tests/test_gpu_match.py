"""lba_match_project on the GPU.  Every output is an integer, so there is no tolerance and no settled subset: on every
named case (tests/match_cases.py), in both modes where it applies, feat, status, best_dist, best_dist2, the per-feature
job, n_matches and n_matches_mono are IDENTICAL to the sequential restatement (tests/match_oracle.py), `rounds` is
identical to the round-based restatement, and the inputs come back byte for byte.  Without an oracle, bitwise: a
40-search batch and a 300-search batch against each search alone, two runs, a fresh tracker against one that ran
lba_triangulate before.  Refused calls return their code, set the tracker's error text and write nothing."""
import ctypes

import numpy as np
import pytest

import match_cases as mc
from amc_lba.abi import LBA_E_ARG, LBA_E_LIMIT, MATCH_CAM_DTYPE, MATCH_FEAT_DTYPE, MATCH_JOB_DTYPE, ptr
from amc_lba.match import (MATCH_BEST, MATCH_JOB_OUTPUTS, MATCH_NO_CAND, MATCH_RATIO, LbaMatchParams, _bind,
                           make_match_search, match_params, match_searches, pack_searches, tracker_last_error)
from amc_lba.track import Tracker, track_config

pytestmark = pytest.mark.gpu

JOB_INPUTS = [f for f in MATCH_JOB_DTYPE.names if f not in MATCH_JOB_OUTPUTS]
FEAT_INPUTS = [f for f in MATCH_FEAT_DTYPE.names if f != "job"]
CAM_INPUTS = [f for f in MATCH_CAM_DTYPE.names if f != "rounds"]
MODES = pytest.mark.parametrize("mode", mc.BOTH, ids=["ratio", "best"])


@pytest.fixture(scope="module")
def tracker():
    t = Tracker(track_config())
    yield t
    t.close()


def _junk(s):
    """a copy whose output fields hold junk, so every one of them must be written"""
    c = s.copy()
    c.feats["job"], c.cams["rounds"] = 77, 77
    for f in MATCH_JOB_OUTPUTS:
        c.jobs[f] = 77
    return c


@pytest.mark.parametrize("name,mode", mc.NAMES, ids=mc.IDS)
def test_case_is_identical_to_the_restatements(tracker, name, mode):
    s, p, seq, rnd, _, _ = mc.case(name, mode)
    S, (out,) = match_searches(tracker, [_junk(s)], p)
    for f in MATCH_JOB_OUTPUTS:
        assert (out.jobs[f] == getattr(seq, f)).all(), (f, np.flatnonzero(out.jobs[f] != getattr(seq, f))[:10])
    assert (out.feats["job"] == seq.job).all()
    assert S[0]["n_matches"] == seq.n_matches and S[0]["n_matches_mono"] == seq.n_matches_mono
    assert (out.cams["rounds"] == rnd.rounds).all(), (out.cams["rounds"], rnd.rounds)
    for arr, ref, fields in ((out.jobs, s.jobs, JOB_INPUTS), (out.feats, s.feats, FEAT_INPUTS), (out.cams, s.cams, CAM_INPUTS)):
        for f in fields:
            assert arr[f].tobytes() == ref[f].tobytes(), f


def _same(a, b):
    return a.jobs.tobytes() == b.jobs.tobytes() and a.feats.tobytes() == b.feats.tobytes() and a.cams.tobytes() == b.cams.tobytes()


def _batch_against_alone(tracker, searches, p_of, picks):
    S, outs = match_searches(tracker, [_junk(s) for s in searches], p_of(None))
    assert S["n_matches"].sum() > 0
    for k in picks:
        S1, (one,) = match_searches(tracker, [_junk(searches[k])], p_of(searches[k]))
        assert _same(one, outs[k]), k
        assert S1[0]["n_matches"] == S[k]["n_matches"] and S1[0]["n_matches_mono"] == S[k]["n_matches_mono"]


@MODES
def test_batch_of_40_equals_each_search_alone(tracker, mode):
    # the searches have 1 .. 4 cameras: stereo_cam 0 is in range for all of them
    _batch_against_alone(tracker, mc.batch(mode), lambda s: match_params(mode, 1), range(40))


@MODES
def test_batch_of_300_small_searches_equals_each_alone(tracker, mode):
    _batch_against_alone(tracker, mc.small_batch(mode), lambda s: match_params(mode, 1), range(300))


@MODES
def test_two_runs_fresh_tracker_and_triangulate_between(tracker, mode):
    from amc_lba.triangulate import make_tri_pairs, tri_params
    s, p, _, _, _, _ = mc.case("generated", mode)
    other = Tracker(track_config())
    _, (fresh,) = match_searches(other, [_junk(s)], p)
    other.close()
    _, (first,) = match_searches(tracker, [_junk(s)], p)
    _, (again,) = match_searches(tracker, [_junk(s)], p)
    pairs, rows, kfs, cams, _ = make_tri_pairs(n_pairs=2, n_rows=60, seed=5)
    tracker.triangulate(pairs, rows, kfs, cams, 4, tri_params(1.2))
    _, (after,) = match_searches(tracker, [_junk(s)], p)
    assert _same(again, first) and _same(after, first) and _same(fresh, first)


def test_not_finite_jobs_have_no_candidates_and_the_call_returns(tracker):
    for mode in mc.BOTH:
        s, p, _, _, _, _ = mc.case("not_finite", mode)
        _, (out,) = match_searches(tracker, [_junk(s)], p)
        assert (out.jobs["status"][:-1] == MATCH_NO_CAND).all() and (out.jobs["feat"][:-1] == -1).all()


# ---- refusals
def _call(tracker, a, p, **over):
    S, cams, cs, cf, feats, jobs = a
    n = dict(n_searches=len(S), n_cams=len(cams), n_cs=len(cs), n_cf=len(cf), n_feats=len(feats), n_jobs=len(jobs))
    n.update(over)
    return _bind().lba_match_project(tracker.h, ptr(S), n["n_searches"], ptr(cams), n["n_cams"], ptr(cs), n["n_cs"], ptr(cf),
                                     n["n_cf"], ptr(feats), n["n_feats"], ptr(jobs), n["n_jobs"],
                                     ctypes.byref(p) if p is not None else None)


def _refused(tracker, a, p, code=LBA_E_ARG, **over):
    b = tuple(x.copy() for x in a)
    # another refusal first, so that the one under test must set the text itself
    assert _bind().lba_match_project(tracker.h, None, -1, None, 0, None, 0, None, 0, None, 0, None, 0, None) == LBA_E_ARG
    before = tracker_last_error(tracker)
    assert _call(tracker, b, p, **over) == code
    text = tracker_last_error(tracker)
    assert text.startswith("lba_match_project: ") and text != before
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))      # nothing written
    return text


def test_refused_calls_write_nothing_and_the_next_call_succeeds(tracker):
    s2 = [make_match_search(mode=MATCH_BEST, n_cam=2, n_feat=40, n_points=30, seed=900 + k) for k in range(2)]
    for s in s2:
        s.feats["job"], s.cams["rounds"] = 55, 55
        for f in MATCH_JOB_OUTPUTS:
            s.jobs[f] = 55
    a = pack_searches(s2)
    a[0]["n_matches"] = a[0]["n_matches_mono"] = -3
    p = match_params(MATCH_BEST, 2)
    L = _bind()

    def mod(i, k, field, value):
        b = [x.copy() for x in a]
        if field is None:
            b[i][k] = value
        else:
            b[i][field][k] = value
        return tuple(b)

    full = (ptr(a[0]), 2, ptr(a[1]), len(a[1]), ptr(a[2]), len(a[2]), ptr(a[3]), len(a[3]), ptr(a[4]), len(a[4]),
            ptr(a[5]), len(a[5]), ctypes.byref(p))
    assert L.lba_match_project(None, *full) == LBA_E_ARG
    texts = set()
    for null in (0, 2, 4, 6, 8, 10, 12):
        b = list(full)
        b[null] = None
        assert L.lba_match_project(tracker.h, *b) == LBA_E_ARG
        assert "null" in tracker_last_error(tracker)
    for neg in (1, 3, 5, 7, 9, 11):
        b = list(full)
        b[neg] = -1
        assert L.lba_match_project(tracker.h, *b) == LBA_E_ARG
        assert "negative" in tracker_last_error(tracker)
    # a search's ranges
    for field, value in (("cam0", -1), ("n_cam", 0), ("n_cam", 3), ("feat0", -1), ("n_feat", -1), ("n_feat", 10 ** 6),
                         ("job0", -1), ("n_jobs", -1), ("n_jobs", 10 ** 6), ("cell0", -1), ("cell0", 2), ("cf0", -1),
                         ("cf0", 10 ** 6)):
        texts.add(_refused(tracker, mod(0, 1, field, value), p))
    texts.add(_refused(tracker, mod(0, 1, "cam0", 1), p))                 # overlaps the search before
    texts.add(_refused(tracker, a, p, n_cams=3))
    texts.add(_refused(tracker, a, p, n_cs=len(a[2]) - 1))
    texts.add(_refused(tracker, a, p, n_cf=len(a[3]) - 1))
    texts.add(_refused(tracker, a, p, n_feats=len(a[4]) - 1))
    texts.add(_refused(tracker, a, p, n_jobs=len(a[5]) - 1))
    # the grid
    cs1 = int(a[0][1]["cell0"])
    first_full = cs1 + int(np.flatnonzero(np.diff(a[2][cs1:]) > 0)[0])      # a cell of search 1 that holds a feature
    texts.add(_refused(tracker, mod(2, cs1, None, 1), p))                   # does not begin at 0
    texts.add(_refused(tracker, mod(2, first_full + 1, None, a[2][first_full + 1] - 2), p))   # decreases
    cf1 = int(a[0][1]["cf0"])
    texts.add(_refused(tracker, mod(3, cf1, None, -1), p))
    texts.add(_refused(tracker, mod(3, cf1, None, len(s2[1].feats)), p))
    f_first = int(a[3][cf1])                                                # the first cell's feature: camera 0's
    other = int(np.flatnonzero(s2[1].feats["cam"] != s2[1].feats["cam"][f_first])[0])
    texts.add(_refused(tracker, mod(3, cf1, None, other), p))               # a feature of another camera
    # features and jobs
    f0, j0 = int(a[0][1]["feat0"]), int(a[0][1]["job0"])
    for field, value in (("cam", -1), ("cam", 2), ("octave", -1), ("octave", 256)):
        texts.add(_refused(tracker, mod(4, f0 + 3, field, value), p))
    for field, value in (("cam", -1), ("cam", 2)):
        texts.add(_refused(tracker, mod(5, j0 + 3, field, value), p))
    b = mod(5, j0 + 3, "min_level", 3)
    b[5]["max_level"][j0 + 3] = 2
    texts.add(_refused(tracker, b, p))                                      # a level range that is not ordered
    # parameters
    for bad in (LbaMatchParams(2, 100, 0.8, 1, 1, 1), LbaMatchParams(-1, 100, 0.8, 1, 1, 1), LbaMatchParams(1, 256, 0.8, 1, 1, 1),
                LbaMatchParams(1, -1, 0.8, 1, 1, 1), LbaMatchParams(1, 100, float("nan"), 1, 1, 1),
                LbaMatchParams(1, 100, 0.8, 2, 1, 1), LbaMatchParams(1, 100, 0.8, -2, 1, 1), LbaMatchParams(0, 100, 0.8, 1, 0, 1)):
        texts.add(_refused(tracker, a, bad))
    assert len(texts) >= 12
    # the limit of the header: one feature more than LBA_MATCH_MAX_FEAT in one camera
    big = pack_searches([mc.over_limit()])
    assert "8192" in _refused(tracker, big, match_params(MATCH_BEST, 1), code=LBA_E_LIMIT)
    # the next valid call runs clean and writes every output
    b = tuple(x.copy() for x in a)
    assert _call(tracker, b, p) == 0
    assert (b[5]["status"] != 55).all() and (b[4]["job"] != 55).all() and (b[1]["rounds"] != 55).all()
    assert (b[0]["n_matches"] > 0).all()
    _, outs = match_searches(tracker, s2, p)
    assert b[5].tobytes() == np.concatenate([o.jobs for o in outs]).tobytes()


def test_empty_calls(tracker):
    p = match_params(MATCH_RATIO, 1)
    assert _bind().lba_match_project(tracker.h, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, ctypes.byref(p)) == 0
    s = make_match_search(mode=MATCH_RATIO, n_cam=2, n_feat=30, n_points=20, seed=77)
    no_jobs = type(s)(s.cams, s.cell_start, s.cell_feat, s.feats, s.jobs[:0])
    S, (out,) = match_searches(tracker, [_junk(no_jobs)], match_params(MATCH_RATIO, 2))
    assert S[0]["n_matches"] == 0 and (out.feats["job"] == -1).all() and (out.cams["rounds"] == 0).all()
