"""lba_triangulate on the GPU: the named cases (tests/tri_cases.py) against the fp64 restatement (tests/tri_oracle.py),
and, without an oracle, bitwise: a 300-pair batch against each pair alone, two runs, a fresh tracker against one that
ran lba_sim3_ransac before; rows that are not LBA_TRI_OK keep their X bytes; refused calls write nothing.

Against the restatement, on settled rows (every fp64 comparison further than 1e-9 relative from its gate): status and
stereo_point identical; n_new / n_stereo the sums of the device's own statuses; X of a triangulated LBA_TRI_OK row
within 2 * 64 * 4 u sigma1 / (sigma3 - sigma4) * (1 + |X|) sqrt(1 + |X|^2) (tri_cases.x_bound: the null vector's bound
of tests/test_tri_math_host.py carried through the division by w), X of a stereo point within 16 u max(1, |X|_inf).
The margins seen are printed (pytest -s) and recorded in profiles/triangulate_margins.log."""
import ctypes

import numpy as np
import pytest

import tri_cases as tc
import tri_oracle as to
from amc_lba.abi import LBA_E_ARG, LBA_E_LIMIT, TRI_CAM_DTYPE, TRI_ROW_DTYPE, ptr
from amc_lba.triangulate import (TRI_MAX_CAM, TRI_OK, TRI_PAIR_OUTPUTS, TRI_ROW_OUTPUTS, LbaTriParams, _bind,
                                 make_tri_pairs, ratio_factor, tri_params)
from amc_lba.track import Tracker, track_config

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
N_BATCH = 300      # pairs of the batch: with one to three chunks each, far more workgroups than an MI355X has CUs (256)
ROW_INPUTS = [f for f in TRI_ROW_DTYPE.names if f not in TRI_ROW_OUTPUTS]


@pytest.fixture(scope="module")
def tracker():
    t = Tracker(track_config())
    yield t
    t.close()


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_matches_restatement(tracker, name):
    c, r64, _ = tc.case(name)
    before = c.rows.copy()
    before["X"] = 7.0
    c_in = tc.Case(c.pairs, before, c.kfs, c.cams, c.n_cam, c.ratio, c.far_points, c.th_far)
    pairs, rows = tc.run_device(tracker, c_in)
    m, st = c.in_pairs(), tc.settled_rows(c, r64)
    print(f"{name}: {int((m & ~st).sum())} of {int(m.sum())} rows unsettled; device statuses {np.bincount(rows['status'][m], minlength=11)}")
    if c.reported:
        print(f"{name}: reported, not compared: status {rows['status'][m]}, X {rows['X'][m]}; restatement {r64.status[m]}, {r64.X[m]}")
    assert (rows["status"][st] == r64.status[st]).all(), np.flatnonzero(st & (rows["status"] != r64.status))
    assert (rows["stereo_point"][st] == r64.stereo[st]).all()
    # the counts are the sums of the device's own statuses; inputs come back as passed
    for p, P in enumerate(pairs):
        sl = slice(int(P["row0"]), int(P["row0"] + P["n_rows"]))
        if name != "shared_rows":
            assert P["n_new"] == (rows["status"][sl] == TRI_OK).sum()
            assert P["n_stereo"] == ((rows["status"][sl] == TRI_OK) & (rows["stereo_point"][sl] != 0)).sum()
        assert 0 <= P["n_stereo"] <= P["n_new"] <= P["n_rows"]
    if name == "shared_rows":      # the rows carry the later pair's result, the counts are per pair
        sl = slice(int(pairs[1]["row0"]), int(pairs[1]["row0"] + pairs[1]["n_rows"]))
        assert pairs[1]["n_new"] == (rows["status"][sl] == TRI_OK).sum()
        assert pairs[0]["n_new"] == r64.n_new[0] or not st.all()
    for f in ROW_INPUTS:
        assert rows[f].tobytes() == c.rows[f].tobytes(), f
    assert rows[~m].tobytes() == before[~m].tobytes()
    # rows that are not LBA_TRI_OK keep their X bytes
    assert (rows["X"][rows["status"] != TRI_OK] == 7.0).all()
    worst_t = worst_s = 0.0
    for i in np.flatnonzero(st & (r64.status == to.OK)):
        if not np.isfinite(r64.X[i]).all():
            assert (np.isnan(rows["X"][i]) == np.isnan(r64.X[i])).all()
            continue
        if r64.triangulated[i]:
            gap, bound = np.linalg.norm(rows["X"][i] - r64.X[i]), tc.x_bound(r64.X[i], r64.sigma[i])
            worst_t = max(worst_t, gap / bound)
        else:
            gap, bound = np.abs(rows["X"][i] - r64.X[i]).max(), 16 * U * max(1.0, np.abs(r64.X[i]).max())
            worst_s = max(worst_s, gap / bound)
        assert gap <= bound, (i, gap, bound)
    print(f"{name}: triangulated X at {worst_t:.2e} of its bound, stereo X at {worst_s:.2e} of its bound")


def _batch():
    """N_BATCH pairs of 70 .. 190 rows, every pair with keyframes of its own"""
    parts = [make_tri_pairs(n_pairs=1, n_rows=n, seed=71 + k)[:4] for k, n in enumerate((70, 129, 190, 64))]
    pairs, rows, kfs, cams, r0 = [], [], [], [], 0
    for p in range(N_BATCH):
        P, R, K, C = (a.copy() for a in parts[p % 4])
        P["row0"], P["kf1"], P["kf2"] = r0, 2 * p, 2 * p + 1
        K["cam0"] = (8 * p, 8 * p + 4)
        pairs.append(P); rows.append(R); kfs.append(K); cams.append(C)
        r0 += len(R)
    return np.concatenate(pairs), np.concatenate(rows), np.concatenate(kfs), np.concatenate(cams)


def test_batch_equals_each_pair_alone(tracker):
    pairs, rows, kfs, cams = _batch()
    prm = tri_params(1.2)
    bp, br = tracker.triangulate(pairs.copy(), rows.copy(), kfs, cams, 4, prm)
    assert bp["n_new"].sum() > 0.2 * len(rows) and (bp["n_new"] < bp["n_rows"]).any()
    for k in list(range(0, N_BATCH, 37)) + [N_BATCH - 1]:
        P = pairs[k]
        one = pairs[k:k + 1].copy()
        sl = slice(int(P["row0"]), int(P["row0"] + P["n_rows"]))
        one["row0"], one["kf1"], one["kf2"] = 0, 0, 1
        okf = kfs[[P["kf1"], P["kf2"]]].copy()
        ocam = np.concatenate([cams[kf["cam0"]:kf["cam0"] + 4] for kf in okf])
        okf["cam0"] = (0, 4)
        sp, sr = tracker.triangulate(one, rows[sl].copy(), okf, ocam, 4, prm)
        assert sr.tobytes() == br[sl].tobytes(), k
        for f in TRI_PAIR_OUTPUTS:
            assert sp[0][f] == bp[k][f], (k, f)


def test_two_runs_fresh_tracker_and_other_calls_between(tracker):
    from amc_lba.sim3_ransac import make_sim3_ransac_pairs
    c, _, _ = tc.case("rows_255_256_257")
    other = Tracker(track_config())
    fresh = tc.run_device(other, c)
    other.close()
    first = tc.run_device(tracker, c)
    again = tc.run_device(tracker, c)
    sp, sc, ss, scams, _ = make_sim3_ransac_pairs(n_pairs=2, n_corr=40, n_hyp=20, seed=5)
    tracker.sim3_ransac(sp, sc, ss, scams, 4)
    after = tc.run_device(tracker, c)
    for res in (again, after, fresh):
        assert res[0].tobytes() == first[0].tobytes() and res[1].tobytes() == first[1].tobytes()


def test_default_parameters(tracker):
    c, _, _ = tc.case("generated")
    dp, dr = tracker.triangulate(c.pairs.copy(), c.rows.copy(), c.kfs, c.cams, 4, None)
    ep, er = tracker.triangulate(c.pairs.copy(), c.rows.copy(), c.kfs, c.cams, 4, LbaTriParams(1.5 * 1.2, 0.0, 0, 0))
    assert dp.tobytes() == ep.tobytes() and dr.tobytes() == er.tobytes()


def _call(tracker, pairs, rows, kfs, cams, n_cam=4, prm=None, n_rows=None, n_kf=None, n_cam_rows=None):
    return _bind().lba_triangulate(tracker.h, ptr(pairs), len(pairs), ptr(rows), len(rows) if n_rows is None else n_rows,
                                   ptr(kfs), len(kfs) if n_kf is None else n_kf, ptr(cams),
                                   len(cams) if n_cam_rows is None else n_cam_rows, n_cam,
                                   ctypes.byref(prm) if prm is not None else None)


def _refused(tracker, pairs, rows, kfs, cams, code=LBA_E_ARG, **kw):
    p, r = pairs.copy(), rows.copy()
    assert _call(tracker, p, r, kfs, cams, **kw) == code
    assert p.tobytes() == pairs.tobytes() and r.tobytes() == rows.tobytes()      # nothing written


def test_refused_calls_write_nothing_and_the_next_call_succeeds(tracker):
    pairs, rows, kfs, cams, _ = make_tri_pairs(n_pairs=2, n_rows=20, seed=91)
    rows["status"], rows["stereo_point"], rows["X"] = 5, 5, 7.0
    pairs["n_new"] = pairs["n_stereo"] = -3

    def mod(arr, k, field, value):
        out = arr.copy()
        out[field][k] = value
        return out

    L = _bind()
    a = (ptr(pairs), 2, ptr(rows), len(rows), ptr(kfs), len(kfs), ptr(cams), len(cams), 4, None)
    assert L.lba_triangulate(None, *a) == LBA_E_ARG
    for null in (0, 2, 4, 6):
        b = list(a)
        b[null] = None
        assert L.lba_triangulate(tracker.h, *b) == LBA_E_ARG
    for neg in (1, 3, 5, 7):
        b = list(a)
        b[neg] = -1
        assert L.lba_triangulate(tracker.h, *b) == LBA_E_ARG
    _refused(tracker, pairs, rows, kfs, cams, n_cam=0)
    _refused(tracker, mod(pairs, 1, "kf1", -1), rows, kfs, cams)
    _refused(tracker, mod(pairs, 1, "kf2", 3), rows, kfs, cams)                 # three keyframes
    _refused(tracker, pairs, rows, kfs, cams, n_kf=2)
    _refused(tracker, mod(pairs, 1, "row0", -1), rows, kfs, cams)
    _refused(tracker, mod(pairs, 1, "n_rows", -1), rows, kfs, cams)
    _refused(tracker, mod(pairs, 1, "n_rows", 21), rows, kfs, cams)             # past the end of rows
    _refused(tracker, pairs, rows, kfs, cams, n_rows=39)
    _refused(tracker, pairs, rows, mod(kfs, 2, "cam0", -1), cams)
    _refused(tracker, pairs, rows, mod(kfs, 2, "cam0", 9), cams)                # 9 + 4 > 12 camera rows
    _refused(tracker, pairs, rows, kfs, cams, n_cam_rows=11)
    _refused(tracker, pairs, mod(rows, 39, "cam1", 4), kfs, cams)
    _refused(tracker, pairs, mod(rows, 39, "cam2", -1), kfs, cams)
    for bad in (0.0, -1.8, np.nan, np.inf):
        _refused(tracker, pairs, rows, kfs, cams, prm=LbaTriParams(bad, 0.0, 0, 0))
    # the limit of the header: more than 64 cameras per keyframe
    many = np.zeros(3 * (TRI_MAX_CAM + 1), TRI_CAM_DTYPE)
    far = kfs.copy()
    far["cam0"] = np.arange(3) * (TRI_MAX_CAM + 1)
    _refused(tracker, pairs, rows, far, many, n_cam=TRI_MAX_CAM + 1, code=LBA_E_LIMIT)
    # exactly 64 is accepted: the four cameras of every keyframe first, the last one (stereo) at index 63
    wide = np.zeros(3 * TRI_MAX_CAM, TRI_CAM_DTYPE)
    for k in range(3):
        wide[k * 64:(k + 1) * 64] = cams[4 * k + 3]
        wide[k * 64:k * 64 + 3] = cams[4 * k:4 * k + 3]
    wkf = kfs.copy()
    wkf["cam0"] = np.arange(3) * 64
    wrows = rows.copy()
    for f in ("cam1", "cam2"):
        wrows[f][wrows[f] == 3] = 63
    wp = pairs.copy()
    assert _call(tracker, wp, wrows, wkf, wide, n_cam=TRI_MAX_CAM, prm=tri_params(1.2)) == 0
    # the next valid call runs clean and gives what the 64-camera call gave
    p, r = tracker.triangulate(pairs.copy(), rows.copy(), kfs, cams, 4, tri_params(1.2))
    assert (p["n_new"] > 0).all() and (r["status"] >= 0).all() and (r["status"] <= 10).all()
    assert r["status"].tobytes() == wrows["status"].tobytes() and r["X"].tobytes() == wrows["X"].tobytes()
    assert p["n_new"].tobytes() == wp["n_new"].tobytes()
    assert (r["X"][r["status"] != TRI_OK] == 7.0).all()


def test_empty_calls(tracker):
    pairs, rows, kfs, cams, _ = make_tri_pairs(n_pairs=2, n_rows=20, seed=92)
    L = _bind()
    assert L.lba_triangulate(tracker.h, None, 0, None, 0, ptr(kfs), len(kfs), ptr(cams), len(cams), 4, None) == 0
    empty = pairs.copy()
    empty["n_rows"][1] = 0
    empty["n_new"] = empty["n_stereo"] = 5
    rows["status"] = 5
    p, r = tracker.triangulate(empty.copy(), rows.copy(), kfs, cams, 4, tri_params(1.2))
    assert p[1]["n_new"] == 0 and p[1]["n_stereo"] == 0 and p[0]["n_new"] > 0
    assert r[20:].tobytes() == rows[20:].tobytes() and (r["status"][:20] != 5).all()
    none = pairs.copy()
    none["n_rows"] = 0
    none["n_new"] = 5
    p, r = tracker.triangulate(none, rows.copy(), kfs, cams, 4, None)
    assert (p["n_new"] == 0).all() and r.tobytes() == rows.tobytes()
    assert ratio_factor(1.2) > 0
