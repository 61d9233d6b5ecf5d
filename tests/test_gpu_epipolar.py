"""lba_match_epipolar on the GPU: the named cases (tests/epi_cases.py) against the fp64 restatement
(tests/epi_oracle.py: `sequential`), and, without an oracle, bitwise: a batch against each pair alone, two runs, a fresh
tracker against one that ran lba_triangulate before; refused calls write nothing and leave a message.

Against the restatement, on settled jobs (every fp64 comparison of every eligible candidate further than 1e-9 relative
from its gate): idx2, dist and status identical; n_matches identical where all jobs of the pair are settled.  Outputs
are pre-filled with junk, so every row must be written; inputs come back as passed."""
import ctypes

import numpy as np
import pytest

import epi_cases as ec
import epi_oracle as eo
from amc_lba.abi import EPI_ROW_DTYPE, LBA_E_ARG, LBA_E_LIMIT, TRI_CAM_DTYPE, ptr
from amc_lba.epipolar import (EPI_MAX_CAM, EPI_NO_NODE, LbaEpiParams, _bind, epi_matches, epi_params, make_epi_pairs)
from amc_lba.track import Tracker, track_config
from amc_lba.triangulate import tri_params, tri_rows

pytestmark = pytest.mark.gpu

JUNK = -77


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
    out = np.full(n_out + 3, JUNK, np.int32).repeat(4).view(EPI_ROW_DTYPE)
    ins = [a.copy() for a in (c.kfs, c.ekfs, c.cams, c.feats, c.node_id, c.node_start, c.node_feat)]
    p = epi_params(**dict(eo.PRM, **(c.prm if prm is None else prm)))
    pairs, out = tracker.match_epipolar(pairs, *ins[:3], c.n_cam, *ins[3:], p, out=out)
    for a, b in zip(ins, (c.kfs, c.ekfs, c.cams, c.feats, c.node_id, c.node_start, c.node_feat)):
        assert a.tobytes() == b.tobytes()
    for f in ("kf1", "kf2", "out0"):
        assert (pairs[f] == c.pairs[f]).all()
    assert (out[n_out:].view(np.int32) == JUNK).all()       # nothing behind the last pair's rows
    return pairs, out[:n_out]


def results(c, pairs, out):
    res = []
    for P in pairs:
        r = out[int(P["out0"]):int(P["out0"]) + int(c.ekfs[P["kf1"]]["n_feat"])]
        res.append(eo.Result(r["idx2"].astype(np.int64), r["dist"].astype(np.int64), r["status"].astype(np.int64), int(P["n_matches"])))
    return res


def compare(c, res, r64, st, label):
    all_settled = True
    for p, (r, w, s) in enumerate(zip(res, r64, st)):
        assert ((r.status >= 0) & (r.status <= 5)).all(), (label, p, "a row was not written")
        for f in ("idx2", "dist", "status"):
            assert (getattr(r, f)[s] == getattr(w, f)[s]).all(), (label, p, f, np.flatnonzero(s & (getattr(r, f) != getattr(w, f))))
        assert (r.n_matches == (r.status == eo.OK).sum())
        if s.all():
            assert r.n_matches == w.n_matches, (label, p)
        all_settled &= bool(s.all())
    return all_settled


@pytest.mark.parametrize("name", ec.NAMES)
def test_case_matches_restatement(tracker, name):
    c, r64, st = ec.case(name)
    pairs, out = device(tracker, c)
    res = results(c, pairs, out)
    n, bad = sum(len(s) for s in st), sum(int((~s).sum()) for s in st)
    print(f"{name}: {bad} of {n} jobs unsettled; device statuses {np.bincount(out['status'], minlength=6)}; "
          f"n_matches {pairs['n_matches'][:4].tolist()}")
    if compare(c, res, r64, st, name):
        c.prop(c, res)


@pytest.mark.parametrize("prm", [dict(only_stereo=1), dict(coarse=1), dict(check_orientation=1), dict(th_low=30),
                                 dict(only_stereo=1, coarse=1, check_orientation=1)], ids=lambda d: "+".join(d))
def test_flags_on_generated_pairs(tracker, prm):
    c = ec.generated(2, 3, 80, 8, 77, prm=prm)
    jobs = eo.jobs_of(c)
    r64, st = [eo.sequential(j) for j in jobs], [eo.settled(j) for j in jobs]
    pairs, out = device(tracker, c)
    compare(c, results(c, pairs, out), r64, st, str(prm))
    assert sum(r.n_matches for r in r64) > 0


def _batch(n_pairs=60):
    """`n_pairs` pairs over four generated sets of keyframes, each set behind the other, KF1 of a set in all its pairs"""
    sets = [make_epi_pairs(n_pairs // 4, 2, 130, 50, seed=40 + k) for k in range(4)]
    pairs, kfs, ekfs, cams, feats, nid, nst, nf = ([] for _ in range(8))
    at = dict(kf=0, cam=0, feat=0, row=0, nf=0, out=0)
    for P, K, E, C, F, I, S, N, _ in sets:
        P, K, E = P.copy(), K.copy(), E.copy()
        P["kf1"] += at["kf"]; P["kf2"] += at["kf"]; P["out0"] += at["out"]
        K["cam0"] += at["cam"]
        E["feat0"] += at["feat"]; E["node0"] += at["row"]; E["nf0"] += at["nf"]
        for lst, a in zip((pairs, kfs, ekfs, cams, feats, nid, nst, nf), (P, K, E, C, F, I, S, N)):
            lst.append(a)
        at = dict(kf=at["kf"] + len(K), cam=at["cam"] + len(C), feat=at["feat"] + len(F), row=at["row"] + len(I),
                  nf=at["nf"] + len(N), out=at["out"] + int(E["n_feat"][0]) * len(P))
    cat = [np.concatenate(a) for a in (pairs, kfs, ekfs, cams, feats, nid, nst, nf)]
    return ec.Case(*cat[:4], 2, *cat[4:], {}, None), sets


def test_batch_equals_each_pair_alone(tracker):
    c, sets = _batch()
    bp, bo = device(tracker, c)
    assert (bp["n_matches"] > 0).all() and (bo["status"] == EPI_NO_NODE).any()
    per = len(c.pairs) // 4
    for k in (0, 7, per, 2 * per + 3, len(c.pairs) - 1):
        P, K, E, C, F, I, S, N, _ = sets[k // per]
        one = ec.Case(P[k % per:k % per + 1].copy(), K, E, C, 2, F, I, S, N, {}, None)
        one.pairs["out0"] = 0
        sp, so = device(tracker, one)
        n1 = int(E["n_feat"][0])
        assert so.tobytes() == bo[int(bp[k]["out0"]):int(bp[k]["out0"]) + n1].tobytes(), k
        assert sp[0]["n_matches"] == bp[k]["n_matches"]


def test_two_runs_fresh_tracker_and_other_calls_between(tracker):
    from amc_lba.triangulate import make_tri_pairs
    c, _, _ = ec.case("kf1_in_20_pairs")
    other = Tracker(track_config())
    fresh = device(other, c)
    other.close()
    first = device(tracker, c)
    again = device(tracker, c)
    tp, tr, tk, tcams, _ = make_tri_pairs(n_pairs=2, n_rows=40, seed=5)
    tracker.triangulate(tp, tr, tk, tcams, 4, tri_params(1.2))
    after = device(tracker, c)
    for res in (again, after, fresh):
        assert res[0].tobytes() == first[0].tobytes() and res[1].tobytes() == first[1].tobytes()


def test_default_parameters_and_profile(tracker):
    c, _, _ = ec.case("generated_4x400")
    a = tracker.match_epipolar(c.pairs.copy(), c.kfs, c.ekfs, c.cams, c.n_cam, c.feats, c.node_id, c.node_start, c.node_feat, None)
    b = tracker.match_epipolar(c.pairs.copy(), c.kfs, c.ekfs, c.cams, c.n_cam, c.feats, c.node_id, c.node_start, c.node_feat,
                               LbaEpiParams(50, 0, 0, 0))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    tracker.match_epipolar_kernel_ms(True)
    device(tracker, c)
    ms = tracker.match_epipolar_kernel_ms(False)
    print(f"generated_4x400: k_epi_tables {ms[0] * 1e3:.1f} us, k_epi_match {ms[1] * 1e3:.1f} us")
    assert len(ms) == 2 and all(0.0 < m < 1000.0 for m in ms)


def test_matches_chain_into_triangulate(tracker):
    """match -> rows -> triangulate on the tracker handle, with the same keyframe and camera records"""
    pairs, kfs, ekfs, cams, feats, nid, nst, nf, truth = make_epi_pairs(2, 4, 150, 30, seed=9)
    pairs, out = tracker.match_epipolar(pairs, kfs, ekfs, cams, 4, feats, nid, nst, nf)
    from amc_lba.abi import TRI_PAIR_DTYPE
    tp, rows = np.zeros(len(pairs), TRI_PAIR_DTYPE), []
    for p, P in enumerate(pairs):
        m = epi_matches(P, out, ekfs)
        assert len(m) == P["n_matches"] > 0
        tp[p]["kf1"], tp[p]["kf2"], tp[p]["row0"], tp[p]["n_rows"] = P["kf1"], P["kf2"], sum(len(r) for r in rows), len(m)
        rows.append(tri_rows(m, truth["kf"][P["kf1"]], truth["kf"][P["kf2"]], 4))
    tp, tr = tracker.triangulate(tp, np.concatenate(rows), kfs, cams, 4, tri_params(1.2))
    assert (tp["n_new"] > 0).all() and (tp["n_new"] <= tp["n_rows"]).all()


def _args(tracker, c, p_arr, o_arr, **over):
    a = dict(pairs=ptr(p_arr), n_pairs=len(p_arr), out=ptr(o_arr), n_out=len(o_arr), kfs=ptr(c.kfs), ekfs=ptr(c.ekfs),
             n_kf=len(c.kfs), cams=ptr(c.cams), n_cam_rows=len(c.cams), n_cam=c.n_cam, feats=ptr(c.feats),
             n_feats=len(c.feats), node_id=ptr(c.node_id), node_start=ptr(c.node_start), n_node_rows=len(c.node_id),
             node_feat=ptr(c.node_feat), n_node_feat=len(c.node_feat), prm=None)
    a.update(over)
    return [tracker.h] + list(a.values())


def _refused(tracker, c, code=LBA_E_ARG, **over):
    """the call with some arguments or arrays replaced is refused, writes nothing and leaves a message"""
    repl = {k: np.ascontiguousarray(v) for k, v in over.items() if isinstance(v, np.ndarray)}
    c2 = c._replace(**{k: v for k, v in repl.items() if k in c._fields})
    pairs, out = c2.pairs.copy(), np.full(len(c.feats) * 4, JUNK, np.int32).view(EPI_ROW_DTYPE)
    pairs["n_matches"] = JUNK
    before = pairs.copy()
    raw = {k: v for k, v in over.items() if not isinstance(v, np.ndarray)}
    rc = _bind().lba_match_epipolar(*_args(tracker, c2, pairs, out, **raw))
    assert rc == code, (over.keys(), rc)
    assert pairs.tobytes() == before.tobytes() and (out.view(np.int32) == JUNK).all()
    assert len(tracker.last_error()) > 0


def _mod(arr, k, field, value):
    out = arr.copy()
    if field is None:
        out[k] = value
    else:
        out[field][k] = value
    return out


def test_refused_calls_write_nothing_and_the_next_call_succeeds(tracker):
    c, r64, st = ec.case("kf1_in_20_pairs")
    L = _bind()
    pairs, out = c.pairs.copy(), np.zeros(len(c.feats), EPI_ROW_DTYPE)
    assert L.lba_match_epipolar(None, *_args(tracker, c, pairs, out)[1:]) == LBA_E_ARG
    for null in ("pairs", "out", "kfs", "ekfs", "cams", "feats", "node_id", "node_start", "node_feat"):
        _refused(tracker, c, **{null: None})
    for neg in ("n_pairs", "n_out", "n_kf", "n_cam_rows", "n_feats", "n_node_rows", "n_node_feat"):
        _refused(tracker, c, **{neg: -1})
    _refused(tracker, c, n_cam=0)
    _refused(tracker, c, pairs=_mod(c.pairs, 1, "kf1", -1))
    _refused(tracker, c, pairs=_mod(c.pairs, 1, "kf2", len(c.kfs)))
    _refused(tracker, c, n_kf=len(c.kfs) - 1)
    _refused(tracker, c, pairs=_mod(c.pairs, 1, "out0", -1))
    _refused(tracker, c, pairs=_mod(c.pairs, 3, "out0", c.pairs["out0"][2] + 1))           # overlaps its neighbour
    _refused(tracker, c, n_out=int(c.pairs["out0"][-1]) + int(c.ekfs["n_feat"][0]) - 1)     # the last range is cut short
    _refused(tracker, c, kfs=_mod(c.kfs, 2, "cam0", -1))
    _refused(tracker, c, kfs=_mod(c.kfs, 2, "cam0", len(c.cams) - 1))
    _refused(tracker, c, n_cam_rows=len(c.cams) - 1)
    _refused(tracker, c, ekfs=_mod(c.ekfs, 1, "feat0", -1))
    _refused(tracker, c, ekfs=_mod(c.ekfs, 20, "n_feat", c.ekfs["n_feat"][20] + 1))
    _refused(tracker, c, n_feats=len(c.feats) - 1)
    _refused(tracker, c, ekfs=_mod(c.ekfs, 20, "n_node", c.ekfs["n_node"][20] + 1))         # past node_id / node_start
    _refused(tracker, c, ekfs=_mod(c.ekfs, 1, "node0", -1))
    _refused(tracker, c, ekfs=_mod(c.ekfs, 20, "nf0", c.ekfs["nf0"][20] + 1))               # past node_feat
    n0 = int(c.ekfs["node0"][3])
    _refused(tracker, c, node_id=_mod(c.node_id, n0 + 1, None, c.node_id[n0]))              # not strictly ascending
    _refused(tracker, c, node_start=_mod(c.node_start, n0, None, 1))                        # does not start at 0
    _refused(tracker, c, node_start=_mod(c.node_start, n0 + 1, None, c.node_start[n0 + 2] + 1))    # decreases behind it
    f0 = int(c.ekfs["nf0"][3])
    _refused(tracker, c, node_feat=_mod(c.node_feat, f0, None, -1))
    _refused(tracker, c, node_feat=_mod(c.node_feat, f0, None, c.ekfs["n_feat"][3]))
    _refused(tracker, c, node_feat=_mod(c.node_feat, f0, None, c.node_feat[f0 + 1]))        # listed twice
    _refused(tracker, c, feats=_mod(c.feats, 5, "cam", c.n_cam))
    _refused(tracker, c, feats=_mod(c.feats, 5, "cam", -1))
    for th in (-1, 256):
        prm = LbaEpiParams(th, 0, 0, 0)
        _refused(tracker, c, prm=ctypes.byref(prm))
    # the limit of the header: more than 64 cameras per keyframe
    many = np.zeros(len(c.kfs) * (EPI_MAX_CAM + 1), TRI_CAM_DTYPE)
    far = c.kfs.copy()
    far["cam0"] = np.arange(len(c.kfs)) * (EPI_MAX_CAM + 1)
    _refused(tracker, c, code=LBA_E_LIMIT, kfs=far, cams=many, n_cam=EPI_MAX_CAM + 1, n_cam_rows=len(many))
    # exactly 64 is accepted: the two cameras of every keyframe first and last, the stereo one at index 63
    wide = np.zeros(len(c.kfs) * EPI_MAX_CAM, TRI_CAM_DTYPE)
    for k in range(len(c.kfs)):
        wide[k * 64:(k + 1) * 64] = c.cams[2 * k + 1]
        wide[k * 64] = c.cams[2 * k]
    wkf = c.kfs.copy()
    wkf["cam0"] = np.arange(len(c.kfs)) * 64
    wf = c.feats.copy()
    wf["cam"][wf["cam"] == 1] = 63
    wp, wo = device(tracker, c._replace(kfs=wkf, cams=wide, feats=wf, n_cam=EPI_MAX_CAM))
    # the next valid call runs clean and gives what the restatement and the 64-camera call give
    p, o = device(tracker, c)
    compare(c, results(c, p, o), r64, st, "after the refusals")
    assert o.tobytes() == wo.tobytes() and p.tobytes() == wp.tobytes()


def test_empty_calls(tracker):
    c, _, _ = ec.case("kf1_in_20_pairs")
    L = _bind()
    none = np.zeros(0, c.pairs.dtype)
    assert L.lba_match_epipolar(*_args(tracker, c, none, np.zeros(0, EPI_ROW_DTYPE), pairs=None, out=None)) == 0
    # keyframes without features, without nodes, and a pair of a keyframe with itself
    e = c.ekfs.copy()
    e["n_feat"][1], e["n_node"][1], e["n_node"][2] = 0, 0, 0
    pairs = c.pairs[:4].copy()
    pairs["kf1"], pairs["kf2"] = (0, 1, 0, 3), (1, 0, 2, 3)
    pairs["out0"] = (0, 80, 80, 160)
    c2 = c._replace(ekfs=e, pairs=pairs)
    p, o = device(tracker, c2)
    assert p["n_matches"].tolist()[:3] == [0, 0, 0]
    assert (o["status"][:80] == EPI_NO_NODE).all() and (o["status"][80:160] == EPI_NO_NODE).all()
    r = eo.sequential(eo.jobs_of(c2)[3])
    s = eo.settled(eo.jobs_of(c2)[3])
    assert (o["idx2"][160:][s] == r.idx2[s]).all() and (o["status"][160:][s] == r.status[s]).all()
    assert p["n_matches"][3] == (o["status"][160:] == eo.OK).sum()
