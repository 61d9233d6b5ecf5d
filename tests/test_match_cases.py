"""The named cases of lba_match_project have their properties, and the two restatements of tests/match_oracle.py (the
reference's sequential loop and the round-based resolve) agree on every case and on 200 further generated frames, in
every output and, where defined, in the bound on `rounds`.  On the generated frames the order matters: at least 5 % of
the jobs end differently from the same job run alone against the entry `taken` state, so a device without the resolve
phase cannot pass tests/test_gpu_match.py."""
import numpy as np
import pytest

import match_cases as mc
import match_oracle as mo
from amc_lba.match import (GRID_CELLS, MATCH_OK, MATCH_ROT, build_grid, c_round,
                           jobs_last_frame, jobs_local_points, make_match_search, match_cams, match_params, pack_searches,
                           scale_factors)


@pytest.mark.parametrize("name,mode", mc.NAMES, ids=mc.IDS)
def test_case_has_its_property_and_the_restatements_agree(name, mode):
    s, p, seq, rnd, check, cands = mc.case(name, mode)
    check(s, seq, rnd, cands)
    assert seq.same_outputs(rnd)
    per_cam = np.bincount(s.jobs["cam"], minlength=s.n_cam)
    assert (rnd.rounds <= per_cam).all() and ((rnd.rounds > 0) == (per_cam > 0)).all()
    assert all(len(c) <= mo.capacity(s, k) for k, c in enumerate(cands))
    assert seq.n_matches == (seq.status == MATCH_OK).sum() and seq.n_matches_mono <= seq.n_matches + (seq.status == MATCH_ROT).sum()


def _order_matters(s, p, seq, cands):
    st, ft = mo.alone(s, p, cands)
    before_rot = np.where(seq.status == MATCH_ROT, MATCH_OK, seq.status)
    return ((st != before_rot) | ((ft != seq.feat) & (st == MATCH_OK))).mean()


@pytest.mark.parametrize("mode", mc.BOTH, ids=["ratio", "best"])
def test_generated_frames_restatements_agree_and_order_matters(mode):
    share = []
    for seed in range(200):
        s = make_match_search(mode=mode, n_cam=1 + seed % 4, n_feat=60 + seed % 50, n_points=80 + seed % 70, seed=1000 + seed)
        p = match_params(mode, s.n_cam)
        cands = mo.candidates(s, p)
        seq, rnd = mo.sequential(s, p, cands), mo.by_rounds(s, p, cands)
        assert seq.same_outputs(rnd), seed
        assert (rnd.rounds <= np.bincount(s.jobs["cam"], minlength=s.n_cam)).all()
        share.append(_order_matters(s, p, seq, cands))
    print(f"jobs that end differently alone: mean {np.mean(share):.3f}, min {np.min(share):.3f}")
    assert np.mean(share) >= 0.05
    s, p, seq, _, _, cands = mc.case("generated", mode)
    assert _order_matters(s, p, seq, cands) >= 0.05


@pytest.mark.parametrize("mode", mc.BOTH, ids=["ratio", "best"])
def test_batches_are_what_they_claim(mode):
    b = mc.batch(mode)
    assert len(b) == 40 and len({(s.n_cam, len(s.feats), len(s.jobs)) for s in b}) >= 30 and len(b[7].jobs) == 0
    S, cams, cs, cf, feats, jobs = pack_searches(b)
    assert S["n_jobs"].sum() == len(jobs) and S["cell0"][1] == b[0].n_cam * GRID_CELLS + 1
    assert sum(s.n_cam for s in mc.small_batch(mode)) > 256


def test_helpers():
    assert c_round(np.float32([0.5, 1.5, 2.5, -0.5, 10.49])).tolist() == [1, 2, 3, -1, 10]
    cams = match_cams(2)
    f = np.zeros(5, mc.MATCH_FEAT_DTYPE)
    f["x"], f["y"], f["cam"] = [5.0, 4.9, 639.9, 105.0, 5.0], [5.0, 5.0, 5.0, 105.0, 5.0], [0, 0, 0, 1, 1]
    cs, cf = build_grid(f, cams)
    assert cf.tolist() == [1, 0, 4, 3]           # 4.9 rounds into cell 0, 5.0 into cell 1; 639.9 rounds out of the grid
    assert cs[0] == 0 and cs[1] == 0 and cs[2] == 1 and cs[50] == 2 and cs[-1] == 4
    sf = scale_factors(8)
    j = jobs_local_points(np.array([[True, False], [True, True]]), np.ones((2, 2)), np.ones((2, 2)), np.zeros((2, 2)),
                          np.array([[2, 0], [0, 3]]), np.array([[0.999, 0.0], [0.9, 0.9]]), np.zeros((2, 8), np.uint32),
                          [1, 0], sf, th=3.0)
    assert j["cam"].tolist() == [0, 0, 1] and j["point"].tolist() == [0, 1, 1] and j["blocks"].tolist() == [1, 0, 0]
    assert j["radius"][0] == np.float32(2.5) * np.float32(3.0) * sf[2] and j["min_level"].tolist() == [1, -1, 2]
    Rcw, tcw = np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3))
    K, bounds = np.tile([320.0, 320.0, 320.0, 240.0], (2, 1)), np.tile([0.0, 640.0, 0.0, 480.0], (2, 1))
    j = jobs_last_frame([[0, 0, 2.0], [0, 0, -2.0], [5.0, 0, 2.0]], Rcw, tcw, K, bounds, [1, 1, 1], [0, 0, 0],
                        np.zeros((3, 8), np.uint32), [1, 1, 1], sf, 40.0, 15.0)
    assert j["point"].tolist() == [0, 0] and j["x"].tolist() == [320.0, 320.0] and j["ur"][0] == np.float32(300.0)
    assert j["radius"][0] == np.float32(15.0) * sf[1] and j["max_level"].tolist() == [2, 2]
