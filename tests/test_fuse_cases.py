"""CPU checks of lba_match_fuse's cases and of its two numpy restatements (tests/fuse_oracle.py): each named case has the
property it is named for; the loop as written and the vectorised route agree on every case and on 200 further seeds;
every named case and every GPU seed is settled (PredictScale's quotient keeps M_LEVEL from an integer, the bound
tests/test_s3p_cases.py demands for the same function; nothing else is decided by a rounding); and each mistake a device
could make (ties to the last, no error gates, the matrix-form rotation, IsInKFCamera applied up front) changes a counted
number of rows."""
import numpy as np
import pytest

import fuse_cases as fc
import fuse_oracle as fo
from amc_lba.fuse import FUSE_KF, FUSE_NO_CAMERA, FUSE_OK, FUSE_SIM3, FUSE_TOO_FAR, make_fuse_problem

F = np.float32


def restate(c, mode):
    return [fo.sequential(c.targets[t], c.points[p0:p0 + n], mode, fc.TH[mode]) for t, p0, n in c.searches]


@pytest.mark.parametrize("mode", fc.MODES, ids=("kf", "sim3"))
@pytest.mark.parametrize("name", fc.NAMES)
def test_case_has_its_property_and_both_routes_agree(name, mode):
    c = fc.case(name)
    seq = restate(c, mode)
    for (t, p0, n), (rows, _) in zip(c.searches, seq):
        assert fo.same_rows(rows, fo.vectorised(c.targets[t], c.points[p0:p0 + n], mode, fc.TH[mode]))
        assert rows.shape == (n, c.targets[t].n_cam)
        if mode == FUSE_SIM3:
            assert (rows["status"][:, -1] == FUSE_NO_CAMERA).all() and (rows["status"][:, :-1] != FUSE_NO_CAMERA).all()
        else:
            assert (rows["status"] != FUSE_NO_CAMERA).all()
        assert ((rows["feat"] >= 0) == np.isin(rows["status"], (FUSE_OK, FUSE_TOO_FAR)) & (rows["best_dist"] <
                (256 if mode == FUSE_KF else 257))).all()
    exp = c.expect.get(mode, {})
    flat = {k: np.concatenate([r[k].ravel() for r, _ in seq]) if seq else np.zeros(0) for k in fo.FUSE_ROW_DTYPE.names}
    if "status" in exp:
        assert fc.names(flat["status"]) == exp["status"]
    for key in ("feat", "best_dist", "level", "n_cand"):
        if key in exp:
            assert flat[key].tolist() == exp[key], key
    if "n_ok" in exp:
        assert [int((r["status"] == FUSE_OK).sum()) for r, _ in seq] == exp["n_ok"]


def test_z_zero_projects_to_infinity_and_is_out_of_image():
    rows, _ = restate(fc.case("gates"), FUSE_KF)[0]
    assert np.isinf(rows["x"][1, 0]) and fc.names(rows["status"][1]) == ["OUT_OF_IMAGE"] * 2


@pytest.mark.parametrize("seed", range(200))
def test_both_routes_agree_on_further_seeds(seed):
    prob = make_fuse_problem(n_kf=2, n_cam=1 + seed % 4, n_feat=60, n_points=80, seed=1000 + seed)
    mode = fc.MODES[(seed // 4) % 2]
    P = prob.points(np.arange(prob.n_ids))
    rows, _ = fo.sequential(prob.targets[1], P, mode, fc.TH[mode])
    assert fo.same_rows(rows, fo.vectorised(prob.targets[1], P, mode, fc.TH[mode]))


def test_every_named_case_and_gpu_seed_is_settled():
    for name in fc.NAMES:
        for mode in fc.MODES:
            for _, quot in restate(fc.case(name), mode):
                assert fc.level_settled(quot), name
    for seed in fc.GPU_SEEDS:
        prob = fc.gpu_problem(seed)
        P = prob.points(np.arange(prob.n_ids))
        for tg in prob.targets:
            assert fc.level_settled(fo.sequential(tg, P, FUSE_KF, fc.TH[FUSE_KF])[1]), seed


def test_each_mistake_changes_a_counted_number_of_rows():
    """a device with ties to the last, without the error gates or with the matrix-form rotation would fail the GPU
    test: on the named cases and the first GPU seed each changes this many rows (status, feat, best_dist, or the bits
    of x, y for the rotation).  IsInKFCamera applied up front: the rows of (point, camera) pairs the initial map
    observes; tests/test_fuse_walk.py counts those of them the walk goes on to use."""
    counts = dict(ties_last=0, no_error_gate=0, matrix_rotation=0)
    xy_bits = 0
    problems = [(c.targets[t], c.points[p0:p0 + n]) for c in map(fc.case, fc.NAMES) for t, p0, n in c.searches]
    prob = fc.gpu_problem(0)
    P = prob.points(np.arange(prob.n_ids))
    problems += [(tg, P) for tg in prob.targets[:4]]
    for tg, pts in problems:
        ref, _ = fo.sequential(tg, pts, FUSE_KF, fc.TH[FUSE_KF])
        for v in counts:
            got, _ = fo.sequential(tg, pts, FUSE_KF, fc.TH[FUSE_KF], variant=v)
            counts[v] += fo.diff_rows(ref, got)
            if v == "matrix_rotation":
                xy_bits += int(((ref["x"].view(np.uint32) != got["x"].view(np.uint32)) |
                                (ref["y"].view(np.uint32) != got["y"].view(np.uint32))).sum())
    m = fo.ToyMap.from_problem(prob)
    in_kf = sum(int(m.in_camera(int(pid), 1, c)) for pid in range(prob.n_ids) for c in range(4))
    print("rows changed by each mistake:", counts, "rows whose x or y bits the matrix rotation changes:", xy_bits,
          "rows of keyframe 1 an up-front IsInKFCamera would drop:", in_kf)
    assert counts["ties_last"] > 0 and counts["no_error_gate"] > 0 and xy_bits > 0 and in_kf > 0
