"""The packers and the generator of amc_lba.mappoint: obs_from_map's order, pack_points' ranges, points_to_s3p's fields,
keyframes_from_targets against the targets it reads, and make_mp_problem's ranges, determinism and variety."""
import numpy as np
import pytest

from amc_lba.abi import MP_OBS_DTYPE, MP_POINT_DTYPE
from amc_lba.fuse import make_fuse_problem
from amc_lba.mappoint import (MP_MAX_OBS, keyframes_from_targets, make_mp_problem, obs_from_map, pack_points,
                              points_to_s3p, synthetic_keyframes)

F = np.float32


def test_obs_from_map_keeps_keyframe_order_and_cameras_ascending():
    m = {7: [-1, 4, -1, 9], 2: [3, -1, -1, -1], 5: [-1, -1, -1, -1], 9: [1, 2, 3, 4]}
    L = obs_from_map(m)
    assert L.dtype == MP_OBS_DTYPE and list(zip(L["kf"], L["feat"])) == [(2, 3), (7, 4), (7, 9), (9, 1), (9, 2), (9, 3), (9, 4)]
    L = obs_from_map(m, order=[9, 7, 11, 2], index={9: 0, 7: 1, 2: 2, 5: 3})
    assert list(zip(L["kf"], L["feat"])) == [(0, 1), (0, 2), (0, 3), (0, 4), (1, 4), (1, 9), (2, 3)]
    assert len(obs_from_map({})) == 0 and len(obs_from_map({1: [-1, -1]})) == 0


def test_pack_points_lays_the_lists_one_behind_the_other():
    a, b, c = obs_from_map({0: [1, 2]}), obs_from_map({}), obs_from_map({3: [-1, 5], 4: [6, -1]})
    P, obs = pack_points([a, b, c], [[1, 2, 3], [4, 5, 6], [7, 8, 9]], [0, -1, 4], ops=[3, 1, 2], bad=[0, 0, 1],
                         max_distance=[1.0, 2.0, 3.0])
    assert P.dtype == MP_POINT_DTYPE and P["obs0"].tolist() == [0, 2, 2] and P["n_obs"].tolist() == [2, 0, 2]
    assert obs["feat"].tolist() == [1, 2, 5, 6] and P["ref_kf"].tolist() == [0, -1, 4]
    assert P["ops"].tolist() == [3, 1, 2] and P["bad"].tolist() == [0, 0, 1] and P["max_distance"].tolist() == [1.0, 2.0, 3.0]
    P, obs = pack_points([], np.zeros((0, 3)), [])
    assert len(P) == 0 and len(obs) == 0


def test_points_to_s3p_applies_the_invariance_factors_in_float():
    P = np.zeros(3, MP_POINT_DTYPE)
    P["pos"], P["normal"] = [[1, 2, 3]] * 3, [[0, 0, 1]] * 3
    P["min_distance"], P["max_distance"] = F([0.3, 1.7, 2.9]), F([3.3, 7.1, 11.9])
    P["desc"], P["bad"] = np.arange(24).reshape(3, 8), [0, 1, 0]
    S = points_to_s3p(P)
    assert S["min_dist"].tobytes() == (F(0.8) * P["min_distance"]).astype(F).tobytes()
    assert S["max_dist"].tobytes() == (F(1.2) * P["max_distance"]).astype(F).tobytes()
    assert S["max_distance"].tobytes() == P["max_distance"].tobytes() and S["skip"].tolist() == [0, 1, 0]
    assert S["desc"].tolist() == P["desc"].tolist() and S["normal"].tolist() == P["normal"].tolist()
    assert points_to_s3p(P, skip=[1, 1, 1])["skip"].tolist() == [1, 1, 1]


def test_keyframes_from_targets_reads_the_targets():
    prob = make_fuse_problem(n_kf=3, n_cam=3, n_feat=20, n_points=40, seed=4)
    K = keyframes_from_targets(prob.targets)
    assert K.n_cam == 3 and K.scale_top == prob.targets[0].sf[-1] and K.kfs["cam0"].tolist() == [0, 3, 6]
    for k, t in enumerate(prob.targets):
        f = K.feats[int(K.ekfs["feat0"][k]):int(K.ekfs["feat0"][k]) + int(K.ekfs["n_feat"][k])]
        assert f["cam"].tolist() == t.feats["cam"].tolist() and f["desc"].tolist() == t.feats["desc"].tolist()
        assert f["scale"].tobytes() == t.sf[t.feats["octave"]].tobytes()
        for c in range(3):
            assert K.centre(k, c).tobytes() == t.fcams["ow"][c].tobytes()       # float -> double -> float is exact


@pytest.mark.parametrize("scene", ("fuse", "epipolar"))
def test_generated_problem_is_valid_and_deterministic(scene):
    a = make_mp_problem(3, scene=scene, n_kf=5, n_cam=3, n_feat=24, n_points=40, long_tracks=2, long_obs=(65, 90))
    b = make_mp_problem(3, scene=scene, n_kf=5, n_cam=3, n_feat=24, n_points=40, long_tracks=2, long_obs=(65, 90))
    assert a.points.tobytes() == b.points.tobytes() and a.obs.tobytes() == b.obs.tobytes()
    assert a.kf_bad.tobytes() == b.kf_bad.tobytes()
    P, obs, K = a.points, a.obs, a.K
    assert (obs["kf"] >= 0).all() and (obs["kf"] < len(K.kfs)).all()
    assert (obs["feat"] >= 0).all() and (obs["feat"] < K.ekfs["n_feat"][obs["kf"]]).all()
    assert (P["obs0"] >= 0).all() and (P["obs0"] + P["n_obs"] <= len(obs)).all() and P["n_obs"].max() <= MP_MAX_OBS
    assert (P["n_obs"] > 64).sum() == 2 and set(P["ops"].tolist()) <= {1, 2, 3}
    assert (P["ref_kf"] >= -1).all() and (P["ref_kf"] < len(K.kfs)).all()
    for p in P:                                   # keyframes in order, cameras ascending within a keyframe
        L = obs[int(p["obs0"]):int(p["obs0"]) + int(p["n_obs"])]
        if int(p["n_obs"]) <= 64:
            cam = K.feats["cam"][K.ekfs["feat0"][L["kf"]] + L["feat"]]
            key = L["kf"].astype(np.int64) * 64 + cam
            assert (np.diff(key) > 0).all()
    c = make_mp_problem(4, scene=scene, n_kf=5, n_cam=3, n_feat=24, n_points=40)
    assert c.points.tobytes() != a.points[:len(c.points)].tobytes()


def test_synthetic_keyframes_are_camera_major_with_float_centres():
    K = synthetic_keyframes(3, 4, 5, np.random.default_rng(0))
    assert len(K.feats) == 60 and K.feats["cam"][:20].tolist() == sorted(K.feats["cam"][:20].tolist())
    assert (K.cams["Ow"] == K.cams["Ow"].astype(F).astype(np.float64)).all()
    assert K.ekfs["feat0"].tolist() == [0, 20, 40] and K.ekfs["n_feat"].tolist() == [20, 20, 20]
