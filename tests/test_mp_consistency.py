"""The restatement of MapPoint's refresh (tests/mp_oracle.py) against the forms the project already has: the
descriptor's choice equals amc_lba.fuse.distinctive_descriptor and ToyMap.compute_distinctive_descriptors on random
inputs, and for two observations the geometry equals amc_lba.triangulate.new_point_geometry bit for bit."""
import numpy as np
import pytest

import fuse_oracle as fo
import mp_cases as mc
import mp_oracle as mo
from amc_lba.fuse import distinctive_descriptor, make_fuse_problem
from amc_lba.mappoint import MP_DESC, MP_NORMAL, keyframes_from_targets, obs_from_map, pack_points
from amc_lba.triangulate import new_point_geometry

F = np.float32


@pytest.mark.parametrize("seed", range(6))
def test_descriptor_choice_equals_distinctive_descriptor(seed):
    rng = np.random.default_rng(seed)
    K = mc.big_world()
    for n in (1, 2, 3, 4, 5, 8, 17, 40, 70):
        L = mc.long_list(K, n, rng)
        near = rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)      # a cluster, so medians tie
        for o in L[::2]:
            K.feats["desc"][int(K.ekfs["feat0"][o["kf"]]) + int(o["feat"])] = near ^ np.uint32(1 << int(rng.integers(0, 3)))
        P, obs = mc.one(K, L, ops=MP_DESC)
        descs = np.stack([K.feature(o["kf"], o["feat"])["desc"] for o in L])
        for form in (mo.refresh_loops, mo.refresh_vec):
            R = form(P[0], obs, K)
            assert int(R["best_obs"]) == distinctive_descriptor(descs), (n, form.__name__)
            assert R["desc"].tolist() == descs[int(R["best_obs"])].tolist()


@pytest.mark.parametrize("seed", (0, 1))
def test_descriptor_equals_the_toy_maps(seed):
    prob = make_fuse_problem(n_kf=6, n_cam=4, n_feat=60, n_points=150, seed=seed)
    m = fo.ToyMap.from_problem(prob)
    K = keyframes_from_targets(prob.targets)
    ids = [i for i, p in enumerate(m.pts) if p.obs]
    P, obs = pack_points([obs_from_map(m.pts[i].obs) for i in ids], prob.pos[ids], 0, ops=MP_DESC)
    R = mo.refresh_batch(P, obs, K)
    assert (R["best_obs"] >= 0).all() and (R["n_obs"] > 1).sum() > 20
    for i, r in zip(ids, R):
        m.pts[i].desc = np.zeros(8, np.uint32)
        m.compute_distinctive_descriptors(i)
        assert r["desc"].tolist() == m.pts[i].desc.tolist(), i


def test_two_observations_equal_new_point_geometry_bitwise():
    rng = np.random.default_rng(9)
    K = mc.world(n_kf=10, seed=9)
    lists, pos, refs, want = [], [], [], []
    for _ in range(300):
        k1, k2 = rng.choice(10, 2, replace=False)
        L = mc.lst((int(k1), int(rng.integers(0, 4)), 0), (int(k2), int(rng.integers(0, 4)), 1))
        X = rng.normal(0, 5, 3).astype(F)
        f1 = K.feature(L[0]["kf"], L[0]["feat"])
        f2 = K.feature(L[1]["kf"], L[1]["feat"])
        want.append(new_point_geometry(X, K.centre(L[0]["kf"], f1["cam"]), K.centre(L[1]["kf"], f2["cam"]), f1["scale"],
                                       K.scale_top))
        lists.append(L); pos.append(X); refs.append(int(k1))
    P, obs = pack_points(lists, pos, refs, ops=MP_NORMAL)
    for form in (mo.refresh_loops, mo.refresh_vec):
        R = mo.refresh_batch(P, obs, K, form=form)
        for r, (normal, min_d, max_d) in zip(R, want):
            assert r["normal"].tobytes() == normal[0].tobytes()
            assert r["min_distance"].tobytes() == min_d[0].tobytes() and r["max_distance"].tobytes() == max_d[0].tobytes()
