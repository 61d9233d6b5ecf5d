"""CPU checks of amc_lba.fuse's packers, generator and caller-side helpers: the dtypes mirror the C structs' sizes, the
packed offsets address each target's own arrays, the generator is seeded, settled and has what it promises (occupied
features, duplicated points, points visible in two cameras of one keyframe, jobs that are accepted), and
distinctive_descriptor is ComputeDistinctiveDescriptors' choice."""
import numpy as np

import fuse_oracle as fo
from amc_lba.abi import FUSE_CAM_DTYPE, FUSE_ROW_DTYPE, FUSE_SEARCH_DTYPE, FUSE_TARGET_DTYPE
from amc_lba.fuse import (FUSE_KF, FUSE_OK, FUSE_SIM3, TH_KF, distinctive_descriptor, level_quotients, make_fuse_problem,
                          pack_searches, pack_targets, split_rows)
from amc_lba.match import GRID_CELLS, build_grid


def test_dtypes_have_the_abi_sizes():
    assert (FUSE_CAM_DTYPE.itemsize, FUSE_TARGET_DTYPE.itemsize, FUSE_SEARCH_DTYPE.itemsize,
            FUSE_ROW_DTYPE.itemsize) == (72, 48, 32, 32)


def test_pack_targets_addresses_each_targets_own_arrays():
    a = make_fuse_problem(n_kf=2, n_cam=3, n_feat=40, n_points=60, seed=1).targets
    b = make_fuse_problem(n_kf=1, n_cam=1, n_feat=25, n_points=60, seed=2, n_levels=5).targets
    targets = [a[0], b[0], a[1]]
    pk = pack_targets(targets)
    for T, t in zip(pk.T, targets):
        assert (T["n_cam"], T["n_feat"], T["n_levels"]) == (t.n_cam, len(t.feats), t.n_levels)
        assert pk.fcams[T["cam0"]:T["cam0"] + T["n_cam"]].tobytes() == t.fcams.tobytes()
        assert pk.gcams[T["cam0"]:T["cam0"] + T["n_cam"]].tobytes() == t.gcams.tobytes()
        assert pk.feats[T["feat0"]:T["feat0"] + T["n_feat"]].tobytes() == t.feats.tobytes()
        cs = pk.cell_start[T["cell0"]:T["cell0"] + t.n_cam * GRID_CELLS + 1]
        assert cs[0] == 0 and (cs == t.cell_start).all()
        assert (pk.cell_feat[T["cf0"]:T["cf0"] + cs[-1]] == t.cell_feat).all()
        assert (pk.sf[T["sf0"]:T["sf0"] + T["n_levels"]] == t.sf).all()
        assert (pk.sigma[T["sigma0"]:T["sigma0"] + T["n_levels"]] == t.sigma).all()
        assert (T["bf"], T["log_scale_factor"]) == (t.bf, t.log_scale_factor)
    S = pack_searches(pk.T, [(0, 0, 10, FUSE_KF, 3.0), (1, 0, 10, FUSE_SIM3, 4.0), (2, 4, 0, FUSE_KF, 3.0), (0, 2, 5, FUSE_KF, 3.0)])
    assert S["row0"].tolist() == [0, 30, 40, 40]
    rows = np.zeros(55, FUSE_ROW_DTYPE)
    assert [r.shape for r in split_rows(pk.T, S, rows)] == [(10, 3), (10, 1), (0, 3), (5, 3)]
    assert len(pack_targets([]).T) == 0


def test_generator_is_seeded_and_its_grid_is_build_grids():
    a, b = make_fuse_problem(seed=3, n_kf=3, n_points=150, n_feat=80), make_fuse_problem(seed=3, n_kf=3, n_points=150, n_feat=80)
    c = make_fuse_problem(seed=4, n_kf=3, n_points=150, n_feat=80)
    assert a.pos.tobytes() == b.pos.tobytes() and a.obs.tobytes() == b.obs.tobytes() and a.desc.tobytes() == b.desc.tobytes()
    assert a.targets[1].feats.tobytes() == b.targets[1].feats.tobytes() and a.pos.tobytes() != c.pos.tobytes()
    for t in a.targets:
        cs, cf = build_grid(t.feats, t.gcams)
        assert (cs == t.cell_start).all() and (cf == t.cell_feat).all()
        assert (t.feats["u_right"][t.feats["cam"] == t.n_cam - 1] >= 0).any()


def test_generator_has_what_it_promises():
    prob = make_fuse_problem(n_kf=6, n_cam=4, n_feat=150, n_points=300, seed=0)
    m = fo.ToyMap.from_problem(prob)
    n_points = 300
    assert prob.n_ids > n_points                                            # duplicated points
    dup = np.arange(n_points, prob.n_ids)
    assert sum(m.observations(int(i)) > 0 for i in dup) * 2 >= len(dup)          # and most of them are observed
    assert sum((m.mp[k] >= 0).sum() for k in m.mp) > 200                     # occupied features
    two = sum(1 for P in m.pts for o in P.obs.values() if sum(i != -1 for i in o) >= 2)
    assert two > 0                                                          # a point in two cameras of one keyframe
    P = prob.points(np.arange(prob.n_ids))
    rows, quot = fo.sequential(prob.targets[1], P, FUSE_KF, TH_KF)
    assert (rows["status"] == FUSE_OK).sum() > 50                           # jobs are accepted
    occ = m.mp[1][rows["feat"][rows["status"] == FUSE_OK]]
    assert (occ >= 0).any() and (occ < 0).any()                             # onto occupants and onto free features
    q = level_quotients(prob.max_distance, prob.pos, np.concatenate([t.fcams["ow"] for t in prob.targets]),
                        prob.targets[0].log_scale_factor)
    assert (np.abs(q - np.round(q)) > 1e-9).all()                           # settled against every camera centre
    assert np.nanmin(np.abs(quot - np.round(quot))) > 1e-9


def test_kf_points_and_points_follow_the_observations():
    prob = make_fuse_problem(n_kf=3, n_points=100, n_feat=60, seed=7)
    ids = prob.kf_points(1)
    for pid, k, f in prob.obs:
        if k == 1:
            assert ids[f] == pid
    P = prob.points(ids)
    assert (P["skip"] == (ids < 0)).all()
    has = ids >= 0
    assert (P["pos"][has] == prob.pos[ids[has]]).all() and (P["desc"][has] == prob.desc[ids[has]]).all()


def test_distinctive_descriptor_is_the_toy_maps_choice():
    rng = np.random.default_rng(5)
    for n in range(1, 8):
        descs = rng.integers(0, 2 ** 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
        descs[n // 2] = descs[0]                                            # a tie: the first wins
        feats = (np.zeros(n, np.int32), np.full(n, -1.0, np.float32), descs)
        m = fo.ToyMap(1, {k: (feats[0][k:k + 1], feats[1][k:k + 1], descs[k:k + 1]) for k in range(n)}, [descs[0] * 0])
        for k in range(n):
            m.add(0, k, 0)
        m.compute_distinctive_descriptors(0)
        assert m.pts[0].desc.tobytes() == descs[distinctive_descriptor(descs)].tobytes()
