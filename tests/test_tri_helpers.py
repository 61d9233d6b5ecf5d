"""The caller's side of CreateNewMapPoints on plain arrays (amc_lba.triangulate): tri_rows, ratio_factor,
new_point_geometry, first_wins, and the synthetic generator's promises."""
import numpy as np

import tri_oracle as to
from amc_lba.abi import TRI_PAIR_DTYPE, TRI_ROW_DTYPE
from amc_lba.triangulate import (TRI_OK, TRI_STATUS_NAMES, first_wins, make_tri_pairs, new_point_geometry, ratio_factor,
                                 scale_pyramid, tri_params, tri_rows)


def _kf(rng, n_keys, n_cam, n_stereo):
    sf, sig2 = scale_pyramid(8)
    cam = rng.integers(0, n_cam, n_keys)
    local = np.full(n_keys, -1)
    last = np.flatnonzero(cam == n_cam - 1)
    local[last] = rng.permutation(len(last))
    u_right = np.where(rng.random(len(last)) < 0.5, -1.0, rng.uniform(0, 900, len(last))).astype(np.float32)
    return {"key_to_cam": cam, "keys_un": rng.uniform(0, 900, (n_keys, 2)), "keys": rng.uniform(0, 900, (n_keys, 2)),
            "octave": rng.integers(0, 8, n_keys), "global_to_local": local, "u_right": u_right,
            "depth": rng.uniform(1, 30, len(last)).astype(np.float32), "level_sigma2": sig2, "scale_factors": sf}


def test_tri_rows_follows_the_reference_row_by_row():
    rng = np.random.default_rng(1)
    kf1, kf2 = _kf(rng, 60, 4, 0), _kf(rng, 50, 4, 0)
    matches = np.stack([rng.integers(0, 60, 40), rng.integers(0, 50, 40)], axis=1)
    rows = tri_rows(matches, kf1, kf2, 4)
    assert rows.dtype == TRI_ROW_DTYPE and len(rows) == 40
    for r, (i1, i2) in zip(rows, matches):
        for side, kf, i in ((1, kf1, i1), (2, kf2, i2)):
            cam = kf["key_to_cam"][i]
            assert r[f"cam{side}"] == cam
            assert (r[f"z{side}"] == np.float32(kf["keys_un"][i])).all() and (r[f"k{side}"] == np.float32(kf["keys"][i])).all()
            ur = kf["u_right"][kf["global_to_local"][i]] if cam == 3 else -1.0     # only the LAST camera (:420, :428)
            assert r[f"ur{side}"] == ur
            if ur >= 0:
                assert r[f"depth{side}"] == kf["depth"][kf["global_to_local"][i]]
            assert r[f"sigma2_{side}"] == kf["level_sigma2"][kf["octave"][i]]
            assert r[f"scale{side}"] == kf["scale_factors"][kf["octave"][i]]
    assert (rows["ur1"][kf1["key_to_cam"][matches[:, 0]] != 3] == -1.0).all()
    assert not rows["status"].any() and not rows["X"].any()
    assert len(tri_rows(np.zeros((0, 2), int), kf1, kf2, 4)) == 0


def test_ratio_factor_is_the_float_product():
    assert ratio_factor(1.2) == float(np.float32(1.5) * np.float32(1.2))
    assert ratio_factor(1.2) != 1.5 * 1.2 and abs(ratio_factor(1.2) - 1.8) < 1e-6
    assert ratio_factor(2.0) == 3.0
    p = tri_params(1.2, far_points=True, th_far=20.0)
    assert p.ratio_factor == ratio_factor(1.2) and p.far_points == 1 and p.th_far == 20.0


def test_new_point_geometry():
    rng = np.random.default_rng(2)
    X = rng.normal(0, 5, (20, 3)).astype(np.float32)
    O1, O2 = rng.normal(0, 1, (20, 3)).astype(np.float32), rng.normal(0, 1, (20, 3)).astype(np.float32)
    sf, _ = scale_pyramid(8)
    s1 = sf[rng.integers(0, 8, 20)]
    normal, dmin, dmax = new_point_geometry(X, O1, O2, s1, sf[-1])
    assert normal.dtype == dmin.dtype == dmax.dtype == np.float32
    for i in range(20):
        n1, n2 = X[i] - O1[i], X[i] - O2[i]
        want = (n1 / np.linalg.norm(n1) + n2 / np.linalg.norm(n2)) / 2
        assert np.abs(normal[i] - want).max() < 1e-6
        d = np.linalg.norm(n1.astype(np.float64))
        assert abs(dmax[i] - d * s1[i]) <= 4e-7 * dmax[i] and abs(dmin[i] - d * s1[i] / sf[-1]) <= 4e-7 * dmin[i]
    # the order of the two observations does not matter to the normal; the reference keyframe is KF1
    n_swapped, _, dmax_swapped = new_point_geometry(X, O2, O1, s1, sf[-1])
    assert (n_swapped == normal).all() and not (dmax_swapped == dmax).all()
    one = new_point_geometry(X[0], O1[0], O2[0], s1[0], sf[-1])
    assert one[0].shape == (1, 3) and one[1][0] == dmin[0]


def test_first_wins_keeps_the_first_accepted_row_per_keypoint():
    pairs = np.zeros(2, TRI_PAIR_DTYPE)
    pairs["kf1"], pairs["kf2"], pairs["row0"], pairs["n_rows"] = 0, (1, 2), (0, 4), (4, 4)
    rows = np.zeros(8, TRI_ROW_DTYPE)
    rows["status"] = [0, 1, 0, 0, 0, 0, 0, 6]
    idx1 = np.array([5, 6, 7, 5, 5, 6, 8, 9])     # keypoints of the current keyframe
    idx2 = np.array([1, 2, 3, 4, 1, 2, 2, 3])     # keypoints of either neighbour
    keep = first_wins(pairs, rows, idx1, idx2)
    # row 3: keypoint 5 of KF0 already taken by row 0; row 4 likewise (another neighbour, same keypoint of KF0);
    # row 5: keypoint 6 is free because row 1 was refused; row 6: keypoint 2 of KF2 taken by row 5; 1, 7 not accepted
    assert keep.tolist() == [True, False, True, False, False, True, False, False]
    # the same keypoint index in two different neighbours is two keypoints
    rows["status"] = 0
    keep = first_wins(pairs, rows, np.arange(8), np.array([0, 1, 2, 3, 0, 1, 2, 3]))
    assert keep.all()
    assert first_wins(pairs[:0], rows, idx1, idx2).sum() == 0
    assert TRI_OK == 0 and len(TRI_STATUS_NAMES) == 11


def test_generator_keeps_a_third_through_the_parallax_gate():
    pairs, rows, kfs, cams, truth = make_tri_pairs(n_pairs=4, n_rows=100, seed=3)
    assert len(kfs) == 5 and (pairs["kf1"] == 0).all() and len(cams) == 20
    r = to.run(pairs, rows, kfs, cams, 4, ratio_factor(1.2))
    assert (r.status != to.PARALLAX).mean() >= 1 / 3
    assert (r.status == to.OK).mean() >= 1 / 3
    ok = (r.status == to.OK) & ~truth["gross"]
    assert np.median(np.linalg.norm(r.X[ok] - truth["X"][ok], axis=1)) < 1.0
    # float-valued, last camera stereo only
    for f in ("z1", "z2", "k1", "k2", "ur1", "depth1", "sigma2_1", "scale2"):
        assert (rows[f] == rows[f].astype(np.float32)).all()
    assert (rows["ur1"][rows["cam1"] != 3] == -1).all() and (rows["ur1"][rows["cam1"] == 3] >= 0).any()
    own, _, k2, _, _ = make_tri_pairs(n_pairs=3, n_rows=5, seed=3, shared_current=False)
    assert len(k2) == 6 and own["kf1"].tolist() == [0, 2, 4]
