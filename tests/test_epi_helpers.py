"""The caller's side of lba_match_epipolar on plain arrays (amc_lba.epipolar), on the CPU: feat_vec_csr, epi_feats,
pack_epi_keyframes / epi_pairs, epi_matches, and the chain epi_matches -> tri_rows on a generated pair."""
import numpy as np

import epi_cases as ec
import epi_oracle as eo
from amc_lba.abi import EPI_ROW_DTYPE
from amc_lba.epipolar import (EPI_NO_MATCH, EPI_OK, EPI_ROT, epi_feats, epi_matches, epi_pairs, feat_vec_csr,
                              make_epi_pairs, pack_epi_keyframes)
from amc_lba.triangulate import scale_pyramid, tri_rows


def test_feat_vec_csr():
    nid, start, feat = feat_vec_csr([3, -1, 1, 3, 1, 7])
    assert nid.tolist() == [1, 3, 7] and start.tolist() == [0, 2, 4, 5] and feat.tolist() == [2, 4, 0, 3, 5]
    assert all(a.dtype == np.int32 for a in (nid, start, feat))
    nid, start, feat = feat_vec_csr([])
    assert nid.tolist() == [] and start.tolist() == [0] and feat.tolist() == []
    nid, start, feat = feat_vec_csr([-1, -1])
    assert nid.tolist() == [] and start.tolist() == [0] and feat.tolist() == []
    # keypoints ascend within a node, node ids ascend strictly
    rng = np.random.default_rng(1)
    nodes = rng.integers(-1, 9, 200)
    nid, start, feat = feat_vec_csr(nodes)
    assert (np.diff(nid) > 0).all() and start[0] == 0 and start[-1] == (nodes >= 0).sum() == len(feat)
    for k, n in enumerate(nid):
        l = feat[start[k]:start[k + 1]]
        assert (np.diff(l) > 0).all() and (nodes[l] == n).all() and len(l) == (nodes == n).sum()


def _kf():
    sf, sig2 = scale_pyramid(8)
    return {"key_to_cam": [0, 0, 1, 1], "keys_un": [[10.5, 20.25], [30, 40], [50, 60], [70, 80]], "keys": np.zeros((4, 2)),
            "octave": [0, 2, 1, 7], "global_to_local": [0, 1, 0, 1], "u_right": [45.5, -1.0], "depth": [3.0, 0.0],
            "level_sigma2": sig2, "scale_factors": sf, "angle": [1.0, 2.0, 3.0, 359.5], "has_point": [0, 1, 0, 0],
            "desc": np.arange(4 * 32, dtype=np.uint8).reshape(4, 32)}


def test_epi_feats():
    sf, sig2 = scale_pyramid(8)
    f = epi_feats(_kf())
    assert f["x"].tolist() == [10.5, 30, 50, 70] and f["y"].tolist() == [20.25, 40, 60, 80]
    assert f["cam"].tolist() == [0, 0, 1, 1] and f["has_point"].tolist() == [0, 1, 0, 0]
    assert f["angle"].tolist() == [1.0, 2.0, 3.0, 359.5]
    assert (f["scale"] == sf[[0, 2, 1, 7]]).all() and (f["sigma2"] == sig2[[0, 2, 1, 7]]).all()
    # mvuRight[mmpGlobalToLocalID[idx]] where that exists (the kernel asks for the last camera as well)
    assert f["u_right"].tolist() == [45.5, -1.0, 45.5, -1.0]
    assert f["desc"][1].tolist() == np.arange(32, 64, dtype=np.uint8).view(np.uint32).tolist()
    kf = _kf()
    kf["desc"] = kf["desc"].view(np.uint32)
    del kf["angle"], kf["has_point"]
    g = epi_feats(kf)
    assert (g["desc"] == f["desc"]).all() and (g["angle"] == 0).all() and (g["has_point"] == 0).all()


def test_pack_and_pairs():
    f = epi_feats(_kf())
    ekfs, feats, nid, nst, nf = pack_epi_keyframes([f, f[:0], f[:3]], [[5, 5, -1, 2], [], [9, 9, 9]])
    assert ekfs["feat0"].tolist() == [0, 4, 4] and ekfs["n_feat"].tolist() == [4, 0, 3]
    assert ekfs["node0"].tolist() == [0, 3, 4] and ekfs["n_node"].tolist() == [2, 0, 1] and ekfs["nf0"].tolist() == [0, 3, 3]
    assert nid.tolist() == [2, 5, -1, -1, 9, -1] and nst.tolist() == [0, 1, 3, 0, 0, 3] and nf.tolist() == [3, 0, 1, 0, 1, 2]
    assert len(feats) == 7
    pairs = epi_pairs([0, 2, 1], [2, 0, 0], ekfs)
    assert pairs["out0"].tolist() == [0, 4, 7] and pairs["kf1"].tolist() == [0, 2, 1] and pairs["kf2"].tolist() == [2, 0, 0]


def test_epi_matches():
    ekfs = np.zeros(2, pack_epi_keyframes([], [])[0].dtype)
    ekfs["n_feat"] = (5, 3)
    pairs = epi_pairs([0, 1], [1, 0], ekfs)
    out = np.zeros(8, EPI_ROW_DTYPE)
    out["status"] = [EPI_OK, EPI_NO_MATCH, EPI_ROT, EPI_OK, EPI_NO_MATCH, EPI_NO_MATCH, EPI_OK, EPI_NO_MATCH]
    out["idx2"] = [2, -1, 1, 0, -1, -1, 4, -1]
    assert epi_matches(pairs[0], out, ekfs).tolist() == [[0, 2], [3, 0]]          # LBA_EPI_ROT is no match
    assert epi_matches(pairs[1], out, ekfs).tolist() == [[1, 4]]
    out["status"] = EPI_NO_MATCH
    assert epi_matches(pairs[0], out, ekfs).shape == (0, 2)


def test_generator_is_seeded_and_well_formed():
    a, b = make_epi_pairs(2, 2, 20, 4, seed=3), make_epi_pairs(2, 2, 20, 4, seed=3)
    for x, y in zip(a[:8], b[:8]):
        assert x.tobytes() == y.tobytes()
    assert make_epi_pairs(2, 2, 20, 4, seed=4)[4].tobytes() != a[4].tobytes()
    pairs, kfs, ekfs, cams, feats, nid, nst, nf, truth = a
    assert len(kfs) == 3 and len(cams) == 6 and (ekfs["n_feat"] == 40).all() and len(feats) == 120
    assert pairs["kf1"].tolist() == [0, 0] and pairs["kf2"].tolist() == [1, 2] and pairs["out0"].tolist() == [0, 40]
    last = feats["cam"] == 1
    # mvuRight is indexed by the local id, so other cameras' keypoints find a value there too: the camera rule matters
    assert (feats["u_right"][last] >= 0).any() and (feats["u_right"][last] < 0).any() and (feats["u_right"][~last] >= 0).any()
    assert feats["has_point"].any()
    for p, partner in enumerate(truth["partner"]):      # partners mostly share a node
        seen = np.flatnonzero(partner >= 0)
        n1, n2 = truth["nodes"][0][seen], truth["nodes"][p + 1][partner[seen]]
        assert len(seen) > 10 and (n1 == n2).mean() > 0.8


def test_matches_feed_tri_rows():
    c, r64, _ = ec.case("generated_4x400")
    truth = make_epi_pairs(1, 4, 400, 40, 32)[8]
    out = np.zeros(len(r64[0].status), EPI_ROW_DTYPE)
    out["idx2"], out["dist"], out["status"] = r64[0].idx2, r64[0].dist, r64[0].status
    m = epi_matches(c.pairs[0], out, c.ekfs)
    assert m.shape == (r64[0].n_matches, 2) and (np.diff(m[:, 0]) > 0).all()
    # most matches are the true partners
    assert (truth["partner"][0][m[:, 0]] == m[:, 1]).mean() > 0.9
    kf1, kf2 = truth["kf"][0], truth["kf"][1]
    rows = tri_rows(m, kf1, kf2, 4)
    assert rows.shape == (len(m),)
    i1, i2 = (int(v) for v in m[len(m) // 2])
    r = rows[len(m) // 2]
    f1, f2 = c.feats[i1], c.feats[c.ekfs[1]["feat0"] + i2]
    assert (r["cam1"], r["cam2"]) == (f1["cam"], f2["cam"]) == (kf1["key_to_cam"][i1], kf2["key_to_cam"][i2])
    assert r["z1"].tolist() == [f1["x"], f1["y"]] and r["z2"].tolist() == [f2["x"], f2["y"]]
    assert (r["sigma2_1"], r["sigma2_2"], r["scale1"], r["scale2"]) == (f1["sigma2"], f2["sigma2"], f1["scale"], f2["scale"])
    # ur is the feature's u_right for the last camera and -1 elsewhere: the two stereo rules agree
    for side, f in ((1, f1), (2, f2)):
        assert (r[f"ur{side}"] >= 0) == eo.is_stereo(f, 4)
    st = np.array([eo.is_stereo(c.feats[i], 4) for i in m[:, 0]])
    assert ((rows["ur1"] >= 0) == st).all()
