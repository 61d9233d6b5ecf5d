"""amc_lba.sim3_project's three host helpers against direct restatements of the LoopClosing.cc lines they stand for:
points_from_keyframes (:554-572 / :778-794), matched_kf (ORBmatcher.cc:675-676) and scw_from_pair (:576-579)."""
import numpy as np

from amc_lba.sim3 import SIM3_PAIR_DTYPE
from amc_lba.sim3_project import matched_kf, points_from_keyframes, scw_from_pair


def test_points_from_keyframes_is_the_spmappoints_dedup():
    rng = np.random.default_rng(5)
    n_ids = 300
    bad = rng.random(n_ids) < 0.1
    kf_points = [rng.integers(-1, n_ids, rng.integers(0, 200)) for _ in range(11)]
    kf_points.append(np.zeros(0, np.int64))
    pts, kfs = points_from_keyframes(kf_points, bad)
    # the loop as written, on objects
    sp, vp, vk = set(), [], []
    for k, ids in enumerate(kf_points):
        for i in ids:
            if i < 0 or bad[i]:
                continue
            if i not in sp:
                sp.add(int(i))
                vp.append(int(i))
                vk.append(k)
    assert pts.tolist() == vp and kfs.tolist() == vk
    assert len(set(vp)) == len(vp) and not bad[pts].any()
    # a point seen by two keyframes stays with the first
    pts2, kfs2 = points_from_keyframes([[4, 7], [7, 9, -1]], np.zeros(10, bool))
    assert pts2.tolist() == [4, 7, 9] and kfs2.tolist() == [0, 0, 1]


def test_matched_kf_follows_the_matched_points():
    feat_point = np.array([-1, 2, 0, -1, 2])
    point_kf = np.array([5, 6, 7])
    assert matched_kf(feat_point, point_kf).tolist() == [-1, 7, 5, -1, 7]
    # the loop as written: vpMatchedKF[bestIdx] = pKFi at every acceptance, the last one staying
    rng = np.random.default_rng(1)
    n_feat, n_pts = 40, 25
    pkf = rng.integers(0, 6, n_pts)
    vm, vk = np.full(n_feat, -1), np.full(n_feat, -1)
    for p in range(n_pts):
        f = int(rng.integers(0, n_feat))
        vm[f], vk[f] = p, pkf[p]
    assert matched_kf(vm, pkf).tolist() == vk.tolist()


def _mat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_scw_from_pair_is_the_sim3_product():
    rng = np.random.default_rng(2)
    for _ in range(20):
        pair = np.zeros(1, SIM3_PAIR_DTYPE)[0]
        q1 = rng.normal(size=4)
        pair["q"], pair["t"], pair["s"] = q1 / np.linalg.norm(q1), rng.normal(size=3), rng.uniform(0.5, 2.0)
        q2 = rng.normal(size=4)
        q2 /= np.linalg.norm(q2)
        t2 = rng.normal(size=3)
        q, t, s = scw_from_pair(pair, q2, t2)
        assert q.dtype == np.float32 and t.dtype == np.float32
        # as 4 x 4 similarity matrices: [s R, t; 0, 1] products (g2o::Sim3::operator*)
        A, B = np.eye(4), np.eye(4)
        A[:3, :3], A[:3, 3] = pair["s"] * _mat(pair["q"]), pair["t"]
        B[:3, :3], B[:3, 3] = _mat(q2), t2
        Cm = A @ B
        assert np.allclose(float(s) * _mat(q.astype(float)), Cm[:3, :3], atol=2e-6)
        assert np.allclose(t, Cm[:3, 3], atol=2e-6) and abs(float(s) - pair["s"]) < 1e-6
        # a point: Scw x = Scm (Smw x)
        x = rng.normal(size=3)
        assert np.allclose(float(s) * _mat(q.astype(float)) @ x + t, (A @ B @ np.append(x, 1))[:3], atol=1e-5)
