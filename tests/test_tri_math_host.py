"""The product's CreateNewMapPoints maths (amc-slam_amd/csrc/lba_tri_math.hpp: the fixed-sweep one-sided Jacobi
tri_null4, tri_triangulate, the gates, tri_row) built for the host (tests/native/tri_harness.cpp) against
numpy.linalg.svd and the fp64 restatement (tests/tri_oracle.py).

The null vector is held to the project's backward-error form: |A v|_2 <= sigma4 + 64 n u |A|_2 with n = 4, u = 2^-53,
and to numpy's vector within the sum of the two solvers' backward errors over the gap, 2 * 64 n u sigma1 /
(sigma3 - sigma4), on generated rows and on matrices whose sigma3 / sigma4 goes down to 1 + 1e-6."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tri_cases as tc
import tri_oracle as to
from amc_lba.abi import ptr
from amc_lba.triangulate import make_tri_pairs, tri_keyframes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
U = 2.0 ** -53
BACKWARD = 64 * 4 * U


@pytest.fixture(scope="module")
def harness():
    src = os.path.join(ROOT, "tests", "native", "tri_harness.cpp")
    out = os.path.join(ROOT, "tests", "native", "_build", "libtri_harness.so")
    deps = [src, os.path.join(ROOT, "include", "amc_lba.h")] + [os.path.join(ROOT, "amc-slam_amd", "csrc", h) for h in ("lba_tri_math.hpp", "lba_math.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.tri_null.argtypes = [_dp, ctypes.c_int, _dp, _dp]
    L.tri_A.argtypes = [_dp] * 5
    L.tri_A.restype = None
    L.tri_point.argtypes = [_dp] * 5
    L.tri_cos.argtypes = [ctypes.c_double] * 2
    L.tri_cos.restype = ctypes.c_double
    L.tri_unproject.argtypes = [_dp, ctypes.c_double, vp, vp, _dp]
    L.tri_reproj.argtypes = [vp, ctypes.c_double, _dp, _dp, ctypes.c_double, ctypes.c_double]
    L.tri_rows_host.argtypes = [vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double]
    L.tri_rows_host.restype = None
    return L


def _d(a):
    return a.ctypes.data_as(_dp)


def _null(L, A, sweeps=None):
    A = np.ascontiguousarray(A, float)
    v, sig = np.zeros(4), np.zeros(1)
    assert L.tri_null(_d(A), L.tri_sweeps() if sweeps is None else sweeps, _d(v), _d(sig)) == 0
    return v, sig[0]


def _matrices():
    """A of generated rows, and U diag(s) V^T with sigma3 / sigma4 from 2 down to 1 + 1e-6"""
    out = []
    pairs, rows, kfs, cams, _ = make_tri_pairs(n_pairs=2, n_rows=100, seed=40)
    for P in pairs:
        for r in rows[P["row0"]:P["row0"] + P["n_rows"]]:
            c1, c2 = cams[kfs[P["kf1"]]["cam0"] + r["cam1"]], cams[kfs[P["kf2"]]["cam0"] + r["cam2"]]
            xn1 = [(r["z1"][0] - c1["cx"]) / c1["fx"], (r["z1"][1] - c1["cy"]) / c1["fy"]]
            xn2 = [(r["z2"][0] - c2["cx"]) / c2["fx"], (r["z2"][1] - c2["cy"]) / c2["fy"]]
            out.append(to.build_A(xn1, c1["Tcw"].reshape(3, 4), xn2, c2["Tcw"].reshape(3, 4)))
    rng = np.random.default_rng(41)
    for k in range(100):
        Q1, _ = np.linalg.qr(rng.normal(size=(4, 4)))
        Q2, _ = np.linalg.qr(rng.normal(size=(4, 4)))
        g = 10.0 ** (-6.0 * k / 99)
        s4 = 10.0 ** rng.uniform(-3, 0)
        s = np.array([10.0 ** rng.uniform(0.5, 1), rng.uniform(1.5, 3.0), 1 + g, 1.0]) * [1, s4, s4, s4]
        out.append(Q1 @ np.diag(s) @ Q2.T)
    return out


def test_null_vector_residual_and_direction(harness):
    worst_r = worst_v = 0.0
    for A in _matrices():
        v, sig = _null(harness, A)
        _, s, Vt = np.linalg.svd(A)
        assert abs(np.linalg.norm(v) - 1.0) <= BACKWARD
        res = np.linalg.norm(A @ v)
        assert res <= s[3] + BACKWARD * s[0], (res - s[3]) / s[0]
        ref = Vt[3] if Vt[3] @ v >= 0 else -Vt[3]
        bound = 2 * BACKWARD * s[0] / (s[2] - s[3])
        assert np.linalg.norm(v - ref) <= bound, (np.linalg.norm(v - ref), bound)
        worst_r, worst_v = max(worst_r, (res - s[3]) / (BACKWARD * s[0])), max(worst_v, np.linalg.norm(v - ref) / bound)
    print(f"residual at {worst_r:.2e} of its bound, direction at {worst_v:.2e} of its bound")


def test_the_sweep_count_is_the_one_that_converges_plus_one(harness):
    """one sweep fewer meets the residual bound on every matrix too; two fewer does not"""
    n = harness.tri_sweeps()
    mats = _matrices()

    def misses(sweeps):
        count = 0
        for A in mats:
            v, _ = _null(harness, A, sweeps)
            s = np.linalg.svd(A, compute_uv=False)
            count += np.linalg.norm(A @ v) > s[3] + BACKWARD * s[0]
        return count
    assert misses(n) == 0 and misses(n - 1) == 0 and misses(n - 2) > 0


def test_parallel_rays_give_w_zero_exactly(harness):
    """identity rotations, t2 = (-1, 0, 0), both rays (0, 0, 1): A's third column is zero, the null vector is e3 and
    w == 0 exactly: LBA_TRI_W_ZERO, the status no float keypoints reach"""
    T1 = np.hstack([np.eye(3), np.zeros((3, 1))]).ravel()
    T2 = np.hstack([np.eye(3), [[-1.0], [0.0], [0.0]]]).ravel()
    xn = np.array([0.0, 0.0, 1.0])
    A = np.zeros(16)
    harness.tri_A(_d(xn), _d(T1), _d(xn), _d(T2), _d(A))
    assert (A.reshape(4, 4) == to.build_A(xn, T1.reshape(3, 4), xn, T2.reshape(3, 4))).all()
    assert (A.reshape(4, 4)[:, 2] == 0).all()
    v, sig = _null(harness, A)
    assert v[3] == 0.0 and abs(v[2]) == 1.0 and sig == 0.0
    X = np.full(3, 7.0)
    assert harness.tri_point(_d(xn), _d(T1), _d(xn), _d(T2), _d(X)) == 0 and (X == 7.0).all()
    # a NaN in A ends the same way, and ends
    xn_nan = np.array([np.nan, 0.0, 1.0])
    assert harness.tri_point(_d(xn_nan), _d(T1), _d(xn), _d(T2), _d(X)) == 0 and (X == 7.0).all()


def test_cos_stereo_is_cos_of_twice_atan2(harness):
    rng = np.random.default_rng(42)
    for b, d in [(0.12, 0.0), (0.12, -1.0), (0.0, 0.0), (0.12, 5.0)] + [(rng.uniform(0.05, 0.5), rng.uniform(0.1, 100)) for _ in range(200)]:
        want = np.cos(2 * np.arctan2(b / 2, d))
        assert abs(harness.tri_cos(b, d) - want) <= 8 * U, (b, d)
    assert np.isnan(harness.tri_cos(0.12, np.nan))


def test_unproject_stereo_and_reprojection_gates(harness):
    kfs, cams = tri_keyframes([(np.eye(3), np.zeros(3)), (tc._two((1.0, 0.0, 0.3))[0][1]["Rwb"].reshape(3, 3), np.array([1.0, 2.0, 3.0]))], 4)
    k = np.array([500.25, 310.5])
    X = np.full(3, 7.0)
    for z in (0.0, -1.0, np.nan):
        assert harness.tri_unproject(_d(k), z, ptr(cams[7:8]), ptr(kfs[1:2]), _d(X)) == 0 and (X == 7.0).all()
    assert harness.tri_unproject(_d(k), 4.0, ptr(cams[7:8]), ptr(kfs[1:2]), _d(X)) == 1
    c = cams[7]
    want = kfs[1]["Rwb"].reshape(3, 3) @ [(k[0] - c["cx"]) * 4.0 * c["invfx"], (k[1] - c["cy"]) * 4.0 * c["invfy"], 4.0] + kfs[1]["twb"]
    assert np.abs(X - want).max() <= 16 * U * np.abs(want).max()
    rng = np.random.default_rng(43)
    for _ in range(200):
        xyz = np.array([rng.normal(0, 2), rng.normal(0, 2), rng.uniform(1, 20)])
        u, v = c["fx"] * xyz[0] / xyz[2] + c["cx"], c["fy"] * xyz[1] / xyz[2] + c["cy"]
        kp = np.array([u, v]) + rng.normal(0, 2.0, 2)
        ur = u - kfs[1]["bf"] / xyz[2] + rng.normal(0, 2.0)
        e2 = (u - kp[0]) ** 2 + (v - kp[1]) ** 2
        if abs(e2 - 5.991) > 1e-9:
            assert harness.tri_reproj(ptr(cams[7:8]), kfs[1]["bf"], _d(xyz), _d(kp), -1.0, 1.0) == int(e2 > 5.991)
        e3 = e2 + (u - kfs[1]["bf"] / xyz[2] - ur) ** 2
        if ur >= 0 and abs(e3 - 7.8) > 1e-9:
            assert harness.tri_reproj(ptr(cams[7:8]), kfs[1]["bf"], _d(xyz), _d(kp), ur, 1.0) == int(e3 > 7.8)
    # a NaN error passes the gate, as in the reference
    assert harness.tri_reproj(ptr(cams[7:8]), kfs[1]["bf"], _d(np.array([0.0, 0.0, 5.0])), _d(np.array([np.nan, 1.0])), -1.0, 1.0) == 0


@pytest.mark.parametrize("name", tc.NAMES)
def test_rows_on_the_host_match_the_restatement(harness, name):
    """tri_row, the function the kernel calls per thread, over every named case"""
    c, r64, _ = tc.case(name)
    rows = c.rows.copy()
    rows["X"] = 7.0
    harness.tri_rows_host(ptr(c.pairs), len(c.pairs), ptr(rows), ptr(c.kfs), ptr(c.cams), c.n_cam, c.ratio, c.far_points, c.th_far)
    st = tc.settled_rows(c, r64)
    assert (rows["status"][st] == r64.status[st]).all() and (rows["stereo_point"][st] == r64.stereo[st]).all()
    if name != "shared_rows":   # (this harness visits a shared row twice in place; the scatter is lba_triangulate's)
        assert (rows["X"][c.in_pairs() & (rows["status"] != to.OK)] == 7.0).all()
    for i in np.flatnonzero(st & (r64.status == to.OK) & np.isfinite(r64.X).all(1)):
        if r64.triangulated[i]:
            assert np.linalg.norm(rows["X"][i] - r64.X[i]) <= tc.x_bound(r64.X[i], r64.sigma[i])
        else:
            assert np.abs(rows["X"][i] - r64.X[i]).max() <= 16 * U * max(1.0, np.abs(r64.X[i]).max())
    if name == "nan_keypoint":
        assert rows["status"][0] == to.OK and np.isnan(rows["X"][0]).any()
