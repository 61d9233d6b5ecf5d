"""The product's Sim3 maths (amc-slam_amd/csrc/lba_math.hpp: sim3_exp, sim3_mul, sim3_inv, sim3_map, sim3_edge12,
sim3_edge21) built for the host and put together as k_sim3 does (tests/native/sim3_harness.cpp), against the numpy
restatement (tests/sim3_oracle.py): Sim3(update) and the vertex's left update on both sides of |sigma| = 1e-5 and
theta = 1e-5 (all four branches, and update = 0), map, inverse, both edge errors and both analytic Jacobians.  The two
evaluate the same formulas in another order (the product carries a unit quaternion and rotation matrices, the
restatement g2o's unnormalised quaternion), so they agree to rounding: 1e-9 relative, the bound of
tests/test_vel_math_host.py for the same kind of comparison.  The analytic Jacobian is also held against a central
difference of step 1e-6 through the restatement's oplus, to 1e-6 relative."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sim3_oracle as so
from amc_lba.sim3 import make_sim3_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def sim3_harness():
    src = os.path.join(ROOT, "tests", "native", "sim3_harness.cpp")
    out = os.path.join(ROOT, "tests", "native", "_build", "libsim3_harness.so")
    deps = [src, os.path.join(ROOT, "amc-slam_amd", "csrc", "lba_math.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    L = ctypes.CDLL(out)
    L.sim3_oplus.argtypes = [_dp] * 4
    L.sim3_map_inverse.argtypes = [_dp] * 4
    L.sim3_edges.argtypes = [_dp] * 7 + [ctypes.c_int] + [_dp] * 4
    for f in (L.sim3_oplus, L.sim3_map_inverse, L.sim3_edges):
        f.restype = None
    return L


def _d(a):
    return a.ctypes.data_as(_dp)


def _pack(S):
    return np.array([*S.r, *S.t, S.s], float)


def _gap(got, S):
    """(q up to sign, t, s) of a packed product state against a restatement Sim3, relative to max(1, |.|_inf)."""
    q = S.r / np.linalg.norm(S.r)
    gq = min(np.abs(got[:4] - q).max(), np.abs(got[:4] + q).max())
    gt = np.abs(got[4:7] - S.t).max() / max(1.0, np.abs(S.t).max())
    return max(gq, gt, abs(got[7] - S.s) / max(1.0, abs(S.s)))


def _start():
    pairs, corr, cams, _ = make_sim3_pairs(n_corr=24, n_cam=4, seed=7, s_true=1.15)
    return pairs[0], corr, cams


UPDATES = [
    ("zero", np.zeros(7), 0),
    ("sigma and theta below eps", np.array([3e-6, -4e-6, 5e-6, 0.01, -0.02, 0.03, 6e-6]), 0),
    ("sigma below eps, theta above", np.array([3e-5, -4e-5, 5e-5, 0.01, -0.02, 0.03, -6e-6]), 1),
    ("sigma below eps, regular rotation", np.array([0.02, -0.03, 0.2, 0.4, -0.1, 0.2, 0.0]), 1),
    ("sigma above eps, theta below", np.array([3e-6, -4e-6, 5e-6, 0.01, -0.02, 0.03, 2e-5]), 2),
    ("scale only", np.array([0.0, 0.0, 0.0, 0.3, 0.1, -0.2, 0.25]), 2),
    ("sigma and theta just above eps", np.array([6e-6, -6e-6, 6e-6, 0.01, -0.02, 0.03, -1.1e-5]), 3),
    ("regular", np.array([0.02, -0.03, 0.2, 0.4, -0.1, 0.2, 0.1]), 3),
    ("far", np.array([0.2, -0.1, 0.15, 1.0, -1.0, 0.5, np.log(1.3)]), 3),
]


@pytest.mark.parametrize("what,update,branch", UPDATES, ids=[u[0] for u in UPDATES])
def test_exp_and_left_update_match_restatement(sim3_harness, what, update, branch):
    assert so.exp_coeffs(update)[0] == branch
    pair, _, _ = _start()
    S = so.Sim3(pair["q"], pair["t"], pair["s"])
    expo, out = np.zeros(8), np.zeros(8)
    sim3_harness.sim3_oplus(_d(np.ascontiguousarray(update)), _d(_pack(S)), _d(expo), _d(out))
    g_exp, g_mul = _gap(expo, so.sim3_exp(update)), _gap(out, so.oplus(S, update, False))
    print(f"{what}: product vs restatement  Sim3(update) {g_exp:.2e}  Sim3(update) * S {g_mul:.2e}")
    assert g_exp <= 1e-9 and g_mul <= 1e-9
    if what == "zero":
        assert expo[7] == 1.0 and out[7] == S.s        # s is carried bitwise through a zero sigma (fix_scale)


def test_map_and_inverse_match_restatement(sim3_harness):
    pair, corr, _ = _start()
    S = so.Sim3(pair["q"], pair["t"], pair["s"])
    worst = 0.0
    for row in corr[:8]:
        x = np.ascontiguousarray(row["X2c"])
        y, inv = np.zeros(3), np.zeros(8)
        sim3_harness.sim3_map_inverse(_d(_pack(S)), _d(x), _d(y), _d(inv))
        y_o = S.map(x)
        worst = max(worst, np.abs(y - y_o).max() / max(1.0, np.abs(y_o).max()), _gap(inv, S.inverse()))
    print(f"map / inverse: product vs restatement {worst:.2e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("fix_scale", [0, 1])
def test_edges_and_jacobians_match_restatement(sim3_harness, fix_scale):
    pair, corr, cams = _start()
    S = so.Sim3(pair["q"], pair["t"], pair["s"])
    Sp = _pack(S)
    worst_e = worst_j = worst_fd = 0.0
    for row in corr:
        g1, g2 = cams[int(row["cam1"])], cams[4 + int(row["cam2"])]
        c1, c2 = so.Cam(g1), so.Cam(g2)
        a1 = np.array([*g1["q"], *g1["t"], g1["fx"], g1["fy"], g1["cx"], g1["cy"]], float)
        a2 = np.array([*g2["q"], *g2["t"], g2["fx"], g2["fy"], g2["cx"], g2["cy"]], float)
        e12, e21, J12, J21 = np.zeros(2), np.zeros(2), np.zeros(14), np.zeros(14)
        sim3_harness.sim3_edges(_d(Sp), _d(a1), _d(a2), _d(np.ascontiguousarray(row["X1c"])), _d(np.ascontiguousarray(row["X2c"])),
                                _d(np.ascontiguousarray(row["z1"])), _d(np.ascontiguousarray(row["z2"])), fix_scale,
                                _d(e12), _d(J12), _d(e21), _d(J21))
        for e, J, err, jac in ((e12, J12, so.error12, so.analytic_jac12), (e21, J21, so.error21, so.analytic_jac21)):
            e_o = err(S, c1, c2, row)
            J_o = jac(S, c1, c2, row, bool(fix_scale))
            J_fd = so.numeric_jac(err, S, c1, c2, row, bool(fix_scale), delta=1e-6)
            scale = max(1.0, np.abs(J_o).max())
            worst_e = max(worst_e, np.abs(e - e_o).max() / max(1.0, np.abs(e_o).max()))
            worst_j = max(worst_j, np.abs(J.reshape(2, 7) - J_o).max() / scale)
            worst_fd = max(worst_fd, np.abs(J.reshape(2, 7) - J_fd).max() / scale)
            if fix_scale:
                assert (J.reshape(2, 7)[:, 6] == 0).all() and (J_fd[:, 6] == 0).all()
    print(f"fix_scale {fix_scale}: product vs restatement  e {worst_e:.2e}  J {worst_j:.2e}  J vs central difference {worst_fd:.2e}")
    assert worst_e <= 1e-9 and worst_j <= 1e-9
    assert worst_fd <= 1e-6
