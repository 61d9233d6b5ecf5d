"""The product's pose-graph maths (amc-slam_amd/csrc/lba_pg_math.hpp: sim3_log, sim3_Ad, sim3_pg_edge) built for the
host (tests/native/posegraph_harness.cpp) against the numpy / scipy restatement (tests/posegraph_oracle.py):
Sim3::log on both sides of |sigma| = 1e-5 and of d = 1 - 1e-5 (all four branches), log(exp(x)) = x, Ad, the edge error
and both Jacobians to 1e-9 relative (the two evaluate the same quantities by other routes: the product sums the left
Jacobian's series after halving, the restatement takes scipy's expm of the augmented matrix), and both Jacobians
against a central difference of step 1e-6 through the restatement's oplus to 1e-6 relative.  The central difference's
column 6 is compared only where |sigma(e)| >= 1e-4: in Sim3::log's |sigma| < 1e-5 branches W ignores sigma, so a
difference quotient across them sees no upsilon change."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import posegraph_oracle as po
import sim3_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def pg_harness():
    src = os.path.join(ROOT, "tests", "native", "posegraph_harness.cpp")
    out = os.path.join(ROOT, "tests", "native", "_build", "libposegraph_harness.so")
    deps = [src, os.path.join(ROOT, "amc-slam_amd", "csrc", "lba_pg_math.hpp"),
            os.path.join(ROOT, "amc-slam_amd", "csrc", "lba_math.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    L = ctypes.CDLL(out)
    L.pg_log.argtypes = [_dp] * 2
    L.pg_log_exp.argtypes = [_dp] * 2
    L.pg_Ad.argtypes = [_dp] * 2
    L.pg_left_jac.argtypes = [_dp] * 2
    L.pg_edge.argtypes = [_dp] * 3 + [ctypes.c_int] + [_dp] * 3
    for f in (L.pg_log, L.pg_log_exp, L.pg_Ad, L.pg_left_jac, L.pg_edge):
        f.restype = None
    return L


def _d(a):
    return a.ctypes.data_as(_dp)


def _pack(S):
    return np.array([*(S.r / np.linalg.norm(S.r)), *S.t, S.s], float)


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


# update, the branch of Sim3::log that log(Sim3(update)) takes
UPDATES = [
    ("zero", np.zeros(7), 0),
    ("sigma below eps, d above 1 - eps", np.array([1e-3, -2e-3, 1.5e-3, 0.4, -0.2, 0.3, 6e-6]), 0),
    ("sigma below eps, d just below 1 - eps", np.array([3e-3, -2e-3, 3e-3, 0.4, -0.2, 0.3, -6e-6]), 1),
    ("sigma zero, regular rotation", np.array([0.02, -0.03, 0.2, 0.4, -0.1, 0.2, 0.0]), 1),
    ("sigma just above eps, d above 1 - eps", np.array([1e-3, -2e-3, 1.5e-3, 0.4, -0.2, 0.3, 1.2e-5]), 2),
    ("scale only", np.array([0.0, 0.0, 0.0, 0.3, 0.1, -0.2, 0.25]), 2),
    ("sigma just above eps, d just below 1 - eps", np.array([3e-3, -2e-3, 3e-3, 0.4, -0.2, 0.3, -1.2e-5]), 3),
    ("regular", np.array([0.02, -0.03, 0.2, 0.4, -0.1, 0.2, 0.1]), 3),
    ("far", np.array([0.9, -0.6, 0.5, 25.0, -31.0, 8.0, 0.4]), 3),
]


@pytest.mark.parametrize("what,update,branch", UPDATES, ids=[u[0] for u in UPDATES])
def test_log_matches_restatement_and_inverts_exp(pg_harness, what, update, branch):
    S = so.sim3_exp(update)
    assert po.log_coeffs(S)[0] == branch
    e, e2 = np.zeros(7), np.zeros(7)
    pg_harness.pg_log(_d(_pack(S)), _d(e))
    pg_harness.pg_log_exp(_d(np.ascontiguousarray(update)), _d(e2))
    g_o, g_x = _rel(e, po.sim3_log(S)), _rel(e2, update)
    print(f"{what}: log product vs restatement {g_o:.2e}  log(exp(x)) - x {g_x:.2e}")
    assert g_o <= 1e-9
    # log(exp(x)) = x where the reference's log is one.  With d > 1 - eps it reads omega = deltaR / 2 and the
    # small-angle A and B: exact to second order in theta (theta^2 / 6 = 1.2e-6 relative at theta = 2.7e-3, on
    # components below 0.4).  With |sigma| >= eps on top of that (branch 2) its B = (sigma^2 / 2 - sigma + 1) s /
    # sigma^3 lacks the "- 1" of the limit it stands for (sim3.h:199, and :116 in Sim3(update)), so W is only right
    # where Omega^2 = 0: the round trip is asserted for the pure scale there, and the value against the restatement.
    if branch in (1, 3) or what in ("zero", "scale only"):
        assert g_x <= 1e-9
    elif branch == 0:
        assert g_x <= 1e-8


def _edge_inputs(rng, rot, trans, sigma, noise):
    """C, S0, S1 with E = C S0 S1^-1 = Sim3(noise) for a chosen error, away from the identity."""
    S0 = so.sim3_exp(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3), [rng.normal(0, sigma)]]))
    S1 = so.sim3_exp(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3), [rng.normal(0, sigma)]]))
    C = so.sim3_exp(noise) * S1 * S0.inverse()
    for S in (S0, S1, C):
        S.r = S.r / np.linalg.norm(S.r)
    return C, S0, S1


NOISES = [
    ("zero error", np.zeros(7)),
    ("small", np.array([0.01, -0.02, 0.015, 0.05, -0.02, 0.03, 0.003])),
    ("regular", np.array([0.2, -0.1, 0.3, 1.0, -2.0, 0.5, 0.05])),
    ("no scale error", np.array([0.2, -0.1, 0.3, 1.0, -2.0, 0.5, 0.0])),
    ("above 1 rad and 30 m", np.array([0.9, -0.7, 0.4, 24.0, -19.0, 6.0, 0.4])),
]


@pytest.mark.parametrize("fix_scale", [0, 1])
@pytest.mark.parametrize("what,noise", NOISES, ids=[n[0] for n in NOISES])
def test_edge_and_jacobians(pg_harness, what, noise, fix_scale):
    rng = np.random.default_rng(5)
    C, S0, S1 = _edge_inputs(rng, 0.5, 10.0, 0.0 if fix_scale else 0.1, noise)
    e, J0, J1, A = np.zeros(7), np.zeros(49), np.zeros(49), np.zeros(49)
    pg_harness.pg_edge(_d(_pack(C)), _d(_pack(S0)), _d(_pack(S1)), fix_scale, _d(e), _d(J0), _d(J1))
    pg_harness.pg_Ad(_d(_pack(C)), _d(A))
    e_o = po.edge_error(C, S0, S1)
    J0_o, J1_o = po.analytic_jac(C, S0, S1, bool(fix_scale))
    F0, F1 = po.numeric_jac(C, S0, S1, bool(fix_scale), delta=1e-6)
    g_e, g_A = _rel(e, e_o), _rel(A.reshape(7, 7), po.Ad(C))
    g_J = max(_rel(J0.reshape(7, 7), J0_o), _rel(J1.reshape(7, 7), J1_o))
    cols = slice(0, 7) if abs(e_o[6]) >= 1e-4 or fix_scale else slice(0, 6)
    g_fd = max(np.abs(J.reshape(7, 7)[:, cols] - F[:, cols]).max() / max(1.0, np.abs(F).max())
               for J, F in ((J0, F0), (J1, F1)))
    print(f"{what}, fix_scale {fix_scale}: e {g_e:.2e}  Ad {g_A:.2e}  J vs restatement {g_J:.2e}  J vs central "
          f"difference {g_fd:.2e}  |e| rot {np.linalg.norm(e_o[:3]):.2f} trans {np.linalg.norm(e_o[3:6]):.1f}")
    assert g_e <= 1e-9 and g_A <= 1e-9 and g_J <= 1e-9
    assert g_fd <= 1e-6
    if fix_scale:
        assert (J0.reshape(7, 7)[:, 6] == 0).all() and (J1.reshape(7, 7)[:, 6] == 0).all()
    if what == "above 1 rad and 30 m":
        assert np.linalg.norm(e_o[:3]) > 1.0 and np.linalg.norm(e_o[3:6]) > 30.0


def test_left_jacobian_matches_expm(pg_harness):
    worst = 0.0
    for _, noise in NOISES:
        J = np.zeros(49)
        pg_harness.pg_left_jac(_d(np.ascontiguousarray(noise)), _d(J))
        worst = max(worst, _rel(J.reshape(7, 7), po.left_jac(noise)))
    print(f"left Jacobian: product vs expm of the augmented matrix {worst:.2e}")
    assert worst <= 1e-9
