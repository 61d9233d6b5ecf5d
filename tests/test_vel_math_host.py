"""The product's EdgeVelReproj maths (amc-slam_amd/csrc/lba_math.hpp: vel_motion, vel_reproj_error, vel_reproj_jac)
built for the host and put together as k_vel_hyp does (tests/native/vel_harness.cpp), against the numpy restatement
(tests/vel_oracle.py): error and Jacobian on both sides of the small-angle branches, at dt = 0 and for a point
behind the camera.  The two evaluate the same formulas in another order (the product inverts exp(v dt), the
restatement the whole chain T exp(v dt) Tbc), so they agree to rounding: 1e-9 relative for errors of some pixels and
Jacobian entries of some hundred pixels per m/s computed in double from float-valued inputs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import vel_oracle as vo
from amc_lba.track import make_vel_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def vel_harness():
    src = os.path.join(ROOT, "tests", "native", "vel_harness.cpp")
    out = os.path.join(ROOT, "tests", "native", "_build", "libvel_harness.so")
    deps = [src, os.path.join(ROOT, "amc-slam_amd", "csrc", "lba_math.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    L = ctypes.CDLL(out)
    L.vel_edge.argtypes = [_dp, _dp, _dp, _dp, ctypes.c_double, _dp, _dp, _dp, _dp]
    L.vel_edge.restype = None
    return L


def _d(a):
    return a.ctypes.data_as(_dp)


@pytest.mark.parametrize("what,v,dt", [
    ("zero velocity", np.zeros(6), 0.1),
    ("rotation below 1e-5", np.array([4.0, 0.2, -0.1, 2e-5, -3e-5, 5e-5]), 0.1),
    ("rotation above 1e-5", np.array([4.0, 0.2, -0.1, 1e-4, -2e-4, 3e-4]), 0.1),
    ("regular", np.array([4.0, 0.2, -0.1, 0.02, -0.03, 0.2]), 0.1),
    ("fast turn", np.array([3.0, -0.5, 0.2, 0.3, -0.4, 1.5]), 0.11),
    ("dt = 0", np.array([4.0, 0.2, -0.1, 0.02, -0.03, 0.2]), 0.0),
])
def test_product_edge_matches_restatement(vel_harness, what, v, dt):
    fr, ob, _, cams, _ = make_vel_frames(n_obs=40, n_hyp=0, seed=7)
    rig = vo.Rig(cams)
    q, t = np.ascontiguousarray(fr[0]["q"]), np.ascontiguousarray(fr[0]["t"])
    R = vo.quat_rot(q)
    ob = ob.copy()
    ob["Xw"][0] = 2 * t - ob["Xw"][0]                       # (somewhere else: behind or beside its camera)
    worst_e = worst_j = 0.0
    for o in ob[:16]:
        c = cams[int(o["cam"])]
        cam = np.array([*c["q"], *c["t"], c["fx"], c["fy"], c["cx"], c["cy"]], float)
        e, J = np.zeros(2), np.zeros(12)
        vel_harness.vel_edge(_d(q), _d(t), _d(cam), _d(np.ascontiguousarray(v, float)), dt,
                             _d(np.ascontiguousarray(o["z"])), _d(np.ascontiguousarray(o["Xw"])), _d(e), _d(J))
        e_o = vo.errors(rig, R, t, v, int(o["cam"]), dt, o["z"], o["Xw"])[0]
        J_o = vo.jacobian(rig, R, t, v, int(o["cam"]), dt, o["Xw"])
        worst_e = max(worst_e, np.abs(e - e_o).max() / max(1.0, np.abs(e_o).max()))
        worst_j = max(worst_j, np.abs(J.reshape(2, 6) - J_o).max() / max(1.0, np.abs(J_o).max()))
        if dt == 0.0:
            assert (J == 0).all()
    print(f"{what}: product vs restatement  e {worst_e:.2e}  J {worst_j:.2e}")
    assert worst_e <= 1e-9 and worst_j <= 1e-9
