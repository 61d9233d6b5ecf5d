"""The MCRansac cases (tests/vel_cases.py) and their checker (tests/vel_oracle.py) on the CPU, no GPU.

The restatement's Jacobian agrees with central differences on both sides of RightJacobianPose3's small-angle
branches; every case has the property it is named for; every case keeps the settled cap (at most 10 % of its
hypotheses unsettled, every frame settled: a condition on the inputs, so a case that breaks it gets another seed,
never a higher cap); the numpy mirrors of lba_vel_obs / lba_vel_frame / lba_vel_params have the header's sizes.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import vel_cases as vc
import vel_oracle as vo
from amc_lba.track import make_vel_frames, track_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "amc_lba.h")


# ------------------------------------------------------------------ the restatement itself
def _numeric_jacobian(rig, R, t, v, cam, dt, z, Xw, d=1e-6):
    J = np.zeros((2, 6))
    for k in range(6):
        dv = np.zeros(6)
        dv[k] = d
        J[:, k] = (vo.errors(rig, R, t, v + dv, cam, dt, z, Xw)[0] - vo.errors(rig, R, t, v - dv, cam, dt, z, Xw)[0]) / (2 * d)
    return J


@pytest.mark.parametrize("what,v,dt", [
    ("zero velocity", np.zeros(6), 0.1),
    ("rotation below 1e-5", np.array([4.0, 0.2, -0.1, 2e-5, -3e-5, 5e-5]), 0.1),       # |w dt| = 6e-6
    ("rotation above 1e-5", np.array([4.0, 0.2, -0.1, 1e-4, -2e-4, 3e-4]), 0.1),       # |w dt| = 3.7e-5
    ("regular", np.array([4.0, 0.2, -0.1, 0.02, -0.03, 0.2]), 0.1),
    ("fast turn", np.array([3.0, -0.5, 0.2, 0.3, -0.4, 1.5]), 0.11),
])
def test_jacobian_matches_central_differences(what, v, dt):
    fr, ob, _, cams, _ = make_vel_frames(n_obs=40, n_hyp=0, seed=7)
    rig = vo.Rig(cams)
    R, t = vo.quat_rot(fr[0]["q"]), fr[0]["t"]
    w = np.linalg.norm(v[3:]) * dt
    assert {"rotation below 1e-5": w < 1e-5, "rotation above 1e-5": 1e-5 < w < 1e-4}.get(what, True)
    worst = 0.0
    for o in ob[:12]:
        J = vo.jacobian(rig, R, t, v, int(o["cam"]), dt, o["Xw"])
        Jn = _numeric_jacobian(rig, R, t, v, int(o["cam"]), dt, o["z"], o["Xw"])
        worst = max(worst, np.abs(J - Jn).max() / np.abs(Jn).max())
    print(f"{what}: Jacobian vs central differences {worst:.2e} relative")
    assert worst <= 1e-6


def test_oracle_recovers_the_true_velocity():
    """(the restatement is a working RANSAC: the best hypothesis of a clean frame lies at the truth)"""
    fr, ob, sm, cams, truth = make_vel_frames(n_obs=150, n_hyp=12, noise=0.3, seed=5)
    r = vo.run_frame(fr[0], ob, sm, cams)
    assert r["n_inliers"] >= 0.8 * (~truth["gross"]).sum()
    assert not r["inlier"][truth["gross"]].any()
    assert np.abs(r["vel"] - truth["vel"][0]).max() < 0.1
    assert ((1 <= r["hyp_iterations"]) & (r["hyp_iterations"] <= 40)).all()


# ------------------------------------------------------------------ every case has its property
@pytest.mark.parametrize("name", vc.CASES)
def test_case_shape(name):
    fr, ob, sm, cams, prm = vc.case(name)
    assert len(fr) == 1 and len(ob) <= 200 and len(sm) <= 23 and fr[0]["n_obs"] == len(ob) and fr[0]["n_hyp"] == len(sm)
    assert ((ob["cam"] >= 0) & (ob["cam"] < len(cams))).all()
    for f in ("dt", "z", "w", "Xw"):
        assert np.isfinite(ob[f]).all()
    assert ((sm >= 0) & (sm < len(ob))).all()
    assert all(len(set(t)) == 3 for t in sm.tolist())
    assert len(set(zip(ob["cam"].tolist(), ob["dt"].tolist()))) <= 16
    r = vc.reference(name)[0]
    it = prm.iterations if prm is not None else 40
    assert ((min(1, it) <= r["hyp_iterations"]) & (r["hyp_iterations"] <= it)).all()


def test_plain_and_size_cases():
    fr, ob, sm, cams, _ = vc.case("plain")
    assert len(ob) == 200 and len(sm) == 23 and len(cams) == 4 and len(np.unique(ob["dt"])) == 4
    assert vc.reference("plain")[0]["n_inliers"] > 100
    for n in vc.N_OBS_EDGES:
        assert len(vc.case(f"nobs_{n}")[1]) == n
        assert vc.reference(f"nobs_{n}")[0]["best_hyp"] >= 0
    for n in vc.N_HYP_EDGES:
        assert len(vc.case(f"nhyp_{n}")[2]) == n
    assert vc.reference("nobs_3")[0]["n_inliers"] == 3       # three edges fit six unknowns exactly


def test_dup_tie_first_wins():
    _, _, sm, _, _ = vc.case("dup_tie")
    r = vc.reference("dup_tie")[0]
    b = r["best_hyp"]
    assert 0 <= b < 6 and sorted(sm[b]) == sorted(sm[b + 6]) and list(sm[b]) != list(sm[b + 6])
    assert r["hyp_inliers"][b + 6] == r["hyp_inliers"][b] == r["n_inliers"] == r["hyp_inliers"].max()


def test_one_cam_triples_and_one_dt():
    _, ob, sm, _, _ = vc.case("one_cam_triples")
    assert (ob["cam"][sm] == 1).all() and len(np.unique(ob["cam"])) == 4
    _, ob, _, _, _ = vc.case("one_dt")
    assert len(np.unique(ob["dt"])) == 1 and len(np.unique(ob["cam"])) == 4


def test_zero_start():
    fr, _, _, _, _ = vc.case("zero_start")
    assert (fr[0]["vel"] == 0).all()
    r = vc.reference("zero_start")[0]
    assert np.abs(r["vel"] - vc.truth("zero_start")["vel"][0]).max() < 0.2      # converges from 4 m/s away


def test_sampled_outlier_huber_active():
    fr, ob, sm, cams, _ = vc.case("sampled_outlier")
    gross = vc.truth("sampled_outlier")["gross"]
    rig = vo.Rig(cams)
    R, t = vo.quat_rot(fr[0]["q"]), fr[0]["t"]
    for tri in sm:
        assert gross[tri[0]]
        o = ob[tri[0]]
        e = vo.errors(rig, R, t, fr[0]["vel"], int(o["cam"]), float(o["dt"]), o["z"], o["Xw"])[0]
        assert o["w"] * (e @ e) > vc.HUBER2               # beyond the quadratic range at the start


def test_dt0_cam_keeps_the_start_velocity():
    fr, ob, sm, _, _ = vc.case("dt0_cam")
    assert (ob["dt"][ob["cam"] == 0] == 0).all() and (ob["dt"][ob["cam"] != 0] > 0).all()
    assert (ob["cam"][sm[:3]] == 0).all() and (ob["cam"][sm[3]] == 0).sum() in (1, 2)
    r = vc.reference("dt0_cam")[0]
    for h in range(3):                                      # H = 0: no step is ever taken
        assert (r["hyp_vel"][h] == fr[0]["vel"]).all()
    assert (r["hyp_vel"][3] != fr[0]["vel"]).any()


def test_behind_points_are_scored_without_a_depth_test():
    fr, ob, sm, cams, _ = vc.case("behind")
    rig = vo.Rig(cams)
    R, t = vo.quat_rot(fr[0]["q"]), fr[0]["t"]
    v = vc.truth("behind")["vel"][0]
    depth = np.zeros(len(ob))
    for i, o in enumerate(ob):
        c = int(o["cam"])
        Re, te = vo.se3_exp(v * o["dt"])
        Rwc, twc = R @ Re @ rig.Rbc[c], R @ (Re @ rig.tbc[c] + te) + t
        depth[i] = ((o["Xw"] - twc) @ Rwc)[2]
    assert (depth[:vc.BEHIND] < -1).all() and (depth[vc.BEHIND:] > 1).all()
    assert any(i < vc.BEHIND for i in sm[0]) and any(i < vc.BEHIND for i in sm[1])
    r = vc.reference("behind")[0]
    gross = vc.truth("behind")["gross"]
    keep = ~gross[:vc.BEHIND]
    assert keep.sum() >= 5 and r["inlier"][:vc.BEHIND][keep].sum() >= keep.sum() - 2    # inliers, depth < 0 or not


def test_shuffled_is_a_permutation_of_the_same_problem():
    _, ob, sm, _, _ = vc.case("shuffled")
    _, ob_u, sm_u, _, _, _ = vc._shuffled(shuffle=False)
    perm = vc.shuffle_perm(len(ob))
    assert ob.tobytes() == ob_u[perm].tobytes() and (perm[sm] == sm_u).all()
    assert (np.diff(sm, axis=1) < 0).any()                   # triples no longer ascending on entry


def test_params_and_empty_cases():
    prm = vc.case("params")[4]
    assert (prm.threshold, prm.iterations) == (3.5, 1)
    assert (vc.reference("params")[0]["hyp_iterations"] == 1).all()
    r = vc.reference("all_zero")[0]
    assert (r["hyp_inliers"] == 0).all() and r["best_hyp"] == -1 and r["n_inliers"] == 0 and not r["inlier"].any()
    assert (r["vel"] == vc.case("all_zero")[0][0]["vel"]).all()
    r = vc.reference("nhyp_0")[0]
    assert r["best_hyp"] == -1 and len(r["hyp_inliers"]) == 0


# ------------------------------------------------------------------ conditioning: the settled cap
@pytest.mark.parametrize("name", vc.CASES)
def test_settled_cap(name):
    r = vc.reference(name)[0]
    n = len(r["settled"])
    uns = int((~r["settled"]).sum())
    margin = np.abs(r["hyp_norm"] - (vc.case(name)[4].threshold if vc.case(name)[4] is not None else 2.0))
    print(f"{name}: {uns} of {n} hypotheses unsettled, frame settled {r['frame_settled']}, "
          f"nearest ||e|| to the threshold {margin.min(initial=np.inf):.2e} px")
    assert r["frame_settled"]
    assert uns <= vc.MAX_UNSETTLED * n


# ------------------------------------------------------------------ the mirrors
def _c_sizeof(struct):
    code = f'#include "{HEADER}"\n#include <stdio.h>\nint main(void){{printf("%zu", sizeof({struct}));return 0;}}'
    exe = os.path.join(ROOT, "tests", "native", "_build", "_vel_abi_sz")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["gcc", "-x", "c", "-", "-o", exe], input=code, text=True, check=True)
    return int(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)


def test_vel_structs_match_header():
    from amc_lba.track import VEL_FRAME_DTYPE, VEL_OBS_DTYPE, LbaVelParams
    assert _c_sizeof("lba_vel_obs") == VEL_OBS_DTYPE.itemsize
    assert _c_sizeof("lba_vel_frame") == VEL_FRAME_DTYPE.itemsize
    assert _c_sizeof("lba_vel_params") == ctypes.sizeof(LbaVelParams)
    assert track_config().lambda_init == 0.0                 # (no user lambda in the tracker's configuration)
