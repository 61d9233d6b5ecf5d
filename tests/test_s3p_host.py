"""The Sim3 projection search's maths (amc-slam_amd/csrc/lba_s3p_math.hpp) built for the host with
g++ -O2 -ffp-contract=off (tests/native/s3p_harness.cpp) against the numpy restatement (tests/s3p_oracle.py) on the named
cases: the fp64 pose chain within M_POSE, the float Tcw and every job's x, y, radius, level and status BIT-IDENTICAL,
whole searches identical.  The same harness is built once more as a stand-alone program with
-fsanitize=address,undefined and run (a host build; nothing is loaded into Python)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import s3p_cases as sc
import s3p_oracle as so
from amc_lba.abi import ptr
from amc_lba.sim3_project import S3P_POSE_DTYPE, S3P_ROW_DTYPE, LbaS3pParams, pack_hypotheses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "s3p_harness.cpp")
BUILD = os.path.join(ROOT, "tests", "native", "_build")
DEPS = [SRC, os.path.join(ROOT, "include", "amc_lba.h")] + [os.path.join(ROOT, "amc-slam_amd", "csrc", h)
                                                            for h in ("lba_s3p_math.hpp", "lba_match_math.hpp", "lba_math.hpp")]
F = np.float32


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


def load_harness():
    out = os.path.join(BUILD, "libs3p_harness.so")
    if _stale(out):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", out])
    L = ctypes.CDLL(out)
    vp, f, i = ctypes.c_void_p, ctypes.c_float, ctypes.c_int
    L.sh_pose.argtypes = [vp, vp, vp, vp]
    L.sh_pose.restype = None
    L.sh_project.argtypes = [vp, vp, vp, vp, vp, ctypes.POINTER(LbaS3pParams), vp, vp]
    L.sh_project.restype = None
    L.sh_quotient.argtypes = [f, f, f]
    L.sh_quotient.restype = ctypes.c_double
    L.sh_level.argtypes = [f, f, f, i]
    L.sh_search.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, ctypes.POINTER(LbaS3pParams), vp, vp, vp]
    L.sh_params_ok.argtypes = [ctypes.POINTER(LbaS3pParams)]
    return L


@pytest.fixture(scope="module")
def harness():
    return load_harness()


def host_pose(L, kfm, hyp):
    S, _, _ = pack_hypotheses(kfm, [hyp])
    out = np.zeros((kfm.n_cam, 12))
    for c in range(kfm.n_cam):
        L.sh_pose(ptr(kfm.kf), ptr(kfm.kcams[c:c + 1]), ptr(S), ptr(out[c]))
    return out


def host_search(L, kfm, hyp, prm):
    """the header's sequential loop: an s3p_oracle.Result"""
    S, points, taken = pack_hypotheses(kfm, [hyp])
    res = so.Result(len(hyp.points), kfm.n_cam, len(kfm.feats))
    rows = np.zeros(len(hyp.points) * kfm.n_cam, S3P_ROW_DTYPE)
    poses = np.zeros(kfm.n_cam, S3P_POSE_DTYPE)
    res.n_matches = L.sh_search(ptr(kfm.kf), ptr(kfm.kcams), ptr(kfm.gcams), ptr(kfm.sf), ptr(kfm.cell_start),
                                ptr(kfm.cell_feat), ptr(kfm.feats), len(kfm.feats), ptr(S), ptr(points),
                                ptr(taken) if hyp.taken is not None else None, ctypes.byref(prm), ptr(rows),
                                ptr(res.feat_point), ptr(poses))
    res.rows, res.poses = rows.reshape(len(hyp.points), kfm.n_cam), poses
    return res


@pytest.mark.parametrize("name", sc.NAMES)
def test_pose_chain_within_m_pose_and_float_tcw_identical(harness, name):
    kfm, hyps, _ = sc.case(name)
    if not kfm.kf[0]["has_prev"]:
        return
    for h in hyps:
        got, want = host_pose(harness, kfm, h), so.pose_f64(kfm, h)
        assert so.pose_diff(got, want).max() <= sc.M_POSE, so.pose_diff(got, want).max()
        if (np.abs(want) == (np.abs(want) > 0.5)).all():      # an identity chain: exact in both
            assert got.tobytes() == want.tobytes()
        assert (got.astype(F).view(np.uint32) == want.astype(F).view(np.uint32)).all()


@pytest.mark.parametrize("p", sc.PARAMS, ids=sc.PARAM_IDS)
@pytest.mark.parametrize("name", sc.NAMES)
def test_jobs_and_whole_searches_identical(harness, name, p):
    kfm, hyps, _ = sc.case(name)
    prm = sc.params(p)
    for h in hyps:
        want = so.sequential(kfm, h, prm)
        got = host_search(harness, kfm, h, prm)
        assert want.same(got)
        if not kfm.kf[0]["has_prev"]:
            continue
        # one job at a time through s3p_project, on the oracle's float Tcw
        every = max(1, len(h.points) // 60)
        for k in range(0, len(h.points), every):
            for c in range(kfm.n_cam):
                out, xyr = np.zeros(2, np.int32), np.zeros(3, F)
                harness.sh_project(ptr(want.poses["tcw"][c]), ptr(kfm.kf), ptr(kfm.kcams[c:c + 1]), ptr(h.points[k:k + 1]),
                                   ptr(kfm.sf), ctypes.byref(prm), ptr(out), ptr(xyr))
                st, lvl, u, v, r, _ = so.job(want.poses["tcw"][c], kfm.kcams[c], h.points[k], kfm, prm)
                assert (out[0], out[1]) == (st, lvl)
                assert xyr.view(np.uint32).tolist() == np.array([u, v, r], F).view(np.uint32).tolist()


def test_quirk_g_is_refused_and_quirk_h_is_defined(harness):
    assert harness.sh_params_ok(ctypes.byref(sc.params((8, 1.5, 0))))
    assert not harness.sh_params_ok(ctypes.byref(sc.params((8, 5.125, 0))))     # 50 * 5.125 = 256.25
    assert harness.sh_params_ok(ctypes.byref(sc.params((8, 5.0, 0))))           # 250
    assert harness.sh_level(0.0, 0.0, 0.18, 8) == 0                             # NaN
    assert harness.sh_level(1.0, 0.0, 0.18, 8) == 7                             # +inf
    assert harness.sh_level(0.0, 1.0, 0.18, 8) == 0                             # log(0) = -inf


def test_sanitized_harness_runs_clean():
    """address and undefined-behaviour sanitizers on the stand-alone program (its own main): a host build"""
    out = os.path.join(BUILD, "s3p_harness_san")
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the harness")
    if _stale(out):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DS3P_HARNESS_MAIN", SRC, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
