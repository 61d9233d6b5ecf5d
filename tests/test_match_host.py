"""The product's projection-search maths (amc-slam_amd/csrc/lba_match_math.hpp) built for the host
(tests/native/match_harness.cpp) against the numpy restatement (tests/match_oracle.py) on the named cases,
IDENTICALLY: the cell rectangle, the capacity, one job's gather and decision, a whole search resolved sequentially, and
the rotation pass.  The same harness is built once more as a stand-alone program with -fsanitize=address,undefined and
run (a host build; nothing is loaded into Python)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import match_cases as mc
import match_oracle as mo
from amc_lba.abi import MATCH_SEARCH_DTYPE, ptr
from amc_lba.match import MATCH_BEST, MATCH_OK, MATCH_ROT, LbaMatchParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "match_harness.cpp")
BUILD = os.path.join(ROOT, "tests", "native", "_build")
DEPS = [SRC, os.path.join(ROOT, "include", "amc_lba.h")] + [os.path.join(ROOT, "amc-slam_amd", "csrc", h) for h in ("lba_match_math.hpp", "lba_math.hpp")]
_ip = ctypes.POINTER(ctypes.c_int)


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(BUILD, "libmatch_harness.so")
    if _stale(out):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", out])
    L = ctypes.CDLL(out)
    vp, f = ctypes.c_void_p, ctypes.c_float
    L.mh_rect.argtypes = [f, f, f, vp, _ip]
    L.mh_capacity.argtypes = [vp, vp, vp]
    L.mh_gather.argtypes = [vp, vp, vp, vp, vp, ctypes.POINTER(LbaMatchParams), _ip, _ip, ctypes.c_int]
    L.mh_decide.argtypes = [_ip, _ip, _ip, ctypes.c_int, _ip, ctypes.POINTER(LbaMatchParams), _ip]
    L.mh_decide.restype = None
    L.mh_search.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.POINTER(LbaMatchParams)]
    L.mh_search.restype = None
    L.mh_finish.argtypes = [vp, ctypes.POINTER(LbaMatchParams), vp, vp]
    L.mh_finish.restype = None
    L.mh_rot_bin.argtypes = [f, f]
    L.mh_three_maxima.argtypes = [_ip, _ip]
    L.mh_three_maxima.restype = None
    return L


def _i(a):
    return a.ctypes.data_as(_ip)


def _record(s):
    S = np.zeros(1, MATCH_SEARCH_DTYPE)
    S["n_cam"], S["n_feat"], S["n_jobs"] = s.n_cam, len(s.feats), len(s.jobs)
    return S


@pytest.mark.parametrize("name,mode", mc.NAMES, ids=mc.IDS)
def test_rect_capacity_gather_and_decision(harness, name, mode):
    s, p, seq, _, _, cands = mc.case(name, mode)
    every = max(1, len(s.jobs) // 120)          # at most some 120 jobs of a large case
    taken = np.ascontiguousarray(s.feats["taken"], np.int32)
    for k in range(0, len(s.jobs), every):
        j = s.jobs[k:k + 1]
        out = np.zeros(4, np.int32)
        want = mo.cell_rect(j[0]["x"], j[0]["y"], j[0]["radius"], s.cams[j[0]["cam"]])
        got = harness.mh_rect(j[0]["x"], j[0]["y"], j[0]["radius"], ptr(s.cams[j[0]["cam"]:j[0]["cam"] + 1]), _i(out))
        assert (tuple(out) if got else None) == want
        cap = harness.mh_capacity(ptr(j), ptr(s.cams), ptr(s.cell_start))
        assert cap == mo.capacity(s, k)
        f, d = np.zeros(cap + 1, np.int32), np.zeros(cap + 1, np.int32)
        n = harness.mh_gather(ptr(j), ptr(s.cams), ptr(s.cell_start), ptr(s.cell_feat), ptr(s.feats), ctypes.byref(p),
                              _i(f), _i(d), cap + 1)
        assert n <= cap and list(zip(f[:n], d[:n])) == [(a, b) for a, b, _ in cands[k]]
        # the decision against the ENTRY taken state is the job run alone
        o = np.ascontiguousarray(s.feats["octave"][f[:n]], np.int32)
        res = np.zeros(4, np.int32)
        harness.mh_decide(_i(f), _i(d), _i(o), n, _i(taken), ctypes.byref(p), _i(res))
        scan = mo._scan(cands[k], [bool(t) for t in taken], p.mode)
        assert res.tolist() == [mo._decide(scan, p), scan[4], scan[0], scan[2]]


@pytest.mark.parametrize("name,mode", mc.NAMES, ids=mc.IDS)
def test_whole_search_sequentially(harness, name, mode):
    s, p, seq, _, _, _ = mc.case(name, mode)
    S, feats, jobs = _record(s), s.feats.copy(), s.jobs.copy()
    feats["job"], jobs["feat"], jobs["status"] = 77, 77, 77
    harness.mh_search(ptr(S), ptr(s.cams), ptr(s.cell_start), ptr(s.cell_feat), ptr(feats), ptr(jobs), ctypes.byref(p))
    for k in ("feat", "status", "best_dist", "best_dist2"):
        assert (jobs[k] == getattr(seq, k)).all(), k
    assert (feats["job"] == seq.job).all()
    assert S[0]["n_matches"] == seq.n_matches and S[0]["n_matches_mono"] == seq.n_matches_mono


@pytest.mark.parametrize("name", ["rot_two_bins", "rot_three_bins", "rot_bin_wrap", "generated"])
def test_rotation_pass(harness, name):
    s, p, seq, _, _, _ = mc.case(name, MATCH_BEST)
    # from the decisions before the rotation pass
    S, feats, jobs = _record(s), s.feats.copy(), s.jobs.copy()
    jobs["status"] = np.where(seq.status == MATCH_ROT, MATCH_OK, seq.status)
    jobs["feat"] = seq.feat
    feats["job"] = -1
    for k in np.flatnonzero(jobs["status"] == MATCH_OK):
        feats["job"][jobs["feat"][k]] = k
    harness.mh_finish(ptr(S), ctypes.byref(p), ptr(jobs), ptr(feats))
    assert (jobs["status"] == seq.status).all() and (feats["job"] == seq.job).all() and S[0]["n_matches"] == seq.n_matches
    for j in s.jobs[:40]:
        for f in s.feats[:5]:
            assert harness.mh_rot_bin(j["angle"], f["angle"]) == mo.rot_bin(j["angle"], f["angle"])
    rng = np.random.default_rng(3)
    for _ in range(200):
        h = np.ascontiguousarray(rng.integers(0, rng.integers(2, 40), 30), np.int32)
        out = np.zeros(3, np.int32)
        harness.mh_three_maxima(_i(h), _i(out))
        assert tuple(out) == mo.three_maxima(h)


def test_sanitized_harness_runs_clean():
    """address and undefined-behaviour sanitizers on the stand-alone program (its own main): a host build"""
    out = os.path.join(BUILD, "match_harness_san")
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the harness")
    if _stale(out):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DMATCH_HARNESS_MAIN", SRC, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
