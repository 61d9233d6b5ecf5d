"""MapPoint's refresh (amc-slam_amd/csrc/lba_mp_math.hpp) built for the host with g++ -O2 -ffp-contract=off
(tests/native/mp_harness.cpp) against the numpy restatement (tests/mp_oracle.py) on the named cases and the generated
batches: every field BIT-IDENTICAL (a NaN matching a NaN), with the descriptor chosen by the matrix and std::sort and
once more by the bisection the kernels run.  The same harness is built once more as a stand-alone program with
-fsanitize=address,undefined and run (a host build; nothing is loaded into Python)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import mp_cases as mc
import mp_oracle as mo
from amc_lba.abi import ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "mp_harness.cpp")
BUILD = os.path.join(ROOT, "tests", "native", "_build")
DEPS = [SRC, os.path.join(ROOT, "include", "amc_lba.h")] + [
    os.path.join(ROOT, "amc-slam_amd", "csrc", h) for h in ("lba_mp_math.hpp", "lba_match_math.hpp", "lba_math.hpp")]


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


def load_harness():
    out = os.path.join(BUILD, "libmp_harness.so")
    if _stale(out):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", out])
    L = ctypes.CDLL(out)
    vp, i = ctypes.c_void_p, ctypes.c_int
    L.mh_refresh.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, ctypes.c_float, i]
    L.mh_refresh.restype = None
    return L


@pytest.fixture(scope="module")
def harness():
    return load_harness()


def host_refresh(L, points, obs, K, kf_bad=None, bisect=False):
    """the header's sequential loop on a batch; the inputs are left as they are"""
    out = points.copy()
    bad = None if kf_bad is None else np.ascontiguousarray(kf_bad, np.int32)
    L.mh_refresh(ptr(out), len(out), ptr(obs), ptr(K.kfs), ptr(K.ekfs), ptr(K.cams), ptr(K.feats),
                 None if bad is None else ptr(bad), float(K.scale_top), int(bisect))
    return out


@pytest.mark.parametrize("bisect", (False, True), ids=("sort", "bisect"))
@pytest.mark.parametrize("name", [n for n in mc.NAMES if not mc.case(n).refused])
def test_cases_identical(harness, name, bisect):
    c = mc.case(name)
    got = host_refresh(harness, c.points, c.obs, c.K, c.kf_bad, bisect)
    assert mo.diff_fields(got, mc.reference(name)) == []


@pytest.mark.parametrize("first", range(0, len(mc.SEEDS), 50))
def test_generated_batches_identical(harness, first):
    for seed in range(first, first + 50):
        p = mc.problem(seed)
        want = mo.refresh_batch(p.points, p.obs, p.K, p.kf_bad)
        for bisect in (False, True):
            got = host_refresh(harness, p.points, p.obs, p.K, p.kf_bad, bisect)
            assert mo.diff_fields(got, want) == [], (seed, bisect)


def test_sanitized_harness_runs_clean():
    """address and undefined-behaviour sanitizers on the stand-alone program (its own main): a host build"""
    out = os.path.join(BUILD, "mp_harness_san")
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the harness")
    if _stale(out):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DMP_HARNESS_MAIN", SRC, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
