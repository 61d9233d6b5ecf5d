"""The product's SearchByBoW maths (amc-slam_amd/csrc/lba_bow_math.hpp) built for the host
(tests/native/bow_harness.cpp, g++ -O2 -ffp-contract=off) against the restatement (tests/bow_oracle.py: `sequential`):
a whole pair IDENTICAL in idx2, dist, dist2, status and nmatches on every named case, on generator seeds and in both
overloads; the merge of two partial scans associative, commutative and equal to the scan on random splits; the accept
test on all 257 x 257 (b1, b2) at the ratios in use.  The same harness is built once more as a stand-alone program
with -fsanitize=address,undefined and run (a host build; nothing is loaded into Python)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import bow_cases as bc
import bow_oracle as bo
from amc_lba.abi import BOW_ROW_DTYPE, ptr
from amc_lba.bow import LbaBowParams, bow_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "bow_harness.cpp")
BUILD = os.path.join(ROOT, "tests", "native", "_build")
DEPS = [SRC, os.path.join(ROOT, "include", "amc_lba.h")] + [os.path.join(ROOT, "amc-slam_amd", "csrc", h)
                                                            for h in ("lba_bow_math.hpp", "lba_match_math.hpp", "lba_math.hpp")]
_ip = ctypes.POINTER(ctypes.c_int)


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(BUILD, "libbow_harness.so")
    if _stale(out):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", out])
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.bh_fold_list.argtypes = [vp, vp, ctypes.c_int, vp]
    L.bh_fold_list.restype = None
    L.bh_merge.argtypes = [vp, vp, vp]
    L.bh_merge.restype = None
    L.bh_accept.argtypes = [ctypes.c_int] * 4 + [ctypes.c_float]
    L.bh_search.argtypes = [vp] * 6 + [ctypes.POINTER(LbaBowParams), vp]
    return L


def search(harness, c, p):
    """the pair p of the case through bow_search_host: a Result"""
    P = c.pairs[p]
    n1 = int(c.ekfs[P["kf1"]]["n_feat"])
    rows = np.full(4 * (n1 + 1), 77, np.int32).view(BOW_ROW_DTYPE)
    prm = bow_params(**dict(bo.PRM, **c.prm))
    n = harness.bh_search(ptr(c.ekfs[P["kf1"]:P["kf1"] + 1]), ptr(c.ekfs[P["kf2"]:P["kf2"] + 1]), ptr(c.feats), ptr(c.node_id),
                          ptr(c.node_start), ptr(c.node_feat), ctypes.byref(prm), ptr(rows))
    assert rows[n1]["status"] == 77          # nothing behind the pair's rows
    r = rows[:n1]
    return bo.Result(*(r[f].astype(np.int64) for f in ("idx2", "dist", "dist2", "status")), n)


@pytest.mark.parametrize("mode", bc.MODES, ids=bc.MODE_NAMES.get)
@pytest.mark.parametrize("name", bc.NAMES)
def test_whole_pair_identical(harness, name, mode):
    c, seq = bc.case(name, mode)
    got = [search(harness, c, p) for p in range(len(c.pairs))]
    for g, s in zip(got, seq):
        assert bo.same(g, s), (name, bo.rows_differing(g, s))
    c.prop(c, got)


def test_whole_pair_identical_on_seeds(harness):
    for seed in range(40):
        prm = dict(nn_ratio=(0.9, 0.7, 0.6, 0.8)[seed % 4], check_orientation=seed % 3 != 0, th_low=(50, 50, 30)[seed % 3])
        knobs = dict(bc.VARIANT_GEN if seed % 4 > 1 else {}, n_feat=80 + seed, n_nodes=3 + seed % 5, cluster=1 + seed % 5)
        c = bc.generated(2, 2000 + seed, bc.MODES[seed % 2], prm, **knobs)
        for p, j in enumerate(bo.jobs_of(c)):
            assert bo.same(search(harness, c, p), bo.sequential(j)), seed


def _i3(v=(0, 0, 0)):
    return np.array(v, np.int32)


def _fold(harness, dist, pos):
    out = _i3()
    d, p = np.ascontiguousarray(dist, np.int32), np.ascontiguousarray(pos, np.int32)
    harness.bh_fold_list(ptr(d), ptr(p), len(d), ptr(out))
    return out


def _merge(harness, a, b):
    out = _i3()
    harness.bh_merge(ptr(_i3(a)), ptr(_i3(b)), ptr(out))
    return out


def test_merge_is_associative_and_equals_the_scan(harness):
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(0, 150))
        # few distinct values, so the minimum and the second are often tied; some candidates at 256
        dist = np.where(rng.random(n) < 0.2, 256, rng.integers(0, 6, n) * 37)
        pos = np.arange(n)
        whole = _fold(harness, dist, pos)
        if n and dist.min() < 256:
            two = np.sort(np.concatenate([dist, [256]]))[:2]
            assert whole.tolist() == [two[0], int(np.argmin(dist)), two[1]]
        else:
            assert whole.tolist() == [256, 0xffff, 256]
        # dealt to lanes as the kernel deals them, and cut into three contiguous parts
        lanes = int(rng.integers(1, 65))
        parts = [_fold(harness, dist[l::lanes], pos[l::lanes]) for l in range(lanes)]
        acc = parts[0]
        for k in rng.permutation(np.arange(1, lanes)):
            acc = _merge(harness, acc, parts[k]) if rng.random() < 0.5 else _merge(harness, parts[k], acc)
        assert acc.tolist() == whole.tolist(), trial
        c1, c2 = sorted(rng.integers(0, n + 1, 2))
        a, b, c = (_fold(harness, dist[s], pos[s]) for s in (slice(0, c1), slice(c1, c2), slice(c2, n)))
        left, right = _merge(harness, _merge(harness, a, b), c), _merge(harness, a, _merge(harness, b, c))
        assert left.tolist() == right.tolist() == whole.tolist(), trial
        assert _merge(harness, c, _merge(harness, b, a)).tolist() == whole.tolist(), trial


def test_accept_on_every_pair_of_distances(harness):
    for mode in bc.MODES:
        for ratio in (0.9, 0.7, 0.6, 0.8, 0.75):
            prm = dict(mode=mode, th_low=50, nn_ratio=ratio)
            for b1 in list(range(0, 60)) + [255, 256]:
                for b2 in range(b1, 257):
                    assert harness.bh_accept(b1, b2, mode, 50, ratio) == bo.accept(b1, b2, prm), (mode, ratio, b1, b2)
    # the pairs the double product would accept
    assert harness.bh_accept(3, 5, bo.KF, 50, 0.6) == bo.RATIO and harness.bh_accept(4, 5, bo.KF, 50, 0.8) == bo.RATIO
    assert harness.bh_accept(50, 256, bo.KF, 50, 0.9) == bo.NO_CAND and harness.bh_accept(50, 256, bo.FRAME, 50, 0.9) == bo.OK


def test_sanitized_harness_runs_clean():
    """address and undefined-behaviour sanitizers on the stand-alone program (its own main): a host build"""
    out = os.path.join(BUILD, "bow_harness_san")
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the harness")
    if _stale(out):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DBOW_HARNESS_MAIN", SRC, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
