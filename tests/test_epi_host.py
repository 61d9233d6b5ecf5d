"""The product's SearchForTriangulation maths (amc-slam_amd/csrc/lba_epi_math.hpp) built for the host
(tests/native/epi_harness.cpp, g++ -O2 -ffp-contract=off) against the fp64 restatement (tests/epi_oracle.py) on the
named cases: the tables within 1e-12 relative, both gates on every eligible candidate of a settled job, and a whole
pair (idx2, dist, status identical on settled jobs, nmatches where all are settled).  The same harness is built once
more as a stand-alone program with -fsanitize=address,undefined and run (a host build; nothing is loaded into Python)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import epi_cases as ec
import epi_oracle as eo
from amc_lba.abi import EPI_ROW_DTYPE, ptr
from amc_lba.epipolar import LbaEpiParams, epi_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "epi_harness.cpp")
BUILD = os.path.join(ROOT, "tests", "native", "_build")
DEPS = [SRC, os.path.join(ROOT, "include", "amc_lba.h")] + [os.path.join(ROOT, "amc-slam_amd", "csrc", h)
                                                            for h in ("lba_epi_math.hpp", "lba_match_math.hpp", "lba_math.hpp")]
_dp = ctypes.POINTER(ctypes.c_double)


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(BUILD, "libepi_harness.so")
    if _stale(out):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", out])
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.eh_table.argtypes = [vp, vp, _dp]
    L.eh_table.restype = None
    L.eh_stereo.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float]
    L.eh_near_epipole.argtypes = [_dp, vp]
    L.eh_gate.argtypes = [_dp, vp, vp]
    L.eh_search.argtypes = [vp] * 4 + [ctypes.c_int] + [vp] * 4 + [ctypes.POINTER(LbaEpiParams), vp]
    return L


def _table(harness, c1, c2):
    tab = np.zeros(11)
    harness.eh_table(ptr(np.ascontiguousarray(c1)), ptr(np.ascontiguousarray(c2)), tab.ctypes.data_as(_dp))
    return tab


def _close(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    fin = np.isfinite(want)
    assert (np.isnan(got) == np.isnan(want)).all() and (got[~fin & ~np.isnan(want)] == want[~fin & ~np.isnan(want)]).all()
    assert (np.abs(got[fin] - want[fin]) <= 1e-12 * np.abs(want[fin])).all(), (got, want)


@pytest.mark.parametrize("name", ec.NAMES)
def test_tables_and_gates(harness, name):
    c, _, st = ec.case(name)
    for j, s in list(zip(eo.jobs_of(c), st))[:3]:
        tabs = {}
        for a in range(c.n_cam):
            for b in range(c.n_cam):
                tabs[a, b] = _table(harness, j.cams1[a:a + 1], j.cams2[b:b + 1])
                F, ep = eo.table(j.cams1[a], j.cams2[b])
                _close(tabs[a, b][:9], F.ravel())
                _close(tabs[a, b][9:], ep)
        checked = 0
        for idx1, rows in eo.candidates(j).items():
            if not s[idx1] or checked > 300:
                continue
            k1 = j.f1[idx1:idx1 + 1]
            for idx2, _, _, _, _ in rows:
                k2 = j.f2[idx2:idx2 + 1]
                tab = tabs[int(k1[0]["cam"]), int(k2[0]["cam"])]
                F, ep = tab[:9].reshape(3, 3), tab[9:]
                assert bool(harness.eh_near_epipole(tab.ctypes.data_as(_dp), ptr(k2))) == eo.near_epipole(ep, k2[0], np.float64)[0]
                assert bool(harness.eh_gate(tab.ctypes.data_as(_dp), ptr(k1), ptr(k2))) == eo.epi_gate(F, k1[0], k2[0], np.float64)[0]
                checked += 1
        for f in j.f1[:50]:
            assert bool(harness.eh_stereo(int(f["cam"]), c.n_cam, float(f["u_right"]))) == eo.is_stereo(f, c.n_cam)
    assert harness.eh_stereo(1, 2, 0.0) == 1 and harness.eh_stereo(1, 2, -0.0) == 1 and harness.eh_stereo(0, 2, 5.0) == 0
    assert harness.eh_stereo(1, 2, float("nan")) == 0 and harness.eh_stereo(1, 2, -1e-30) == 0


def search(harness, c, p):
    """the pair p of the case through epi_search_host: (rows, nmatches)"""
    P = c.pairs[p]
    n1 = int(c.ekfs[P["kf1"]]["n_feat"])
    rows = np.zeros(n1 + 1, EPI_ROW_DTYPE)
    rows["idx2"], rows["dist"], rows["status"] = 77, 77, 77
    cams = [np.ascontiguousarray(c.cams[c.kfs[k]["cam0"]:c.kfs[k]["cam0"] + c.n_cam]) for k in (P["kf1"], P["kf2"])]
    prm = epi_params(**dict(eo.PRM, **c.prm))
    n = harness.eh_search(ptr(c.ekfs[P["kf1"]:P["kf1"] + 1]), ptr(c.ekfs[P["kf2"]:P["kf2"] + 1]), ptr(cams[0]), ptr(cams[1]),
                          c.n_cam, ptr(c.feats), ptr(c.node_id), ptr(c.node_start), ptr(c.node_feat), ctypes.byref(prm),
                          ptr(rows))
    assert rows[n1]["status"] == 77          # nothing behind the pair's rows
    return rows[:n1], n


@pytest.mark.parametrize("name", ec.NAMES)
def test_whole_pair(harness, name):
    c, r64, st = ec.case(name)
    got = []
    for p in range(min(4, len(c.pairs))):      # (at most four pairs of a batch case)
        rows, n = search(harness, c, p)
        s = st[p]
        assert (rows["status"] != 77).all()
        for f, want in (("idx2", r64[p].idx2), ("dist", r64[p].dist), ("status", r64[p].status)):
            assert (rows[f][s] == want[s]).all(), (f, np.flatnonzero(s & (rows[f] != want)))
        if s.all():
            assert n == r64[p].n_matches
        got.append(eo.Result(*(rows[f].astype(np.int64) for f in ("idx2", "dist", "status")), n))
    c.prop(c, got + r64[len(got):])


def test_sanitized_harness_runs_clean():
    """address and undefined-behaviour sanitizers on the stand-alone program (its own main): a host build"""
    out = os.path.join(BUILD, "epi_harness_san")
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the harness")
    if _stale(out):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DEPI_HARNESS_MAIN", SRC, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
