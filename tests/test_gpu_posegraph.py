"""lba_posegraph_* (amc-slam_amd/csrc/lba_posegraph.hip) against the numpy restatement of OptimizeEssentialGraph's
optimisation (tests/posegraph_oracle.py, analytic Jacobians) on the cases of tests/posegraph_cases.py.

Per case, at the project's parity tolerances: the errors within 1e-8, H and b within 1e-9 relative, a damped step at
lambda = 1e-16 and at lambda = 1 within 1e-6 normwise, its trial state and chi2 within 1e-9, the final state of
optimize(20) within 1e-6 of max(1, |.|) per field, the final chi2 within 1e-6 relative, 1 <= iterations <= 20
(tests/test_posegraph_cases.py shows on the CPU that these runs are settled: a 1e-12 disturbance of H and b moves the
final state by less than 1e-7).  The parity tests print the margins they measure (pytest -s).

Without an oracle: a step at lambda = -1e9 returns LBA_E_SOLVE and writes nothing, every argument error of the header,
the dense linearisation's size limit and nothing written by a refused call, inactive and fixed vertices bitwise as
passed, a repeated run bitwise equal, a tracker that ran a larger and a smaller graph and lba_sim3_optimize bitwise
equal to a fresh one.
"""
import ctypes

import numpy as np
import pytest

import posegraph_cases as pc
import posegraph_oracle as po
from amc_lba import LbaError
from amc_lba.abi import LBA_E_ARG, LBA_E_EMPTY, LBA_E_LIMIT, LBA_E_SOLVE, ptr
from amc_lba.posegraph import PG_EDGE_DTYPE, PG_VERTEX_DTYPE, LbaPgStats, _bind, posegraph_plan_info
from amc_lba.sim3 import make_sim3_pairs
from amc_lba.track import Tracker, track_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tracker():
    t = Tracker(track_config())
    yield t
    t.close()


@pytest.fixture(scope="module")
def tracker_for(tracker):
    """name -> the tracker with the case's LM settings (the module's one where they are lba_config's defaults)."""
    made = {}

    def get(name):
        opts = pc.options(name)
        if not opts:
            return tracker
        key = tuple(sorted(opts.items()))
        if key not in made:
            made[key] = Tracker(track_config(**opts))
        return made[key]
    yield get
    for t in made.values():
        t.close()


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("name", pc.CASES)
def test_linearisation_matches_restatement(tracker, name):
    v, e, fix = pc.case(name)
    r = pc.reference_step(name, 1.0)
    err, H, b = tracker.posegraph_linearize(v, e, fix)
    g_e = float(np.abs(err - r["errors"]).max() / max(1.0, np.abs(r["errors"]).max()))
    # b = -sum J^T e: relative to the magnitude of its terms (at a minimum b itself cancels to rounding level)
    g_H, g_b = _rel(H, r["H"]), float(np.abs(b - r["b"]).max() / max(r["b_scale"], 1e-300))
    print(f"{name}: errors {g_e:.2e}  H {g_H:.2e}  b {g_b:.2e}  na {r['na']}")
    assert H.shape == r["H"].shape and g_e <= 1e-8 and g_H <= 1e-9 and g_b <= 1e-9
    assert (H == H.T).all()
    if fix:   # the sigma row and column of every block: exactly zero (plus lambda on the diagonal, none here)
        assert (H[6::7, :] == 0).all() and (H[:, 6::7] == 0).all() and (b[6::7] == 0).all()


@pytest.mark.parametrize("lam", [1e-16, 1.0])
@pytest.mark.parametrize("name", pc.CASES)
def test_damped_step_matches_restatement(tracker, name, lam):
    v, e, fix = pc.case(name)
    r = pc.reference_step(name, lam)
    ok, dx, trial, chi = tracker.posegraph_step(v, e, fix, lam)
    assert ok and r["ok"]
    # normwise, relative to the step or, where b cancels to rounding level (a converged start), to the step its
    # terms' magnitudes would give: there dx is the solve of b's rounding error and has no digits of its own
    g_dx = float(np.linalg.norm(dx - r["dx"]) / max(np.linalg.norm(r["dx"]), 1e-6 * r["dx_scale"], 1e-300))
    g_t = po.vertex_gap(trial, r["trial"])
    g_c = abs(chi - r["chi2_trial"]) / max(r["chi2_trial"], 1e-300)
    print(f"{name} lambda {lam:g}: dx {g_dx:.2e}  trial state {g_t:.2e}  trial chi2 {g_c:.2e} ({chi:.6e})")
    assert g_dx <= 1e-6
    assert g_t <= 1e-9
    assert g_c <= 1e-9 or abs(chi - r["chi2_trial"]) <= 1e-18
    if fix:
        assert (dx[6::7] == 0).all()


@pytest.mark.parametrize("name", pc.CASES)
def test_optimize_matches_restatement(tracker_for, name):
    v, e, fix = pc.case(name)
    r = pc.reference(name)
    out, st = tracker_for(name).posegraph_optimize(v.copy(), e, fix, 20, 1e-16)
    g = po.vertex_gap(out, r["v"])
    g_c = abs(st["chi2_final"] - r["chi2_final"]) / max(r["chi2_final"], 1e-300)
    print(f"{name}: final state {g:.2e}  chi2 {st['chi2_initial']:.4e} -> {st['chi2_final']:.6e} (restatement "
          f"{r['chi2_final']:.6e}, rel {g_c:.2e})  iterations GPU {st['iterations']} restatement {r['iterations']}  "
          f"trials {st['trials']} / {r['trials']}  failures {st['solve_failures']} / {r['solve_failures']}  "
          f"levels {st['levels']} launches per solve {st['launches_per_solve']}")
    assert g <= 1e-6
    assert g_c <= 1e-6 or abs(st["chi2_final"] - r["chi2_final"]) <= 1e-18
    assert 1 <= st["iterations"] <= 20
    info = posegraph_plan_info(v, e)
    assert (st["panels"], st["tiles"], st["fill_tiles"], st["levels"], st["chain"]) == tuple(
        info[k] for k in ("panels", "tiles", "fill_tiles", "levels", "chain"))
    # inactive and fixed vertices bitwise as passed; every non-output field as passed
    _, slot = po.activity(v, e)
    for i in np.flatnonzero(slot < 0):
        assert out[i].tobytes() == v[i].tobytes()
    assert out["fixed"].tobytes() == v["fixed"].tobytes()
    if fix:
        assert out["s"].tobytes() == v["s"].tobytes()
    if name == "rejecting":   # every trial of the first iteration refused: the state is untouched, lambda has grown
        assert (st["iterations"], st["trials"], st["solve_failures"], st["result"]) == (1, pc.REJECTING_TRIALS, 0, 1)
        assert st["chi2_final"] == st["chi2_initial"] and st["lambda_final"] == 1e-16 * 2 * 4 * 8
        assert po.vertex_gap(out, v) <= 1e-15      # (the quaternion comes back normalised)


def test_default_lambda_matches_restatement(tracker):
    v, e, fix = pc.case("five_active")
    r = po.optimize(v, e, fix, 20, 0.0, tau=tracker.cfg.tau)
    out, st = tracker.posegraph_optimize(v.copy(), e, fix, 20, 0.0)
    assert po.vertex_gap(out, r["v"]) <= 1e-6 and 1 <= st["iterations"] <= 20


def test_non_positive_pivot_is_a_solve_error_and_writes_nothing(tracker):
    v, e, fix = pc.case("five_active")
    na = posegraph_plan_info(v, e)["na"]
    dx, trial, chi = np.full(7 * na, 7.0), np.zeros(len(v), PG_VERTEX_DTYPE), ctypes.c_double(7.0)
    trial["s"] = 7.0
    keep = trial.copy()
    rc = _bind().lba_posegraph_step(tracker.h, ptr(v), len(v), ptr(e), len(e), fix, -1e9,
                                    dx.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ptr(trial), ctypes.byref(chi))
    assert rc == LBA_E_SOLVE
    assert (dx == 7.0).all() and trial.tobytes() == keep.tobytes() and chi.value == 7.0
    ok, _, _, _ = tracker.posegraph_step(v, e, fix, -1e9)
    assert not ok
    assert tracker.posegraph_step(v, e, fix, 1.0)[0]                 # the next valid call succeeds


def _refused(tracker, v, e, code, fix=1, iterations=20, lam=1e-16):
    keep = v.copy()
    st = LbaPgStats()
    st.iterations = 77
    rc = _bind().lba_posegraph_optimize(tracker.h, ptr(v), len(v), ptr(e) if len(e) else None, len(e), fix, iterations, lam,
                                        ctypes.byref(st))
    assert rc == code
    assert v.tobytes() == keep.tobytes() and st.iterations == 77


def test_argument_errors(tracker):
    v, e, fix = pc.case("five_active")
    L = _bind()
    st = LbaPgStats()
    assert L.lba_posegraph_optimize(None, ptr(v), len(v), ptr(e), len(e), 1, 20, 1e-16, ctypes.byref(st)) == LBA_E_ARG
    assert L.lba_posegraph_optimize(tracker.h, None, len(v), ptr(e), len(e), 1, 20, 1e-16, ctypes.byref(st)) == LBA_E_ARG
    assert L.lba_posegraph_optimize(tracker.h, ptr(v), len(v), None, len(e), 1, 20, 1e-16, ctypes.byref(st)) == LBA_E_ARG
    for field, value in (("v0", len(v)), ("v1", -1), ("s", 0.0), ("s", -1.0), ("s", np.inf), ("s", np.nan)):
        bad = e.copy()
        bad[field][2] = value
        _refused(tracker, v.copy(), bad, LBA_E_ARG)
    bad = e.copy()
    bad["v1"][1] = bad["v0"][1]
    _refused(tracker, v.copy(), bad, LBA_E_ARG)
    for value in (0.0, -2.0, np.nan, np.inf):
        bad = v.copy()
        bad["s"][3] = value
        _refused(tracker, bad, e, LBA_E_ARG)
    _refused(tracker, v.copy(), e, LBA_E_ARG, iterations=-1)
    _refused(tracker, v.copy(), e, LBA_E_ARG, lam=float("nan"))
    # no active edge: no edges at all, or every vertex fixed
    _refused(tracker, v.copy(), e[:0], LBA_E_EMPTY)
    allfixed = v.copy()
    allfixed["fixed"] = 1
    _refused(tracker, allfixed, e, LBA_E_EMPTY)
    with pytest.raises(LbaError):
        tracker.posegraph_optimize(allfixed, e)
    out, st = tracker.posegraph_optimize(v.copy(), e, fix)                # the next valid call succeeds
    assert st["iterations"] >= 1


def test_dense_linearisation_limit(tracker):
    """lba_posegraph_linearize refuses a dense H above 2048 active free vertices (LBA_E_LIMIT) and writes nothing; the
    same chain without H is served."""
    n = 2051                                                        # one fixed, 2050 active: two over the limit
    v = np.zeros(n, PG_VERTEX_DTYPE)
    v["q"][:, 3], v["s"], v["t"][:, 0], v["fixed"][0] = 1.0, 1.0, np.arange(n), 1
    e = np.zeros(n - 1, PG_EDGE_DTYPE)
    e["v0"], e["v1"], e["q"][:, 3], e["s"], e["t"][:, 0] = np.arange(1, n), np.arange(n - 1), 1.0, 1.0, -1.5
    H, b = np.full(4, 7.0), np.full(7 * (n - 1), 7.0)
    dp = ctypes.POINTER(ctypes.c_double)
    L = _bind()
    assert L.lba_posegraph_linearize(tracker.h, ptr(v), n, ptr(e), n - 1, 1, None, H.ctypes.data_as(dp),
                                     b.ctypes.data_as(dp)) == LBA_E_LIMIT
    assert (H == 7.0).all() and (b == 7.0).all()
    assert L.lba_posegraph_linearize(tracker.h, ptr(v), n, ptr(e), n - 1, 1, None, None, b.ctypes.data_as(dp)) == n - 1
    # every edge is 0.5 m short along x: the two terms of an inner vertex cancel, the last vertex keeps its one
    bb = b.reshape(-1, 7)
    assert np.abs(bb[:-1]).max() <= 1e-15 and abs(bb[-1, 3] - 0.5) <= 1e-15 and np.abs(np.delete(bb[-1], 3)).max() <= 1e-15


def test_repeated_and_fresh_tracker_runs_are_bitwise_equal(tracker):
    v, e, fix = pc.case("loop150")
    first, st1 = tracker.posegraph_optimize(v.copy(), e, fix)
    again, st2 = tracker.posegraph_optimize(v.copy(), e, fix)
    assert first.tobytes() == again.tobytes() and st1 == st2
    # a larger and a smaller graph, and another entry point that shares the tracker, in between
    vh, eh, fh = pc.case("hub")
    vs, es, fs = pc.case("two_one")
    small, _ = tracker.posegraph_optimize(vs.copy(), es, fs)
    hub, _ = tracker.posegraph_optimize(vh.copy(), eh, fh)
    pairs, corr, cams, _ = make_sim3_pairs(n_pairs=2, n_corr=30, seed=3)
    tracker.sim3_optimize(pairs, corr, cams, 4)
    third, st3 = tracker.posegraph_optimize(v.copy(), e, fix)
    assert third.tobytes() == first.tobytes() and st3 == st1
    fresh = Tracker(track_config())
    try:
        other, st4 = fresh.posegraph_optimize(v.copy(), e, fix)
        small2, _ = fresh.posegraph_optimize(vs.copy(), es, fs)
        hub2, _ = fresh.posegraph_optimize(vh.copy(), eh, fh)
    finally:
        fresh.close()
    assert other.tobytes() == first.tobytes() and st4 == st1
    assert small2.tobytes() == small.tobytes() and hub2.tobytes() == hub.tobytes()
    step1 = tracker.posegraph_step(v, e, fix, 1.0)
    step2 = tracker.posegraph_step(v, e, fix, 1.0)
    assert step1[1].tobytes() == step2[1].tobytes() and step1[2].tobytes() == step2[2].tobytes() and step1[3] == step2[3]
