"""lba_posegraph_* (amc-slam_amd/csrc/lba_posegraph.hip) against the numpy restatement (tests/posegraph_oracle.py,
analytic Jacobians) on the graphs of tests/posegraph_topology_cases.py: chains and trees, grids, complete graphs, laps,
random connected graphs, several components, and array orders unrelated to the graph order.  The elimination structure
of the tile Cholesky (the plan, the levels, the per-tile update lists) is decided by the graph alone, and only the
result shows a wrong list: these cases take it to 30 levels, 493 tiles of which half are fill-in, dense systems and
panels that hold vertices of different components (tests/test_posegraph_topology_cases.py shows that on the CPU, and
that the runs are settled).

Per case, at the tolerances of tests/test_gpu_posegraph.py: the errors within 1e-8, H and b within 1e-9 relative, a
damped step at lambda = 1e-16 and at lambda = 1 within 1e-6 normwise and per entry within 1e-6 of |dx|_inf, its trial
state and chi2 within 1e-9, the step's normwise backward error on the restatement's system at most 1e-12 (the bound of
tests/test_gpu_configs.py; scipy's Cholesky on the same system, 1e-17 to 1e-16, is printed beside it), the final state
of optimize(20) within 1e-6 and its chi2 within 1e-6 relative.  A relabelled graph gives the same step and the same
final state within 2e-6 (two plans of one system compared directly), and a tracker that ran graphs of 176, 28 and 493
tiles in between repeats its first run bitwise.  `floating` (a component without a fixed vertex) is stepped at
lambda = 1 only.  The parity tests print the margins they measure (pytest -s).
"""
import numpy as np
import pytest

import posegraph_oracle as po
import posegraph_topology_cases as tc
from amc_lba.posegraph import posegraph_plan_info
from amc_lba.track import Tracker, track_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tracker():
    t = Tracker(track_config())
    yield t
    t.close()


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def backward_error(H, lam, b, dx, fix):
    """|r|_inf / (|A|_inf |dx|_inf + |b|_inf) with A = H + lambda I, r = A dx - b, in long double; under fix_scale on
    the six free dofs of every vertex (the sigma rows and columns of H are zero and dx's sigma entries are set to 0)."""
    keep = np.arange(len(b)) % 7 != 6 if fix else np.ones(len(b), bool)
    A = (H + lam * np.eye(len(b)))[np.ix_(keep, keep)].astype(np.longdouble)
    x, rhs = dx[keep].astype(np.longdouble), b[keep].astype(np.longdouble)
    r = A @ x - rhs
    return float(np.abs(r).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(rhs).max()))


@pytest.mark.parametrize("name", tc.SOLVED_CASES)
def test_linearisation_matches_restatement(tracker, name):
    v, e, fix = tc.case(name)
    r = tc.reference_step(name, 1.0)
    err, H, b = tracker.posegraph_linearize(v, e, fix)
    g_e = float(np.abs(err - r["errors"]).max() / max(1.0, np.abs(r["errors"]).max()))
    # b = -sum J^T e: relative to the magnitude of its terms (at a minimum b itself cancels to rounding level)
    g_H, g_b = _rel(H, r["H"]), float(np.abs(b - r["b"]).max() / max(r["b_scale"], 1e-300))
    print(f"{name}: errors {g_e:.2e}  H {g_H:.2e}  b {g_b:.2e}  na {r['na']}")
    assert H.shape == r["H"].shape and g_e <= 1e-8 and g_H <= 1e-9 and g_b <= 1e-9
    assert (H == H.T).all()
    if fix:   # the sigma row and column of every block: exactly zero (plus lambda on the diagonal, none here)
        assert (H[6::7, :] == 0).all() and (H[:, 6::7] == 0).all() and (b[6::7] == 0).all()


STEPS = [(n, lam) for n in tc.SOLVED_CASES for lam in (1e-16, 1.0)] + [("floating", 1.0)]


@pytest.mark.parametrize("name,lam", STEPS)
def test_damped_step_matches_restatement(tracker, name, lam):
    v, e, fix = tc.case(name)
    r = tc.reference_step(name, lam)
    ok, dx, trial, chi = tracker.posegraph_step(v, e, fix, lam)
    assert ok and r["ok"]
    # normwise, relative to the step or, where b cancels to rounding level, to the step its terms' magnitudes would give
    g_dx = float(np.linalg.norm(dx - r["dx"]) / max(np.linalg.norm(r["dx"]), 1e-6 * r["dx_scale"], 1e-300))
    g_entry = float(np.abs(dx - r["dx"]).max() / np.abs(r["dx"]).max())
    g_t = po.vertex_gap(trial, r["trial"])
    g_c = abs(chi - r["chi2_trial"]) / max(r["chi2_trial"], 1e-300)
    w = backward_error(r["H"], lam, r["b"], dx, fix)
    w_ref = backward_error(r["H"], lam, r["b"], r["dx"], fix)
    print(f"{name} lambda {lam:g}: dx {g_dx:.2e}  worst entry / |dx|_inf {g_entry:.2e}  trial state {g_t:.2e}  trial chi2 "
          f"{g_c:.2e} ({chi:.6e})  backward error {w:.2e} (scipy's Cholesky {w_ref:.2e})")
    assert g_dx <= 1e-6
    assert (np.abs(dx - r["dx"]) <= 1e-6 * np.abs(r["dx"]).max()).all()
    assert g_t <= 1e-9
    assert g_c <= 1e-9 or abs(chi - r["chi2_trial"]) <= 1e-18
    assert w <= 1e-12
    if fix:
        assert (dx[6::7] == 0).all()


@pytest.mark.parametrize("name", tc.SOLVED_CASES)
def test_optimize_matches_restatement(tracker, name):
    v, e, fix = tc.case(name)
    r = tc.reference(name)
    out, st = tracker.posegraph_optimize(v.copy(), e, fix, 20, 1e-16)
    g = po.vertex_gap(out, r["v"])
    g_c = abs(st["chi2_final"] - r["chi2_final"]) / max(r["chi2_final"], 1e-300)
    print(f"{name}: final state {g:.2e}  chi2 {st['chi2_initial']:.4e} -> {st['chi2_final']:.6e} (restatement "
          f"{r['chi2_final']:.6e}, rel {g_c:.2e})  iterations GPU {st['iterations']} restatement {r['iterations']}  "
          f"trials {st['trials']} / {r['trials']}  failures {st['solve_failures']} / {r['solve_failures']}  "
          f"tiles {st['tiles']} fill {st['fill_tiles']} levels {st['levels']} launches per solve {st['launches_per_solve']}")
    assert g <= 1e-6
    assert g_c <= 1e-6 or abs(st["chi2_final"] - r["chi2_final"]) <= 1e-18
    assert 1 <= st["iterations"] <= 20
    info = posegraph_plan_info(v, e)
    assert (st["panels"], st["tiles"], st["fill_tiles"], st["levels"], st["chain"]) == tuple(
        info[k] for k in ("panels", "tiles", "fill_tiles", "levels", "chain"))
    assert st["launches_per_solve"] == 1 + 2 * info["levels"]
    # inactive and fixed vertices bitwise as passed; every non-output field as passed
    _, slot = po.activity(v, e)
    assert (slot < 0).sum() == v["fixed"].sum() >= 1
    for i in np.flatnonzero(slot < 0):
        assert out[i].tobytes() == v[i].tobytes()
    assert out["fixed"].tobytes() == v["fixed"].tobytes()
    if fix:
        assert out["s"].tobytes() == v["s"].tobytes()


@pytest.mark.parametrize("permuted,plain", tc.RELABELLED)
def test_relabelled_graph_gives_the_same_step_and_state(tracker, permuted, plain):
    """The permuted case is the plain one under another labelling (the same truth, start and measurements), eliminated
    by another plan: mapped back, the two steps at lambda = 1 agree within 2e-6 normwise, each being within 1e-6 of the
    same restatement step, and so do the two final states."""
    v, e, fix = tc.case(plain)
    vp, ep, _ = tc.case(permuted)
    p = tc.permutation(len(v))
    _, slot = po.activity(v, e)
    _, slot_p = po.activity(vp, ep)
    act = np.flatnonzero(slot >= 0)
    assert (slot_p[p[act]] >= 0).all() and (slot_p >= 0).sum() == len(act)
    src = (7 * slot_p[p[act]][:, None] + np.arange(7)).ravel()      # where the plain order's entries are in dx_p
    ok, dx, trial, chi = tracker.posegraph_step(v, e, fix, 1.0)
    ok_p, dx_p, trial_p, chi_p = tracker.posegraph_step(vp, ep, fix, 1.0)
    assert ok and ok_p
    g_dx = float(np.linalg.norm(dx_p[src] - dx) / np.linalg.norm(dx))
    g_t = po.vertex_gap(trial_p[p], trial)
    out, st = tracker.posegraph_optimize(v.copy(), e, fix, 20, 1e-16)
    out_p, st_p = tracker.posegraph_optimize(vp.copy(), ep, fix, 20, 1e-16)
    g = po.vertex_gap(out_p[p], out)
    print(f"{permuted} vs {plain}: tiles {st_p['tiles']} / {st['tiles']}  levels {st_p['levels']} / {st['levels']}  "
          f"step at lambda 1: dx {g_dx:.2e}  trial state {g_t:.2e}  trial chi2 {abs(chi_p - chi) / chi:.2e}  "
          f"final state {g:.2e}  iterations {st_p['iterations']} / {st['iterations']}")
    assert st_p["tiles"] > st["tiles"] and st_p["levels"] > st["levels"]
    assert g_dx <= 2e-6
    assert g_t <= 2e-9 and abs(chi_p - chi) <= 2e-9 * chi
    assert g <= 2e-6


def test_reuse_across_very_different_plans(tracker):
    """The arena grows and shrinks with the tile count (176, 28, 493, 176): the second run of the 12 x 12 grid is
    bitwise the first and a fresh tracker's."""
    runs = {}
    tiles = []
    for name in ("grid12x12", "complete26", "grid12x12_permuted", "grid12x12"):
        v, e, fix = tc.case(name)
        out, st = tracker.posegraph_optimize(v.copy(), e, fix, 20, 1e-16)
        step = tracker.posegraph_step(v, e, fix, 1.0)
        tiles.append(st["tiles"])
        runs.setdefault(name, []).append((out, st, step))
    assert tiles[0] == tiles[3] and tiles[1] * 4 < tiles[0] and tiles[2] > 2 * tiles[0]
    fresh = Tracker(track_config())
    try:
        v, e, fix = tc.case("grid12x12")
        out, st = fresh.posegraph_optimize(v.copy(), e, fix, 20, 1e-16)
        runs["grid12x12"].append((out, st, fresh.posegraph_step(v, e, fix, 1.0)))
    finally:
        fresh.close()
    first = runs["grid12x12"][0]
    for out, st, step in runs["grid12x12"][1:]:
        assert out.tobytes() == first[0].tobytes() and st == first[1]
        assert step[0] and step[1].tobytes() == first[2][1].tobytes() and step[2].tobytes() == first[2][2].tobytes()
        assert step[3] == first[2][3]
