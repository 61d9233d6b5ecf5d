"""The cases of tests/posegraph_cases.py on the CPU: each has the property it is there for (shown with
lba_posegraph_plan_info, which needs no device, and with the restatement tests/posegraph_oracle.py), and under
fix_scale = 1 each meets the conditions under which the GPU tolerances of tests/test_gpu_posegraph.py mean something:

 1. the analytic run's final state moves by at most 1e-7 when H and b are disturbed by 1e-12 relative;
 2. the reference-faithful numeric-Jacobian run and the analytic run end within 5e-7 of each other.

Iteration and trial counts are printed, not compared: near the minimum the gain ratio's sign is rounding.  Under
fix_scale = 0 the gap to the numeric run is printed only.  Measured values:
profiles/posegraph_margins.log."""
import numpy as np
import pytest

import posegraph_cases as pc
import posegraph_oracle as po
from amc_lba.posegraph import posegraph_plan_info


def _errors(name):
    v, e, fix = pc.case(name)
    G = po.Graph(v, e, fix)
    return G, G.errors(G.states())


@pytest.mark.parametrize("name", pc.FIXED_SCALE_CASES)
def test_fixed_scale_case_is_settled(name):
    a = pc.reference(name)
    p = pc.reference(name, seed=1)
    n = pc.reference(name, jac="numeric")
    g_p, g_n = po.vertex_gap(p["v"], a["v"]), po.vertex_gap(n["v"], a["v"])
    print(f"{name}: disturbed {g_p:.2e}  numeric vs analytic {g_n:.2e}  chi2 {a['chi2_initial']:.3e} -> {a['chi2_final']:.3e}  "
          f"iterations / rejected: analytic {a['iterations']} / {a['rejected']}  disturbed {p['iterations']} / {p['rejected']}  "
          f"numeric {n['iterations']} / {n['rejected']}")
    assert g_p <= 1e-7
    assert g_n <= 5e-7
    assert a["chi2_final"] <= a["chi2_initial"]


@pytest.mark.parametrize("name", [n for n in pc.CASES if n not in pc.FIXED_SCALE_CASES])
def test_free_scale_case_gap_is_reported(name):
    a = pc.reference(name)
    p = pc.reference(name, seed=1)
    n = pc.reference(name, jac="numeric")
    print(f"{name}: disturbed {po.vertex_gap(p['v'], a['v']):.2e}  numeric vs analytic (reported) "
          f"{po.vertex_gap(n['v'], a['v']):.2e}  iterations / rejected: analytic {a['iterations']} / {a['rejected']}  "
          f"numeric {n['iterations']} / {n['rejected']}")
    assert po.vertex_gap(p["v"], a["v"]) <= 1e-7
    assert a["chi2_final"] <= a["chi2_initial"]


def test_sizes_at_the_panel_boundary():
    assert posegraph_plan_info(*pc.case("two_one")[:2])["na"] == 1
    i4, i5 = (posegraph_plan_info(*pc.case(n)[:2]) for n in ("four_active", "five_active"))
    assert (i4["na"], i4["panels"]) == (4, 1) and (i5["na"], i5["panels"]) == (5, 2)


def test_activity_cases():
    v, e, _ = pc.case("isolated_and_fixed_pair")
    ea, slot = po.activity(v, e)
    assert not ea[5] and ea.sum() == len(e) - 1                     # the edge between the fixed 0 and 4
    assert slot[6] == -1 and not v["fixed"][6]                      # the isolated vertex
    assert posegraph_plan_info(v, e)["na"] == 5 == int((slot >= 0).sum())
    v, e, _ = pc.case("fixed_middle")
    assert v["fixed"][4] and v["fixed"].sum() == 1 and posegraph_plan_info(v, e)["na"] == 8
    v, e, _ = pc.case("two_fixed")
    assert v["fixed"].sum() == 2 and posegraph_plan_info(v, e)["na"] == 7


def test_parallel_reversed_and_hub():
    v, e, _ = pc.case("parallel_reversed")
    pairs = list(zip(e["v0"].tolist(), e["v1"].tolist()))
    assert pairs.count((5, 1)) == 2 and (3, 2) in pairs and (2, 3) in pairs
    assert len(set(pairs)) < len(pairs)
    v, e, _ = pc.case("hub")
    assert int(((e["v0"] == 1) | (e["v1"] == 1)).sum()) >= 40


def test_zero_error_and_far_and_branches():
    _, err = _errors("zero_error")
    assert (err[:-1] == 0).all() and err[-1].any()                   # exactly zero, and the closing edge is not
    _, err = _errors("far")
    assert np.linalg.norm(err[:, :3], axis=1).max() > 1.0 and np.linalg.norm(err[:, 3:6], axis=1).max() > 30.0
    for name, want in (("log_branches", {0, 1}), ("log_branches_free", {0, 1, 2, 3})):
        v, e, fix = pc.case(name)
        G = po.Graph(v, e, fix)
        # at the truth (the fixed vertex and the measurements define it) the edges' errors are the chosen noises
        S = G.states()
        got = {po.log_coeffs(G.C[k] * S[int(ed["v0"])] * S[int(ed["v1"])].inverse())[0] for k, ed in enumerate(e)}
        ref = pc.reference(name)
        Sf = G.states(ref["v"])
        got |= {po.log_coeffs(G.C[k] * Sf[int(ed["v0"])] * Sf[int(ed["v1"])].inverse())[0] for k, ed in enumerate(e)}
        print(f"{name}: branches of Sim3::log met at the start and the end {sorted(got)}")
        assert got >= want


def test_loop_graph_plan():
    v, e, _ = pc.case("loop150")
    info = posegraph_plan_info(v, e)
    print(f"loop150: {info}")
    assert 140 <= info["na"] <= 160
    assert info["levels"] >= 3 and info["tail"] >= 1 and info["fill_tiles"] >= 1
    assert info["chain"] < info["panels"]


def test_rejecting_and_converged_starts():
    v, e, fix = pc.case("rejecting")
    for kw in (dict(), dict(seed=1), dict(jac="numeric")):
        r = pc.reference("rejecting", **kw)
        assert (r["iterations"], r["rejected"], r["solve_failures"]) == (1, pc.REJECTING_TRIALS, 0)
        assert r["v"].tobytes() == v.tobytes() and r["chi2_final"] == r["chi2_initial"]
    assert po.optimize(v, e, fix, 1, 1e-16)["rejected"] >= 9      # and with lba_config's ten trials: nine refused
    r = pc.reference("converged")
    v, e, _ = pc.case("converged")
    assert po.vertex_gap(r["v"], v) <= 1e-9 and r["chi2_final"] <= r["chi2_initial"]


@pytest.mark.slow
def test_rejecting_seed_is_the_search_result():
    assert pc.search_rejecting() == pc.REJECTING_SEED
