"""The named cases of lba_sim3_ransac (tests/sim3_ransac_cases.py) on the CPU: each case has its property on the
fp64 restatement; the settledness caps hold (at most 1 % of the (hypothesis, row) flags within M_GATE of a gate, at
most 10 % of the transforms with an eigen-gap below 1e-6, every selection settled); and the reference-faithful float32
run agrees with the fp64 run, which the device is held to, on every settled flag and every settled selection, with
S12 apart by float rounding times the conditioning of a three-point fit (reported; held to S12_F32_BOUND)."""
import numpy as np
import pytest

import sim3_ransac_cases as rc
import sim3_ransac_oracle as ro


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_property_and_caps(name):
    c, r64, _ = rc.case(name)
    c.check(r64)
    for p, res in enumerate(r64):
        flag_ok, transform_ok, sel_ok = ro.settled(res, c.pairs[p], rc.M_GATE, rc.GAP_MIN)
        live = ~(res["degenerate"] | res["nonfinite"])
        n_flags = max(1, flag_ok.size)
        unsettled_t = int((live & ~transform_ok).sum())
        print(f"{name}[{p}]: {flag_ok.shape} flags, unsettled {int((~flag_ok).sum())}; transforms unsettled {unsettled_t} of "
              f"{int(live.sum())}; smallest gap {np.min(res['gap'][live]) if live.any() else float('nan'):.2e}; selection settled {sel_ok}")
        assert (~flag_ok).sum() <= 0.01 * n_flags
        assert unsettled_t <= 0.10 * max(1, int(live.sum()))
        assert sel_ok


@pytest.mark.parametrize("name", rc.NAMES)
def test_float32_run_agrees_where_settled(name):
    c, r64, r32 = rc.case(name)
    for p, (a, b) in enumerate(zip(r64, r32)):
        flag_ok, transform_ok, sel_ok = ro.settled(a, c.pairs[p], rc.M_GATE, rc.GAP_MIN)
        same_kind = a["degenerate"] == b["degenerate"]
        assert same_kind.all()
        assert (a["inlier"] == b["inlier"])[flag_ok].all()
        unsettled = (~flag_ok).sum(1)
        assert (np.abs(a["count"] - b["count"]) <= unsettled).all()
        if sel_ok:
            assert (a["best_hyp"], a["converged"]) == (b["best_hyp"], b["converged"])
        gap = rc.s12_gap(b, a)[transform_ok]
        if gap.size:
            print(f"{name}[{p}]: float32 vs fp64 S12 of {gap.size} settled transforms: worst {gap.max():.2e}")
            assert gap.max() <= rc.S12_F32_BOUND


def test_margin_covers_the_measured_disagreement():
    worst = 0.0
    for name in rc.NAMES:
        c, r64, r32 = rc.case(name)
        for p, (a, b) in enumerate(zip(r64, r32)):
            worst = max(worst, rc.disagreement(a, b, c.pair_inputs(p)[1]))
    print(f"largest gate margin with a float32 / fp64 disagreement: {worst:.3e}; M_GATE {rc.M_GATE:.1e}")
    assert 4 * worst <= rc.M_GATE
