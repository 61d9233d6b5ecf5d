"""The named cases of lba_triangulate (tests/tri_cases.py) on the CPU: each case has its property; its rows are
settled; the float32-faithful restatement (the reference's precision) and the fp64 one (what the device is held to)
give the same status wherever no comparison lies within M_F32 of its gate (tests/tri_cases.py: per gate quantity, 4 x
the measured difference of the two runs); at most 10 % of a case's rows may lie inside it.

A row is settled when every comparison evaluated for it in fp64 has |lhs - rhs| > 1e-9 max(|lhs|, |rhs|); at most 2 %
of a case's rows may be unsettled.  That is a condition on the inputs: rounding order times the null vector's
conditioning, u kappa <= 1e-11, stays two orders inside it.  Two cases stand outside the rule and say why:
`rank_deficient` (reported, not compared) and `dist_zero` (exact binary arithmetic ON the gate)."""
import numpy as np
import pytest

import tri_cases as tc
import tri_oracle as to


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_has_its_property(name):
    c, r64, _ = tc.case(name)
    c.check(c, r64)
    m = c.in_pairs()
    assert (r64.status[m] >= 0).all() and (r64.status[~m] == -1).all()
    for p, P in enumerate(c.pairs):
        assert 0 <= r64.n_stereo[p] <= r64.n_new[p] <= P["n_rows"]


def test_every_status_has_a_case():
    for status, name in tc.STATUS_CASES.items():
        c, r64, r32 = tc.case(name)
        m = c.in_pairs()
        assert (r64.status[m] == status).any() and (r32.status[m] == status).any(), (status, name)
    # LBA_TRI_W_ZERO is held by tests/test_tri_math_host.py: no keypoints reach it through float inputs
    assert to.W_ZERO not in tc.STATUS_CASES


@pytest.mark.parametrize("name", tc.NAMES)
def test_rows_are_settled(name):
    assert to.SETTLED == 1e-9
    c, r64, _ = tc.case(name)
    if c.reported or c.exact:
        return
    m = c.in_pairs()
    unsettled = int((~to.settled(r64))[m].sum())
    print(f"{name}: {unsettled} of {int(m.sum())} rows unsettled")
    assert unsettled <= 0.02 * m.sum()


@pytest.mark.parametrize("name", tc.NAMES)
def test_float32_agrees_outside_its_margin(name):
    c, r64, r32 = tc.case(name)
    if c.reported:
        return
    m = c.in_pairs()
    inside = np.array([tc.inside_f32_margin(x) for x in r64.cmp], bool) & ~np.full(len(m), c.exact)
    differ = (r64.status != r32.status) | (r64.stereo != r32.stereo)
    print(f"{name}: {int(inside[m].sum())} of {int(m.sum())} rows within M_F32 of a gate, "
          f"{int(differ[m].sum())} statuses differ, largest gate difference {tc.gate_differences(r64, r32)[m].max(initial=0):.2e}")
    assert not (differ & m & ~inside).any(), np.flatnonzero(differ & m & ~inside)
    assert inside[m].sum() <= 0.10 * m.sum()
    # M_F32 is 4 x what was measured: the cases themselves stay inside the measurement
    groups = {}
    tc.gate_differences(r64, r32, groups)
    for g, d in groups.items():
        assert d <= tc.M_F32_MEASURED[g], (g, d)
    ok = m & (r64.status == to.OK) & (r32.status == to.OK) & np.isfinite(r64.X).all(1)
    if ok.any():
        rel = np.abs(r64.X[ok] - r32.X[ok]).max(1) / np.maximum(1.0, np.abs(r64.X[ok]).max(1))
        print(f"{name}: X of the float32 run within {rel.max():.2e} relative")
