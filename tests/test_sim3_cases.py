"""The OptimizeSim3 cases of tests/sim3_cases.py on the CPU: each has the property it is named for, each is settled
(the integer outputs are the same for the reference-faithful numeric-Jacobian run, the analytic run and the analytic
run with H and b disturbed by 1e-6 relative, three seeds), and the analytic run's S12 is within the GPU test's
tolerance of the numeric run's, so a GPU result within that tolerance of the analytic run is within twice it of the
reference-faithful one.  `pytest -s` prints the measured gaps (profiles/sim3_margins.log is that output).

Settledness is a condition on the chosen seeds, not on the product: with 0.7 px noise against a gate of
sqrt(10) = 3.2 px at octave 0 an inlier within 1e-6 relative of the gate has odds below 1e-4 per case.
"""
import numpy as np
import pytest

import sim3_cases as sc
import sim3_oracle as so


@pytest.mark.parametrize("name", sc.CASES)
def test_case_is_settled(name):
    assert sc.settled(name)


@pytest.mark.parametrize("name", sc.CASES)
def test_analytic_run_is_within_tolerance_of_the_numeric_run(name):
    a, n = sc.reference(name, "analytic"), sc.reference(name, "numeric")
    gq, gt, gs = so.state_gap(a, n)
    print(f"{name}: analytic vs numeric Jacobian  q {gq:.2e}  t {gt:.2e}  s {gs:.2e}  "
          f"(n_bad {a['n_bad']}, n_in {a['n_in']}, iterations {a['iterations']} / {n['iterations']})")
    assert max(gq, gt, gs) <= sc.TOL


@pytest.mark.parametrize("n", sc.N_CORR_EDGES)
def test_correspondence_counts(n):
    r = sc.reference(f"ncorr_{n}")
    pairs, corr, _, _ = sc.case(f"ncorr_{n}")
    assert len(corr) == n == pairs["n_corr"][0]
    assert r["ret0"] == (n - r["n_bad"] < 10)
    if n == 0:
        assert r["iterations"] == 0 and r["n_in"] == 0
    if n in (1, 9):
        assert r["ret0"] and r["n_in"] == 0 and 1 <= r["iterations"] <= 5     # the first round ran, the second did not
    if n >= 10:
        assert not r["ret0"] and r["n_in"] > 0


def test_clean_takes_five_more_iterations():
    r = sc.reference("clean_40")
    assert r["n_bad"] == 0 and not r["ret0"] and r["n_in"] == 40
    assert r["iterations"] <= 5 + 5


def test_gross_outliers_are_dropped_by_the_first_pass():
    r = sc.reference("outliers_10pct")
    gross = sc.truth("outliers_10pct")["gross"]
    assert r["n_bad"] == gross.sum() == 6 and (r["first_bad"] == gross).all()
    assert not r["ret0"] and r["n_in"] == 54


def test_return0_leaves_the_state_and_writes_the_flags():
    r = sc.reference("return0_12_3")
    pairs, _, _, _ = sc.case("return0_12_3")
    gross = sc.truth("return0_12_3")["gross"]
    assert r["ret0"] and r["n_in"] == 0 and r["n_bad"] == 3
    assert (r["outlier"].astype(bool) == gross).all()
    assert (r["q"] == pairs["q"][0]).all() and (r["t"] == pairs["t"][0]).all() and r["s"] == pairs["s"][0]


def test_survivors_12_of_14():
    r = sc.reference("survivors_12_of_14")
    assert r["n_bad"] == 2 and not r["ret0"] and r["n_in"] == 12


def test_scale_free_and_fixed():
    free, fixed = sc.reference("scale_free"), sc.reference("scale_fixed")
    pf, cf, _, _ = sc.case("scale_free")
    px, cx, _, _ = sc.case("scale_fixed")
    assert cf.tobytes() == cx.tobytes() and pf["s"][0] == px["s"][0] and pf["fix_scale"][0] == 0 and px["fix_scale"][0] == 1
    assert fixed["s"] == px["s"][0]                                   # bitwise: sigma is zeroed in every update
    assert abs(free["s"] - 1.15) < 0.02 and free["s"] != pf["s"][0]


def test_far_start_has_rejected_trials():
    r = sc.reference("far_start")
    assert r["rejected"] >= 1 and not r["ret0"]
    t = sc.truth("far_start")
    assert np.abs(r["t"] - t["t"][0]).max() < 0.05                    # and still gets home


def test_converged_start_steps_fall_below_eps():
    r = sc.reference("converged_start")
    assert 0 in r["branches"]                                         # |sigma| < 1e-5 and theta < 1e-5
    assert so.EPS == 1e-5


def test_camera_pairs():
    _, one, _, n_cam = sc.case("one_campair")
    assert len(set(zip(one["cam1"].tolist(), one["cam2"].tolist()))) == 1 and len(one) == 40
    _, spread, _, n_cam = sc.case("all_campairs")
    assert len(set(zip(spread["cam1"].tolist(), spread["cam2"].tolist()))) == n_cam * n_cam == 9


def test_every_octave():
    _, corr, _, _ = sc.case("every_octave")
    levels = np.float32(1.0 / 1.2 ** (2 * np.arange(8)))
    assert set(corr["w1"].tolist()) == set(corr["w2"].tolist()) == set(np.float64(levels).tolist())


def test_late_outlier():
    r = sc.reference("late_outlier")
    late = r["outlier"].astype(bool) & ~r["first_bad"]
    assert late.sum() >= 1 and not r["ret0"]
    assert r["n_in"] == len(late) - r["n_bad"] - late.sum()


def test_flags_follow_the_rows():
    a, b = sc.reference("rows_in_order"), sc.reference("rows_shuffled")
    perm = sc.shuffle_perm(len(a["outlier"]))
    assert (b["outlier"] == a["outlier"][perm]).all() and a["outlier"].any()
    assert a["n_bad"] == b["n_bad"] and a["n_in"] == b["n_in"]
    assert max(so.state_gap(a, b)) <= sc.TOL                          # (another order of the sums: rounding only)


def test_sim3_structs_match_header(tmp_path):
    """The numpy mirrors of lba_sim3_cam / lba_sim3_corr / lba_sim3_pair have the C layout of include/amc_lba.h."""
    import os
    import subprocess
    from amc_lba.sim3 import SIM3_CAM_DTYPE, SIM3_CORR_DTYPE, SIM3_PAIR_DTYPE
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "amc_lba.h")
    fields = [(s, d, f) for s, d in (("lba_sim3_cam", SIM3_CAM_DTYPE), ("lba_sim3_corr", SIM3_CORR_DTYPE),
                                     ("lba_sim3_pair", SIM3_PAIR_DTYPE)) for f in d.names]
    body = "".join(f'printf("%zu %zu\\n", sizeof({s}), offsetof({s}, {f}));' for s, _, f in fields)
    code = f'#include "{header}"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){{{body}return 0;}}'
    exe = str(tmp_path / "sim3_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-o", exe], input=code, text=True, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    for (s, d, f), line in zip(fields, out):
        size, off = (int(x) for x in line.split())
        assert size == d.itemsize and off == d.fields[f][1], (s, f)


def test_sim3_rows_restates_the_callers_filters():
    from amc_lba.sim3 import sim3_rows
    N = 12
    rng = np.random.default_rng(5)
    match, has1 = np.ones(N, bool), np.ones(N, bool)
    bad1, bad2 = np.zeros(N, bool), np.zeros(N, bool)
    i2, P1, P2 = np.arange(N), rng.uniform(1, 9, (N, 3)), rng.uniform(1, 9, (N, 3))
    match[1] = False          # null match
    i2[2] = -1                # no index in KF2
    bad1[3] = True            # nBadMPs
    bad2[4] = True            # nBadMPs
    has1[5] = False           # nMatchWithoutMP
    P2[6, 2] = -0.5           # behind camera 2
    rows, index, n, counters = sim3_rows(match, has1, bad1, bad2, i2, np.arange(N) % 4, np.arange(N) % 3, P1, P2,
                                         rng.uniform(0, 900, (N, 2)), rng.uniform(0, 900, (N, 2)), np.ones(N), np.ones(N))
    assert index.tolist() == [0, 7, 8, 9, 10, 11] and n == 6 == len(rows)
    assert counters == {"nBadMPs": 2, "nMatchWithoutMP": 1}
    assert (rows["cam1"] == index % 4).all() and (rows["X2c"] == np.float32(P2[index])).all()
