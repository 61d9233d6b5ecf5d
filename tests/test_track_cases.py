"""The tracking edge cases (tests/track_cases.py) on the CPU: each case has the property it is named for, and
is well enough conditioned to be compared with the GPU.

tests/test_gpu_track_edges.py holds k_track to the oracle's integer outputs (outlier flags, n_good,
iterations) exactly, and to its pose within TOL_T / TOL_Q / TOL_V.  An input on which an observation's chi2
sits on a threshold, or an LM gain ratio on zero, would fail there for its conditioning and not for a fault
of the kernel.  The stability test therefore runs the oracle again with every z multiplied by
1 + 1e-9 N(0, 1) (three seeds): the integers must come out the same and the pose within a tenth of the GPU
tolerances.  GPU-versus-oracle differences measured in this project are <= 2.5e-12 on H and b
(profiles/window_structure_margins.log), some 400 times smaller than that disturbance, so a case that keeps
a tenth of the tolerance under it cannot miss the tolerance on the GPU for conditioning alone.  Every name
in track_cases.CASES (all that the GPU test compares) goes through it.

That disturbance does not see one kind of ill-conditioning.  An LM round that reaches the rounding floor of
chi2 (a round that starts at the last one's minimum because no flag changed, or a small user lambda that
converges in two steps) before three bad iterations end it goes on taking trials whose gain is rounding
error: the sums of some hundred terms differ between two orders of summation by more than the trial changes
them.  Whether such a trial is accepted, and with it `iterations`, is then not a property of the input;
g2o itself would give another count on another compiler.  The oracle keeps its count under the disturbance
because its own rounding is reproducible, the device (another order of summation) need not: on the default
frame with lambda_init = 1e-2 it ended the last round after ten rejected trials, one iteration before the
oracle, with the poses 2e-11 apart.  So the stability test also runs the oracle with each frame's rows in
six other orders, and asserts that the oracle counted no LM iteration whose gain lay below 1e-11 of chi2
(some 250 N eps for N = 400 edges) at a point where the trial's outcome changes the iteration count
(orc.track_floor_iterations; lba_oracle.c says when it does not).  The inputs in track_cases.PICK were
chosen by these CPU conditions alone.

A rejected LM trial cannot be seen through orc_track_pose's interface directly; it shows as an iteration
count that depends on max_trials (a round stops when qmax reaches it).
"""
import numpy as np
import pytest

import orc
import track_cases as tc
from amc_lba.abi import MONO, MONO_GP, STEREO
from amc_lba.track import track_config

NAMES = list(tc.CASES)
FIX = (True, False)


def _family(name):
    return name.rsplit("-", 1)[0]


def _fix(name):
    return name.endswith("-fix")


def _kinds(obs):
    return set(int(k) for k in np.unique(obs["kind"]))


# ------------------------------------------------------------------ every case has its property
def test_every_family_has_both_previous_frame_modes():
    fams = {_family(n) for n in NAMES}
    for fam in fams - {f"rejected_{v}" for v in "abc"}:
        assert f"{fam}-fix" in tc.CASES and f"{fam}-free" in tc.CASES, fam
    assert sum(n.startswith("rejected_") and _fix(n) for n in NAMES) >= 2
    assert sum(n.startswith("rejected_") and not _fix(n) for n in NAMES) >= 1
    kw = tc.BASE_KW
    assert kw["n_opt_kf"] == 6 and 400 <= kw["n_lm"] <= 1500 and kw["n_cam"] == 4 and kw["perturb"] is False


@pytest.mark.parametrize("name", NAMES)
def test_case_shape(name):
    """What every case must be for lba_track to take it: the ranges inside the array, finite numbers, valid
    kinds and cameras, prev.fixed as the name says."""
    cfg, frames, obs, cams = tc.case(name)
    assert (frames["prev"]["fixed"] == int(_fix(name))).all()
    assert (frames["obs0"] >= 0).all() and (frames["obs0"] + frames["n_obs"] <= len(obs)).all()
    assert np.isin(obs["kind"], (MONO_GP, MONO, STEREO)).all()
    assert (obs["cam"] >= 0).all() and (obs["cam"] < len(cams)).all()
    for f in ("t", "z", "w", "Xw"):
        assert np.isfinite(obs[f]).all()
    for F in frames:
        o = obs[tc.frame_slice(F)]
        assert tc.n_samples(o) <= 16
        gp = o["kind"] == MONO_GP
        assert ((o["t"][gp] >= F["prev"]["time"]) & (o["t"][gp] <= F["cur"]["time"])).all()
    if not name.startswith("controller_"):
        d = track_config()
        assert (cfg.early_stop, cfg.max_trials, cfg.lambda_init) == (d.early_stop, d.max_trials, d.lambda_init)


@pytest.mark.parametrize("fix", FIX)
def test_regular_sample_counts(fix):
    for n_cam in (1, 2, 4):
        _, frames, obs, cams = tc.case(f"regular_c{n_cam}-{tc.tag(fix)}")
        assert len(cams) == n_cam and tc.n_samples(obs) == n_cam and len(frames) == 1
        assert (MONO_GP in _kinds(obs)) == (n_cam > 1)
        assert {MONO, STEREO} <= _kinds(obs)


@pytest.mark.parametrize("fix", FIX)
def test_kind_filters(fix):
    t = tc.tag(fix)
    _, frames, obs, _ = tc.case(f"gp_only-{t}")
    assert _kinds(obs) == {MONO_GP} and tc.n_samples(obs) == 3 == len(np.unique(obs["t"]))   # no own-pose sample
    _, frames_r, obs_r, _ = tc.case(f"ref_only-{t}")
    assert _kinds(obs_r) == {MONO, STEREO} and tc.n_samples(obs_r) == 1
    _, frames_s, obs_s, _ = tc.case(f"stereo_only-{t}")
    assert _kinds(obs_s) == {STEREO} and tc.n_samples(obs_s) == 1
    _, frames_m, obs_m, _ = tc.case(f"mono_only-{t}")
    assert _kinds(obs_m) == {MONO} and tc.n_samples(obs_m) == 1
    for fr, ob in ((frames, obs), (frames_r, obs_r), (frames_s, obs_s), (frames_m, obs_m)):
        assert fr[0]["n_obs"] == len(ob) >= 7 and fr[0]["obs0"] == 0     # (more than one round)


@pytest.mark.parametrize("fix", FIX)
def test_sample_table_limits(fix):
    _, frames, obs, cams = tc.case(f"samples16-{tc.tag(fix)}")
    assert tc.n_samples(obs) == 16 and len(cams) == 16
    _, frames, obs, cams = tc.case_samples(fix, 17)
    assert tc.n_samples(obs) == 17 and len(cams) == 17


@pytest.mark.parametrize("fix", FIX)
def test_endpoint_stamps(fix):
    name = f"endpoint_stamps-{tc.tag(fix)}"
    _, frames, obs, _ = tc.case(name)
    gp = obs["kind"] == MONO_GP
    at_cur = gp & (obs["t"] == frames[0]["cur"]["time"])
    at_prev = gp & (obs["t"] == frames[0]["prev"]["time"])
    assert at_cur.sum() == 6 and at_prev.sum() == 4
    assert (~gp).any()                         # the own-pose sample shares cur.time with a GP sample
    assert tc.n_samples(obs) == 3 + 2 + 1
    _, ob_o = tc.reference(name)
    assert not ob_o["outlier"][at_cur | at_prev].any()   # re-measured at the keyframes' poses: inliers


@pytest.mark.parametrize("fix", FIX)
def test_sizes(fix):
    for n in tc.SIZES:
        name = f"sizes_{n}-{tc.tag(fix)}"
        _, frames, obs, _ = tc.case(name)
        assert len(obs) == n == frames[0]["n_obs"]
        fr_o, _ = tc.reference(name)
        if n + 3 < 10:
            assert fr_o[0]["iterations"] <= 10          # one round
        else:
            assert fr_o[0]["iterations"] > 10
        if n == 0:
            assert fr_o[0]["n_good"] == 0 and fr_o[0]["iterations"] == 10
    _, _, obs, _ = tc.case(f"sizes_257-{tc.tag(fix)}")
    assert len(_kinds(obs[:6])) >= 2                    # the kinds interleave from the first rows on


@pytest.mark.parametrize("fix", FIX)
def test_behind(fix):
    name = f"behind-{tc.tag(fix)}"
    _, frames, obs, cams = tc.case(name)
    rows = tc.behind_rows(obs)
    k, _, over = tc.pick("behind", fix)
    win = tc.window(**over)
    depth = tc.obs_depth(win.kfs[k], cams, obs)
    assert 8 <= len(rows) <= 12 and _kinds(obs[rows]) == {MONO_GP, MONO, STEREO}
    assert (depth[rows] < -1.0).all()
    rest = np.ones(len(obs), bool)
    rest[rows] = False
    assert (depth[rest] > 0.3).all()
    # consistent measurements: at the true pose their chi2 is that of the pixel noise, below every threshold
    e = obs["z"][rows] - tc.true_projection(win, k, obs[rows])
    e[obs["kind"][rows] != STEREO, 2] = 0.0
    assert ((e * e).sum(axis=1) * obs["w"][rows] < 5.991).all()
    # so isDepthPositive decides: out for mono and GP, and stereo (no depth test) stays in
    _, ob_o = tc.reference(name)
    st = obs["kind"][rows] == STEREO
    assert ob_o["outlier"][rows][~st].all() and not ob_o["outlier"][rows][st].any()


@pytest.mark.parametrize("fix", FIX)
def test_all_outlier_comes_back(fix):
    name = f"all_outlier-{tc.tag(fix)}"
    _, frames, obs, _ = tc.case(name)
    assert (obs["outlier"] == 1).all()
    fr_o, _ = tc.reference(name)
    assert fr_o[0]["n_good"] > 0.8 * len(obs)


@pytest.mark.parametrize("fix", FIX)
def test_controller_stop_rules(fix):
    t = tc.tag(fix)
    assert tc.reference(f"controller_nostop-{t}")[0][0]["iterations"] == 40
    assert tc.reference(f"controller_trials1-{t}")[0][0]["iterations"] == 4
    cfg = tc.case(f"controller_lambda-{t}")[0]
    assert cfg.lambda_init == 1e-2
    assert tc.case(f"controller_trials2-{t}")[0].max_trials == 2
    # the user lambda is in effect: another trajectory than computeLambdaInit's on the same frame
    _, frames, obs, cams = tc.case(f"controller_lambda-{t}")
    fr_d, _ = tc.run_oracle(track_config(), frames, obs, cams)
    assert tc.reference(f"controller_lambda-{t}")[0][0]["cur"].tobytes() != fr_d[0]["cur"].tobytes()


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("rejected_")])
def test_rejected_cases_reject_and_converge(name):
    fix, variant = _fix(name), _family(name)[len("rejected_"):]
    it = {}
    for mt in (2, 10):
        fr, _ = tc.run_oracle(*tc.case_rejected(fix, variant, max_trials=mt))
        it[mt] = int(fr[0]["iterations"])
    print(f"{name}: iterations {it[2]} at max_trials=2, {it[10]} at max_trials=10")
    assert it[2] != it[10]
    fr_o, _ = tc.reference(name)
    assert fr_o[0]["iterations"] == it[10]
    assert fr_o[0]["n_good"] > 0.8 * fr_o[0]["n_obs"]


@pytest.mark.parametrize("fix", FIX)
def test_regular_start_never_rejects(fix):
    """(why `rejected` exists: the generator's own start does not reach the reject branch)"""
    _, frames, obs, cams = tc.case(f"regular_c4-{tc.tag(fix)}")
    it = [int(tc.run_oracle(track_config(max_trials=mt), frames, obs, cams)[0][0]["iterations"]) for mt in (2, 10)]
    assert it[0] == it[1]


@pytest.mark.parametrize("fix", FIX)
def test_cur_fixed_flag_is_ignored(fix):
    name = f"cur_fixed_flag-{tc.tag(fix)}"
    cfg, frames, obs, cams = tc.case(name)
    assert frames[0]["cur"]["fixed"] == 1
    fr_o, ob_o = tc.reference(name)
    free = frames.copy()
    free["cur"]["fixed"] = 0
    fr_f, ob_f = tc.run_oracle(cfg, free, obs, cams)
    assert fr_o[0]["cur"]["fixed"] == 1
    for f in ("q", "t", "vel"):
        np.testing.assert_array_equal(fr_o[0]["cur"][f], fr_f[0]["cur"][f])
    np.testing.assert_array_equal(ob_o["outlier"], ob_f["outlier"])
    assert fr_o[0]["iterations"] == fr_f[0]["iterations"] and fr_o[0]["n_good"] == fr_f[0]["n_good"] > 0


@pytest.mark.parametrize("fix", FIX)
def test_shuffled_obs_oracle_is_equivariant(fix):
    name = f"shuffled_obs-{tc.tag(fix)}"
    cfg, frames, obs, cams = tc.case(name)
    _, _, obs_u, _ = tc.case_shuffled_obs(fix, shuffle=False)
    perm = tc.shuffle_perm(len(obs))
    assert obs.tobytes() == obs_u[perm].tobytes()
    runs = lambda o, kd: int((np.diff(o["kind"] == kd) != 0).sum())   # noqa: E731
    assert runs(obs, MONO_GP) > 50                      # kinds (and with them the samples) interleave
    fr_s, ob_s = tc.reference(name)
    fr_u, ob_u = tc.run_oracle(cfg, frames, obs_u, cams)
    np.testing.assert_array_equal(ob_s["outlier"], ob_u["outlier"][perm])
    assert fr_s[0]["n_good"] == fr_u[0]["n_good"] and fr_s[0]["iterations"] == fr_u[0]["iterations"]
    d = tc.pose_diff(fr_s[0]["cur"], fr_u[0]["cur"])
    assert d[0] <= 0.1 * tc.TOL_T and d[1] <= 0.1 * tc.TOL_Q and d[2] <= 0.1 * tc.TOL_V, d


@pytest.mark.parametrize("fix", FIX)
def test_ranges_layout(fix):
    _, frames, obs, _ = tc.case(f"ranges-{tc.tag(fix)}")
    assert len(frames) == 3 and (np.diff(frames["obs0"]) < 0).all()          # reverse frame order
    used = tc.used_rows(frames, len(obs))
    assert used.sum() == frames["n_obs"].sum() and (~used).sum() == 3 + 5 + 2 + 4
    assert (obs["outlier"][~used] == tc.SENTINEL).all() and (obs["outlier"][used] <= 1).all()
    assert not used[0] and not used[-1]
    ends = frames["obs0"] + frames["n_obs"]
    assert frames["obs0"][1] > ends[2] and frames["obs0"][0] > ends[1]         # unused rows between the ranges
    fr_o, ob_o = tc.reference(f"ranges-{tc.tag(fix)}")
    assert (ob_o["outlier"][~used] == tc.SENTINEL).all()


# ------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("name", NAMES)
def test_case_is_stable_under_disturbance(name):
    cfg, frames, obs, cams = tc.case(name)
    same, (dt, dq, dv), floor = tc.stability(cfg, frames, obs, cams)
    print(f"{name}: oracle vs disturbed / reordered oracle  t {dt:.2e}  q {dq:.2e}  vel {dv:.2e}  integers equal {same}  "
          f"LM decisions at the rounding floor {floor}")
    assert same and floor == 0
    assert dt <= 0.1 * tc.TOL_T and dq <= 0.1 * tc.TOL_Q and dv <= 0.1 * tc.TOL_V


@pytest.mark.parametrize("fix", FIX)
def test_floor_counter_sees_a_round_decided_by_rounding(fix):
    """The default frame under lambda_init = 1e-2 converges in two steps per round and then takes trials whose
    gain is rounding error with fewer than two bad iterations counted: the input the counter is there to keep
    out (the device and the oracle differed by one iteration on it, the poses by 2e-11)."""
    _, frames, obs, cams = tc.case(f"regular_c4-{tc.tag(fix)}")
    orc.track_floor_iterations(reset=True)
    tc.run_oracle(track_config(lambda_init=1e-2), frames, obs, cams)
    assert orc.track_floor_iterations(reset=True) >= 1
    tc.run_oracle(track_config(), frames, obs, cams)
    assert orc.track_floor_iterations(reset=True) == 0


def test_oracle_leaves_inputs_alone():
    """orc.track_pose writes cur's pose and velocity, n_good, iterations and the outlier flags, nothing else."""
    cfg, frames, obs, cams = tc.case("ranges-free")
    fr_o, ob_o = tc.reference("ranges-free")
    assert fr_o["prev"].tobytes() == frames["prev"].tobytes()
    for f in ("time", "bf", "fixed"):
        assert fr_o["cur"][f].tobytes() == frames["cur"][f].tobytes()
    for f in obs.dtype.names:
        if f != "outlier":
            assert ob_o[f].tobytes() == obs[f].tobytes()
