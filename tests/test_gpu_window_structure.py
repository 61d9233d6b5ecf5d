"""Parity on windows of irregular structure (tests/window_mutations.py) and the device path of EdgeStereoGP.

Every other GPU parity test draws its window from amc_lba.synth.make_window, which emits one shape of
graph.  lba_set_problem (csrc/lba_host.hip) and what k_lin_schur, k_exp_asm and k_update consume depend on
structure: the activity marks, the numbering of GP pairs per keyframe b, the sample keys with their 16 inline
slots and overflow list, the order key of landmarks seen by fixed keyframes only, the compression of b and dx
to the active vertices.  The cases here bend that structure one property at a time: fixed keyframes anywhere
(GP observations and motion priors with a fixed newer keyframe), landmarks without a free pose vertex, with one
observation, with none, a keyframe without an edge, arbitrary array order, LBA_STEREO_GP (EdgeStereoGP,
include/G2oTypes.h:404-421), GP pairs that skip a keyframe, cameras sharing a time stamp, observation times
at the ends of the GP interval, more sample times per pair than the inline table holds, and pose systems
of one block up to the 64 / 65-panel boundary where the substitution solve becomes the default.

CPU: each window has the property it is named for (counted in numpy), lba_setup_host_profile accepts it and
reports the expected pose dimension and device-landmark count, and the oracle agrees with itself on a
shuffle of the window within 1e-8 (so 1e-6 against the GPU is a bound on the engine, not on the
conditioning of the case).  GPU (tolerances of tests/test_gpu_parity.py): linearisation, damped steps, whole LM runs
against the oracle; inactive vertices untouched; shuffle equivariance on the device.  The GPU tests print
the margins they measure (pytest -s).
"""
import functools

import numpy as np
import pytest

import amc_lba
import orc
import window_mutations as wm
from amc_lba.abi import FLAG_BAND_SOLVE, FLAG_HOST_LOOP, MONO, STEREO_GP
from amc_lba.synth import make_window

CASE_NAMES = list(wm.CASES)
LAMBDAS = (1.0, 1e-3)
KC_INLINE, SETUP_PIECES = 16, 16   # lba_set_problem's sample-key pass: inline keys per (piece, GP pair), pieces


@functools.lru_cache(maxsize=None)
def _win(name):
    """The case's window, built once; no test changes it."""
    return wm.CASES[name]()


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ------------------------------------------------------------------ references (the oracle, once per case)
@functools.lru_cache(maxsize=None)
def _ref_linearize(name):
    o = orc.Oracle(_win(name))
    chi, res, c2 = o.errors()
    H, b, Hll = o.build_system()
    steps = {lam: o.solve(lam) for lam in LAMBDAS}
    return dict(chi=chi, res=res, c2=c2, H=H, b=b, Hll=Hll, ok=o.depth_ok(), steps=steps, np=o.pose_dim)


@functools.lru_cache(maxsize=None)
def _ref_optimize(name):
    o = orc.Oracle(_win(name))
    n, st = o.optimize(10)
    kf, lm = o.state()
    return dict(n=n, st=st, kf=kf, lm=lm, c2=o.last_obs_chi2(), ok=o.depth_ok())


def _state_diff(kf, lm, kf_o, lm_o):
    """Largest differences of two states: absolute on t and landmarks (metres)."""
    return np.abs(kf["t"] - kf_o["t"]).max(), np.abs(lm - lm_o).max()


# ------------------------------------------------------------------ CPU: the windows have their properties
def _gp_fixed_counts(win):
    o = win.obs
    fixed = win.kfs["fixed"] != 0
    gp = wm.is_gp(o)
    fa, fb = gp & fixed[np.maximum(o["kf_a"], 0)], fixed[o["kf_b"]]
    return int((gp & ~fa & fb).sum()), int((gp & fa & ~fb).sum()), int((gp & fa & fb).sum())


def _free_blocks_per_landmark(win):
    """Per landmark: the number of (observation, free keyframe) incidences."""
    o = win.obs
    fixed = win.kfs["fixed"] != 0
    n = np.bincount(o["lm"], weights=~fixed[o["kf_b"]], minlength=len(win.lm))
    gp = wm.is_gp(o)
    return n + np.bincount(o["lm"][gp], weights=~fixed[o["kf_a"][gp]], minlength=len(win.lm))


def _max_times_per_pair_and_piece(win):
    """Largest number of distinct observation times of one (kf_a, kf_b) pair inside one of the SETUP_PIECES
    contiguous pieces of the observation array (the set-up's pieces: [n i / 16, n (i + 1) / 16))."""
    o, n, best = win.obs, len(win.obs), 0
    for piece in range(SETUP_PIECES):
        s = o[n * piece // SETUP_PIECES: n * (piece + 1) // SETUP_PIECES]
        s = s[wm.is_gp(s)]
        keys = np.unique(np.stack([s["kf_a"].astype(np.float64), s["kf_b"].astype(np.float64), s["t"]], axis=1), axis=0)
        if len(keys):
            _, cnt = np.unique(keys[:, :2], axis=0, return_counts=True)
            best = max(best, int(cnt.max()))
    return best


def _pairs_per_kf_b(win):
    o = win.obs[wm.is_gp(win.obs)]
    pairs = np.unique(np.stack([o["kf_a"], o["kf_b"]], axis=1), axis=0)
    return np.bincount(pairs[:, 1], minlength=len(win.kfs))


def test_base_window_is_the_regular_one():
    w = _win("base")
    o = w.obs
    gp = wm.is_gp(o)
    assert (len(w.kfs), len(o), 12 * int((w.kfs["fixed"] == 0).sum())) == (11, 1703, 120)
    assert np.all(o["kf_a"][gp] == o["kf_b"][gp] - 1) and np.all(np.diff(o["lm"]) >= 0)
    assert np.bincount(o["lm"], minlength=len(w.lm)).min() >= 2 and not np.any(o["kind"] == STEREO_GP)
    assert list(np.nonzero(w.kfs["fixed"])[0]) == [0]


def test_fixed_scattered_properties():
    w = _win("fixed_scattered")
    assert list(np.nonzero(w.kfs["fixed"])[0]) == [0, 4, 5, 10]
    a_free_b_fixed, a_fixed_b_free, both = _gp_fixed_counts(w)
    assert a_free_b_fixed > 0 and a_fixed_b_free > 0 and both == 164
    fixed = w.kfs["fixed"] != 0
    pri = list(zip(w.priors["kf_a"].tolist(), w.priors["kf_b"].tolist()))
    assert (4, 5) in pri                                                   # all-fixed (inactive)
    assert any(not fixed[a] and fixed[b] for a, b in pri)                  # the newer keyframe fixed
    assert any(fixed[a] and not fixed[b] for a, b in pri)
    assert fixed[w.vel_kfs].sum() == 3                                     # velocity edges on fixed keyframes
    # the composition: heavy landmarks (more keyframes than a tile holds) across fixed keyframes
    from test_heavy_landmarks import _heavy_count
    ws = _win("spanning_fixed")
    assert _heavy_count(ws) >= 3 and list(np.nonzero(ws.kfs["fixed"])[0]) == [0, 4, 5, 10]
    assert all(v > 0 for v in _gp_fixed_counts(ws))


def test_one_free_properties():
    w = _win("one_free")
    assert list(np.nonzero(w.kfs["fixed"] == 0)[0]) == [5]


def test_fixed_only_landmarks_properties():
    w = _win("fixed_only_landmarks")
    o = w.obs
    fixed = w.kfs["fixed"] != 0
    for l in range(12):
        s = o[o["lm"] == l]
        assert len(s) == 2 and np.all(s["kind"] == MONO) and np.all(fixed[s["kf_b"]]) and s["kf_b"][0] != s["kf_b"][1]
        assert np.all(s["cam"] == len(w.cams) - 1)
    free = _free_blocks_per_landmark(w)
    assert np.all(free[:12] == 0) and int((free == 0).sum()) >= 12
    # consistent measurements: the residuals of the re-made observations are pixel noise
    _, res, _ = orc.Oracle(w).errors()
    assert np.abs(res[np.isin(o["lm"], np.arange(12))]).max() < 6.0


def test_single_obs_properties():
    w = _win("single_obs")
    cnt = np.bincount(w.obs["lm"], minlength=len(w.lm))
    assert np.all(cnt[20:32] == 1) and np.all(np.delete(cnt, np.arange(20, 32)) >= 2)
    b = _win("base").obs
    for l in range(20, 32):   # the first observation is the one kept
        assert w.obs[w.obs["lm"] == l][0] == b[b["lm"] == l][0]


def test_unobserved_properties():
    w = _win("unobserved")
    o = w.obs
    cnt = np.bincount(o["lm"], minlength=len(w.lm))
    assert list(np.nonzero(cnt == 0)[0]) == [0, 7, 150, 299]
    assert not np.any(o["kf_b"] == 5) and not np.any(wm.is_gp(o) & (o["kf_a"] == 5))
    assert 5 not in w.priors["kf_a"] and 5 not in w.priors["kf_b"] and 5 not in w.vel_kfs
    assert w.kfs["fixed"][5] == 0
    kf_act, lm_act = wm.active_vertices(w)
    assert 5 not in kf_act and len(kf_act) == 9 and len(lm_act) == 296


@pytest.mark.parametrize("name", ["base", "stereo_gp"])
def test_shuffled_properties(name):
    w = _win(name)
    ws, pr = wm.shuffled(w)
    o, os_ = w.obs, ws.obs
    assert np.any(np.diff(os_["lm"]) < 0) and np.any(np.diff(ws.kfs["time"]) < 0)
    assert ws.kfs["fixed"][0] == 0 and ws.kfs["fixed"].sum() == 1          # the fixed keyframe is not the first
    # the same problem: every edge of the shuffle is the original's, read through the permutations
    back = os_.copy()
    back["kf_b"] = pr["kf"][os_["kf_b"]]
    gp = wm.is_gp(os_)
    back["kf_a"][gp] = pr["kf"][os_["kf_a"][gp]]
    back["lm"] = pr["lm"][os_["lm"]]
    assert np.array_equal(back, o[pr["obs"]])
    assert np.array_equal(ws.kfs, w.kfs[pr["kf"]]) and np.array_equal(ws.lm, w.lm[pr["lm"]])
    assert sorted(zip(pr["kf"][ws.priors["kf_a"]], pr["kf"][ws.priors["kf_b"]])) == \
        sorted(zip(w.priors["kf_a"], w.priors["kf_b"]))
    assert sorted(pr["kf"][ws.vel_kfs]) == sorted(w.vel_kfs)
    gps = wm.is_gp(os_)
    assert np.any(os_["kf_a"][gps] != os_["kf_b"][gps] - 1)


def test_stereo_gp_properties():
    w = _win("stereo_gp")
    n_sgp, n_gp = int((w.obs["kind"] == STEREO_GP).sum()), int(wm.is_gp(w.obs).sum())
    assert n_gp == 1195 and 0.45 * n_gp <= n_sgp <= 0.55 * n_gp
    sel = w.obs["kind"] == STEREO_GP
    assert np.array_equal(w.obs["z"][sel, 2], w.obs["z"][sel, 2].astype(np.float32).astype(np.float64))
    _, res, _ = orc.Oracle(w).errors()
    assert np.abs(res[sel, 2]).max() < 6.0 and np.abs(res[sel, 2]).std() > 0.3   # u_r: projection + N(0, 1)
    assert int((_win("stereo_gp_shuffled").obs["kind"] == STEREO_GP).sum()) == n_sgp


def test_skip_pairs_properties():
    w = _win("skip_pairs")
    o = w.obs[wm.is_gp(w.obs)]
    assert np.any(o["kf_a"] == o["kf_b"] - 2) and np.any(o["kf_a"] == o["kf_b"] - 1)
    per_b = _pairs_per_kf_b(w)
    assert np.all(per_b[3:] == 2) and per_b.max() == 2
    assert np.all(w.kfs["time"][o["kf_a"]] <= o["t"]) and np.all(o["t"] <= w.kfs["time"][o["kf_b"]])


def test_shared_stamp_properties():
    w, b = _win("shared_stamp"), _win("base")
    o = w.obs[wm.is_gp(w.obs)]
    shared = 0
    for k in np.unique(o["kf_b"]):
        t0, t1 = (np.unique(o["t"][(o["kf_b"] == k) & (o["cam"] == c)]) for c in (0, 1))
        if len(t0) and len(t1):
            assert np.array_equal(t0, t1)
            shared += 1
    assert shared >= 8
    ob = b.obs[wm.is_gp(b.obs)]
    for k in np.unique(ob["kf_b"]):   # the generator never shares one
        assert len(np.unique(ob["t"][ob["kf_b"] == k])) == len(np.unique(ob["cam"][ob["kf_b"] == k]))


def test_endpoint_times_properties():
    w = _win("endpoint_times")
    o = w.obs[wm.is_gp(w.obs)]
    c0, c1 = o[o["cam"] == 0], o[o["cam"] == 1]
    assert len(c0) > 100 and len(c1) > 100
    assert np.array_equal(c0["t"], w.kfs["time"][c0["kf_b"]]) and np.array_equal(c1["t"], w.kfs["time"][c1["kf_a"]])


def test_many_cams_overflows_the_inline_sample_keys():
    assert _max_times_per_pair_and_piece(_win("many_cams")) > KC_INLINE
    assert _max_times_per_pair_and_piece(_win("base")) <= KC_INLINE


# ------------------------------------------------------------------ CPU: host set-up and the oracle against itself
TABLE = {   # pose dimension, device landmarks
    "base": (120, 300), "fixed_scattered": (84, 300), "one_free": (12, 300), "fixed_only_landmarks": (84, 300),
    "single_obs": (120, 300), "unobserved": (108, 296), "shuffled": (120, 300), "stereo_gp": (120, 300),
    "skip_pairs": (120, 300), "shared_stamp": (120, 300), "endpoint_times": (120, 300), "many_cams": (120, 600),
    "spanning_fixed": (324, 300), "stereo_gp_shuffled": (120, 300),
}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_setup_accepts_the_window(name):
    """lba_setup_host_profile (lba_set_problem's host preprocessing, no GPU): no LBA_E_LIMIT / LBA_E_ARG, and the
    pose dimension and device-landmark count of the active vertices."""
    w = _win(name)
    _, cnt = amc_lba.setup_host_profile(w)     # raises LbaError on any error code
    kf_act, lm_act = wm.active_vertices(w)
    assert (int(cnt[2]), int(cnt[0])) == (12 * len(kf_act), len(lm_act)) == TABLE[name]
    assert int(cnt[1]) == len(kf_act) and int(cnt[3]) >= 1
    o = orc.Oracle(w)
    assert (o.pose_dim, o.lm_dim) == (12 * len(kf_act), 3 * len(lm_act))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_agrees_with_itself_under_shuffle(name):
    """optimize(10) on the window and on a shuffle of it: equal trial counts, keyframe translations and
    landmarks within 1e-8 (absolute, metres).  Only the order of the sums and of the elimination differs, so
    a case that passes is conditioned well enough for the 1e-6 asked of the GPU."""
    w = _win(name)
    ws, pr = wm.shuffled(w, seed=59)
    ref = _ref_optimize(name)
    o = orc.Oracle(ws)
    n, st = o.optimize(10)
    kf, lm = wm.unshuffle_state(*o.state(), pr)
    dt, dl = _state_diff(kf, lm, ref["kf"], ref["lm"])
    print(f"{name}: oracle vs its shuffle: iterations {n}, trials {st.trials}, |dt| {dt:.2e}, |dlm| {dl:.2e}")
    assert (n, st.trials, st.result) == (ref["n"], ref["st"].trials, ref["st"].result)
    assert dt <= 1e-8 and dl <= 1e-8


# ------------------------------------------------------------------ GPU against the oracle
def _check_linearize(p, ref, tag):
    res, H, b, Hll = p.linearize()
    dres = np.linalg.norm(res - ref["res"]) / np.linalg.norm(ref["res"])
    assert H.shape == ref["H"].shape and b.shape == ref["b"].shape and Hll.shape == ref["Hll"].shape
    assert p.pose_dim == ref["np"]
    rH, rb, rL = _rel(H, ref["H"]), _rel(b, ref["b"]), _rel(Hll, ref["Hll"])
    chi, c2, ok = p.eval()
    rchi = abs(chi - ref["chi"]) / ref["chi"]
    print(f"{tag}: linearize res {dres:.2e} H {rH:.2e} b {rb:.2e} Hll {rL:.2e} chi2 {rchi:.2e}")
    assert dres <= 1e-8
    assert rH < 1e-9 and rb < 1e-9 and rL < 1e-9
    assert rchi <= 1e-9
    np.testing.assert_allclose(c2, ref["c2"], rtol=1e-8, atol=1e-10)
    np.testing.assert_array_equal(ok, ref["ok"])
    return H, b, Hll


def _check_step(p, ref_step, tag):
    ok_o, dx_o = ref_step
    lam = tag[1]
    ok, dx = p.solve_step(lam)
    assert ok == ok_o
    assert dx.shape == dx_o.shape
    n = p.pose_dim
    rp, rl = _rel(dx[:n], dx_o[:n]), _rel(dx[n:], dx_o[n:])
    print(f"{tag[0]}: step lambda {lam:g} dx pose {rp:.2e} landmarks {rl:.2e}")
    assert rp <= 1e-6 and rl <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_structure_linearize_matches_oracle(name):
    p = amc_lba.Problem(_win(name))
    _check_linearize(p, _ref_linearize(name), name)
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, FLAG_BAND_SOLVE], ids=["default", "band"])
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_structure_step_matches_oracle(name, lam, flags):
    ref = _ref_linearize(name)
    p = amc_lba.Problem(_win(name), flags=flags)
    assert p.solver_info()["band"] == (1 if flags else 0)
    p.linearize()
    _check_step(p, ref["steps"][lam], (f"{name}[{'band' if flags else 'default'}]", lam))
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, FLAG_HOST_LOOP], ids=["queued", "host_loop"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_structure_optimize_matches_oracle(name, flags):
    ref = _ref_optimize(name)
    st_o, kf_o, lm_o = ref["st"], ref["kf"], ref["lm"]
    p = amc_lba.Problem(_win(name), flags=flags)
    n, st = p.optimize(10)
    kf, lm = p.state()
    q, qo = kf["q"] * np.sign(kf["q"][:, 3:4]), kf_o["q"] * np.sign(kf_o["q"][:, 3:4])
    figs = dict(chi2_initial=abs(st.chi2_initial - st_o.chi2_initial) / st_o.chi2_initial,
                chi2_final=abs(st.chi2_final - st_o.chi2_final) / st_o.chi2_final,
                t=_rel(kf["t"], kf_o["t"]), lm=_rel(lm, lm_o), vel=_rel(kf["vel"], kf_o["vel"]), q=np.abs(q - qo).max())
    print(f"{name}[{'host_loop' if flags else 'queued'}]: optimize iterations {n}/{ref['n']} trials {st.trials}/{st_o.trials} "
          + " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert (n, st.iterations, st.trials, st.result, st.solve_failures) == \
        (ref["n"], st_o.iterations, st_o.trials, st_o.result, st_o.solve_failures)
    assert figs["chi2_initial"] <= 1e-9 and figs["chi2_final"] <= 1e-7
    assert figs["t"] <= 1e-6 and figs["lm"] <= 1e-6 and figs["vel"] <= 1e-5 and figs["q"] <= 1e-7
    np.testing.assert_allclose(p.trial_chi2(), ref["c2"], rtol=1e-6, atol=1e-9)
    _, _, ok = p.eval()
    np.testing.assert_array_equal(ok, ref["ok"])
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unobserved", "one_free", "fixed_scattered"])
def test_inactive_vertices_untouched(name):
    """After optimize(10) every fixed keyframe, the keyframe without an edge and the landmarks without an
    observation come back from state() bit for bit as they went in: t, velocity and xyz as the caller passed
    them, the quaternion as lba_set_problem stored it (the caller's, normalised like the Sophus cast:
    include/amc_lba.h) -- the LM run changes no bit of it."""
    w = _win(name)
    p = amc_lba.Problem(w)
    kf0, lm0 = p.state()
    n, st = p.optimize(10)
    assert n > 0 and st.chi2_final < st.chi2_initial
    kf, lm = p.state()
    kf_act, lm_act = wm.active_vertices(w)
    kf_in = np.setdiff1d(np.arange(len(w.kfs)), kf_act)
    lm_in = np.setdiff1d(np.arange(len(w.lm)), lm_act)
    assert set(np.nonzero(w.kfs["fixed"])[0]) <= set(kf_in)
    if name == "unobserved":
        assert 5 in kf_in and list(lm_in) == [0, 7, 150, 299]
    for f in ("t", "vel", "time", "bf", "fixed"):
        np.testing.assert_array_equal(kf[f][kf_in], w.kfs[f][kf_in], err_msg=f)
    np.testing.assert_array_equal(kf["q"][kf_in], kf0["q"][kf_in])
    qn = w.kfs["q"] / np.linalg.norm(w.kfs["q"], axis=1, keepdims=True)
    assert np.abs(kf0["q"] - qn).max() <= 4 * np.finfo(float).eps        # set_problem: the caller's, normalised
    np.testing.assert_array_equal(lm[lm_in], w.lm[lm_in])
    np.testing.assert_array_equal(lm0, w.lm)
    # and the active ones did move
    assert np.all(np.abs(kf["t"][kf_act] - w.kfs["t"][kf_act]).max(axis=1) > 0)
    assert np.all(np.abs(lm[lm_act] - w.lm[lm_act]).max(axis=1) > 0)
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["base", "stereo_gp"])
def test_shuffle_equivariance_on_device(name):
    """linearize() on the shuffled window, mapped back through the permutations, is linearize() on the
    original up to the order of the sums: within 1e-11 relative and within 100 x the oracle's own figure for
    the same comparison.  optimize(10): the same trial count, states within 1e-8."""
    w = _win(name)
    ws, pr = wm.shuffled(w, seed=59)
    ref = _ref_linearize(name)
    o = orc.Oracle(ws)
    o.errors()
    sys_o = wm.unshuffle_system(*o.build_system(), w, ws, pr)
    own = [_rel(a, b) for a, b in zip(sys_o, (ref["H"], ref["b"], ref["Hll"]))]
    p, ps = amc_lba.Problem(w), amc_lba.Problem(ws)
    _, H, b, Hll = p.linearize()
    _, Hs, bs, Hlls = ps.linearize()
    dev = [_rel(a, b) for a, b in zip(wm.unshuffle_system(Hs, bs, Hlls, w, ws, pr), (H, b, Hll))]
    print(f"{name}: shuffle equivariance (H, b, Hll): device " + " ".join(f"{v:.2e}" for v in dev)
          + "; oracle " + " ".join(f"{v:.2e}" for v in own))
    for d, o_ in zip(dev, own):
        assert d <= 1e-11 and d <= 100 * max(o_, np.finfo(float).eps)
    n, st = p.optimize(10)
    ns, sts = ps.optimize(10)
    assert (n, st.trials, st.result) == (ns, sts.trials, sts.result)
    kf, lm = p.state()
    kfs, lms = wm.unshuffle_state(*ps.state(), pr)
    dt, dl = _state_diff(kfs, lms, kf, lm)
    print(f"{name}: device optimize vs its shuffle |dt| {dt:.2e} |dlm| {dl:.2e}")
    assert dt <= 1e-8 and dl <= 1e-8
    p.close()
    ps.close()


def _boundary_window(n):
    n_lm = {2: 30, 3: 40, 16: 200}.get(n, 2500)
    return make_window(n_opt_kf=n, n_fixed=1, n_lm=n_lm, obs_per_lm=5, n_cam=4, gp=True, global_ba=True, seed=50 + n)


SIZES = {   # pose dimension, panels of 32 rows, substitution solve by default
    "one_free": (12, 1, 0), 2: (24, 1, 0), 3: (36, 2, 0), 16: (192, 6, 0), 170: (2040, 64, 0), 171: (2052, 65, 1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("size", list(SIZES), ids=[str(s) for s in SIZES])
def test_small_and_boundary_pose_systems(size):
    """Pose systems of one block, of less than and exactly a whole number of 32-row panels, and either side
    of the panel count at which the substitution solve becomes the default: linearisation and one step at
    the window's lambda_init against the oracle."""
    w = _win("one_free") if size == "one_free" else _boundary_window(size)
    np_, panels, band = SIZES[size]
    p = amc_lba.Problem(w)
    info = p.solver_info()
    assert p.pose_dim == np_ and info["panels"] == panels and info["band"] == band
    o = orc.Oracle(w)
    chi, res, c2 = o.errors()
    H, b, Hll = o.build_system()
    ref = dict(chi=chi, res=res, c2=c2, H=H, b=b, Hll=Hll, ok=o.depth_ok(), np=o.pose_dim)
    _check_linearize(p, ref, f"size {size}")
    lam = w.cfg["lambda_init"]
    _check_step(p, o.solve(lam), (f"size {size}", lam))
    p.close()
