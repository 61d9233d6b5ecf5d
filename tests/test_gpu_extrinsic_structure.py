"""Extrinsic calibration (lba_cam.ext_free, LocalGPBA's bExtrinsic pass) on the device at its structural edges: the
windows of tests/extrinsic_cases.py against the oracle.

The free extrinsic has a branch of its own in the set-up, the sweep (side == 2), the sample expansion, the edge items,
the solve layout (a dense tail of panels), the update (the other camdb buffer) and the evaluation; the suite ran it on
one shape of window.  Here, per case: linearisation and evaluation at the project's max-norm limits and in the scaled
measures of tests/scaled.py; damped steps at two lambdas through the default, the substitution and the L^-1 solve; whole
LM runs in the queued and the host loop, against the oracle and against each other; what an LM run must not move;
and on chosen cases the extrinsic update alone, shuffle equivariance, engine reuse, the fp32-residual kernels and the
64 / 65-panel switch with the extrinsic tail.

Every limit is one the project states already (tests/test_gpu_window_structure.py, tests/scaled.py,
tests/test_gpu_f32_residual.py), a stated multiple of a figure the oracle gives on the CPU at test time, or a stated
condition; each is printed beside the value measured against it as an `ext_structure` line (pytest -s;
profiles/extrinsic_structure_margins.log holds one run).  The oracle references are built once per case.
"""
import functools
from dataclasses import replace

import numpy as np
import pytest

import amc_lba
import extrinsic_cases as X
import orc
import scaled as S
import test_gpu_window_structure as ws
import window_mutations as wm
from amc_lba.abi import CAM_DTYPE, FLAG_BAND_SOLVE, FLAG_DENSE_SOLVE, FLAG_F32_RESIDUAL, FLAG_HOST_LOOP

pytestmark = pytest.mark.gpu

CASE_NAMES = list(X.CASES)
SOLVES = {"default": 0, "band": FLAG_BAND_SOLVE, "dense": FLAG_DENSE_SOLVE}
LOOPS = {"queued": 0, "host_loop": FLAG_HOST_LOOP}
CAM_FIXED_FIELDS = CAM_DTYPE.names
CAM_KEPT_FIELDS = ("fx", "fy", "cx", "cy", "ext_free", "rbc_ini", "rbc_info")   # of a free camera


def _say(msg):
    print("ext_structure: " + msg)


# ------------------------------------------------------------------ references in the scaled measures (CPU, once)
def _lin_scaled(win, sys_, ref):
    """(scaled_sym H_pp, scaled_sym H_ll, scaled_rhs b) of a system against the oracle's on the window."""
    H, b, Hll = sys_
    return (S.scaled_sym(H, ref["H"]), S.scaled_sym(Hll.reshape(-1, 3, 3), ref["Hll"].reshape(-1, 3, 3)),
            S.scaled_rhs(b, ref["b"], S.full_diag(win, ref["H"], ref["Hll"]), ref["chi"]))


@functools.lru_cache(maxsize=None)
def _lin_limits(name):
    """Per measure: max(T_LIN, 8 x the measure of the oracle's system on the shuffle against its system on the
    window), and that second figure."""
    own = _lin_scaled(X.window(name), X.ref_shuffle(name)["sys"], X.ref_linearize(name))
    return tuple(max(S.T_LIN, 8 * v) for v in own), own


def _parts(dx, x, D, win, pose_dim):
    """scaled_step of (whole, pose part, landmark part, extrinsic rows alone)."""
    e = X.ext_rows(win)
    return S.scaled_step_parts(dx, x, D, pose_dim) + (S.scaled_step(dx[e], x[e], D[e]),)


@functools.lru_cache(maxsize=None)
def _step_ref(name, lam):
    """refined_solve of the oracle's system at lambda with its Jacobi scaling and kappa_s, and r_o: the oracle's own
    scaled_step / (kappa_s u) on that system."""
    win = X.window(name)
    o = orc.Oracle(win)
    o.errors()
    o.build_system()
    A, rhs = S.system(o, lam)
    ok_o, dx_o = X.ref_linearize(name)["steps"][lam]
    assert ok_o
    D, kappa, x = S.jacobi(A), S.kappa_scaled(A), S.refined_solve(A, rhs)
    ku = kappa * S.U
    own = _parts(dx_o, x, D, win, o.pose_dim)
    return dict(D=D, kappa=kappa, x=x, ku=ku, r_o=own[0] / ku, own=tuple(v / ku for v in own))


# ------------------------------------------------------------------ device runs, once per (case, flags)
@functools.lru_cache(maxsize=None)
def _gpu_steps(name, solve):
    p = amc_lba.Problem(X.window(name), flags=SOLVES[solve])
    band = p.solver_info()["band"]
    p.linearize()
    out = {lam: p.solve_step(lam) for lam in X.LAMBDAS}
    p.close()
    return band, out


@functools.lru_cache(maxsize=None)
def _gpu_optimize(name, loop):
    p = amc_lba.Problem(X.window(name), flags=LOOPS[loop])
    kf0, lm0 = p.state()
    n, st = p.optimize(10)
    kf, lm = p.state()
    _, _, ok = p.eval()
    r = dict(n=n, st=st.as_dict(), kf0=kf0, lm0=lm0, kf=kf, lm=lm, cams=p.cams(), c2=p.trial_chi2(), ok=ok)
    p.close()
    return r


# ------------------------------------------------------------------ 1. linearisation
@pytest.mark.parametrize("name", CASE_NAMES)
def test_linearize_matches_oracle(name):
    """linearize() and eval() at the limits of tests/test_gpu_window_structure.py (residuals 1e-8, H_pp, b, H_ll 1e-9
    max-norm, chi2 1e-9, per-observation chi2 rtol 1e-8 / atol 1e-10, depth_ok identical), and H_pp, H_ll and b in the
    scaled measures within max(T_LIN, 8 x the oracle's own shuffle spread).  A structurally zero row that is not
    exactly zero makes a scaled measure inf (ext_unseen_cam)."""
    win, ref = X.window(name), X.ref_linearize(name)
    p = amc_lba.Problem(win)
    sys_ = ws._check_linearize(p, ref, name)
    p.close()
    v = _lin_scaled(win, sys_, ref)
    lim, own = _lin_limits(name)
    _say(f"lin  {name}: scaled H {v[0]:.3e} Hll {v[1]:.3e} b {v[2]:.3e} | oracle vs its shuffle "
         f"{own[0]:.3e} {own[1]:.3e} {own[2]:.3e} | limits {lim[0]:.3e} {lim[1]:.3e} {lim[2]:.3e} (T_LIN {S.T_LIN:.3e})")
    for a, b in zip(v, lim):
        assert a <= b, (v, lim)


# ------------------------------------------------------------------ 2. damped steps
@pytest.mark.parametrize("solve", list(SOLVES))
@pytest.mark.parametrize("lam", X.LAMBDAS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_step_matches_oracle(name, lam, solve):
    """Pose part (keyframes and extrinsics) and landmark part within 1e-6 max-norm of the oracle's step; the whole
    vector, the pose part, the landmark part and the extrinsic rows alone within max(M_STEP, 4 r_o) kappa_s u of
    refined_solve of the oracle's system in scaled_step; solver_info()["band"] follows the flag."""
    win, ref = X.window(name), X.ref_linearize(name)
    band, steps = _gpu_steps(name, solve)
    assert band == (1 if solve == "band" else 0)
    ok_o, dx_o = ref["steps"][lam]
    ok, dx = steps[lam]
    assert ok == ok_o and dx.shape == dx_o.shape
    n = ref["np"]
    rp, rl = X.rel(dx[:n], dx_o[:n]), X.rel(dx[n:], dx_o[n:])
    R = _step_ref(name, lam)
    v = tuple(a / R["ku"] for a in _parts(dx, R["x"], R["D"], win, n))
    lim = max(S.M_STEP, 4 * R["r_o"])
    _say(f"step {name} [{solve}] lambda {lam:g}: max-norm pose {rp:.2e} lm {rl:.2e} (limit 1e-06) | kappa_s "
         f"{R['kappa']:.3e} err/(kappa_s u) whole {v[0]:.3f} pose {v[1]:.3f} lm {v[2]:.3f} ext {v[3]:.3f} | oracle "
         + " ".join(f"{a:.3f}" for a in R["own"]) + f" | limit {lim:.3f} (M_STEP {S.M_STEP:.3f}, r_o {R['r_o']:.3f})")
    assert rp <= 1e-6 and rl <= 1e-6
    for a in v:
        assert a <= lim, (v, lim)
    if name == "ext_unseen_cam":
        z = dx[X.ext_rows(win)[:3]]
        assert np.all(z == 0.0), z


# ------------------------------------------------------------------ 3. LM runs
@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_optimize_matches_oracle(name, loop):
    ref, r = X.ref_optimize(name), _gpu_optimize(name, loop)
    st, st_o = r["st"], ref["st"]
    figs = X.state_figures(r["kf"], r["lm"], r["cams"], ref["kf"], ref["lm"], ref["cams"])
    c0 = abs(st["chi2_initial"] - st_o.chi2_initial) / st_o.chi2_initial
    c1 = abs(st["chi2_final"] - st_o.chi2_final) / st_o.chi2_final
    _say(f"lm   {name} [{loop}]: iterations {r['n']}/{ref['n']} trials {st['trials']}/{st_o.trials} result "
         f"{st['result']}/{st_o.result} chi2_initial {c0:.2e} (1e-09) chi2_final {c1:.2e} (1e-07) "
         + " ".join(f"{k} {v:.2e} ({X.STATE_LIMITS[k]:g})" for k, v in figs.items()))
    assert (r["n"], st["iterations"], st["trials"], st["result"], st["solve_failures"]) == \
        (ref["n"], st_o.iterations, st_o.trials, st_o.result, st_o.solve_failures)
    assert c0 <= 1e-9 and c1 <= 1e-7
    for k, v in figs.items():
        assert v <= X.STATE_LIMITS[k], (k, v)
    np.testing.assert_allclose(r["c2"], ref["c2"], rtol=1e-6, atol=1e-9)
    np.testing.assert_array_equal(r["ok"], ref["ok"])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_queued_and_host_loop_agree_bit_for_bit(name):
    """LBA_FLAG_HOST_LOOP: "same results" (include/amc_lba.h)."""
    a, b = _gpu_optimize(name, "queued"), _gpu_optimize(name, "host_loop")
    for k in ("iterations", "trials", "result", "solve_failures", "chi2_initial", "chi2_final", "lambda_final"):
        assert a["st"][k] == b["st"][k], k
    assert a["n"] == b["n"]
    for k in ("kf", "lm", "cams", "c2", "ok"):
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------ 4. what must not move
@pytest.mark.parametrize("name", CASE_NAMES)
def test_fixed_vertices_and_records_untouched(name):
    """After optimize(10): a camera with ext_free == 0 comes back from cams() bit for bit in every field, a free one
    in its intrinsics, rbc_ini and rbc_info; fixed and inactive keyframes and unobserved landmarks come back as
    test_gpu_window_structure.test_inactive_vertices_untouched states; every active vertex moved."""
    w, r = X.window(name), _gpu_optimize(name, "queued")
    kf_act, lm_act, free = X.active_vertices(w)
    cams, kf, lm = r["cams"], r["kf"], r["lm"]
    fixed_cams = np.setdiff1d(np.arange(len(w.cams)), free)
    assert len(w.cams) - 1 in fixed_cams                     # the reference camera
    for f in CAM_FIXED_FIELDS:
        assert cams[f][fixed_cams].tobytes() == np.ascontiguousarray(w.cams[f][fixed_cams]).tobytes(), f
    for f in CAM_KEPT_FIELDS:
        assert cams[f][free].tobytes() == np.ascontiguousarray(w.cams[f][free]).tobytes(), f
    kf_in = np.setdiff1d(np.arange(len(w.kfs)), kf_act)
    lm_in = np.setdiff1d(np.arange(len(w.lm)), lm_act)
    assert set(np.nonzero(w.kfs["fixed"])[0]) <= set(kf_in)
    for f in ("t", "vel", "time", "bf", "fixed"):
        np.testing.assert_array_equal(kf[f][kf_in], w.kfs[f][kf_in], err_msg=f)
    np.testing.assert_array_equal(kf["q"][kf_in], r["kf0"]["q"][kf_in])
    qn = w.kfs["q"] / np.linalg.norm(w.kfs["q"], axis=1, keepdims=True)
    assert np.abs(r["kf0"]["q"] - qn).max() <= 4 * np.finfo(float).eps
    np.testing.assert_array_equal(lm[lm_in], w.lm[lm_in])
    np.testing.assert_array_equal(r["lm0"], w.lm)
    assert np.all(np.abs(kf["t"][kf_act] - w.kfs["t"][kf_act]).max(axis=1) > 0) if len(kf_act) else True
    assert np.all(np.abs(lm[lm_act] - w.lm[lm_act]).max(axis=1) > 0)
    assert np.all(np.abs(cams["q"][free] - w.cams["q"][free]).max(axis=1) > 0)
    if name == "ext_calib_only":
        assert len(kf_in) == len(w.kfs) and len(free) == 3
    if name == "ext_one_cam":
        assert list(fixed_cams) == [0, 2, 3]
    if name == "ext_unseen_cam":
        assert cams["t"][0].tobytes() == w.cams["t"][0].tobytes()
        seen = free[free != 0]
        assert np.all(np.abs(cams["t"][seen] - w.cams["t"][seen]).max(axis=1) > 0)
    else:
        assert np.all(np.abs(cams["t"][free] - w.cams["t"][free]).max(axis=1) > 0)


# ------------------------------------------------------------------ 5. the extrinsic update alone
@pytest.mark.parametrize("name", ["ext_base", "ext_big_step", "ext_full_info"])
def test_extrinsic_update_isolated_from_the_solve(name):
    """k_update's Tbc <- Tbc exp(d) alone.  lba_trial_state returns no cameras, so: problem A linearises and solves at
    lambda_init (dx and its trial state), problem B runs optimize(1) with early_stop = 0, whose first trial the oracle
    accepts.  B's keyframes and landmarks are A's trial state bit for bit, i.e. B applied that dx; then B's cameras
    are within 8 u of the long-double oplus_cams(win, dx): sign-aligned q absolute, t by scaled.state_deviation's
    rule (the measure and limit of test_gpu_scaled_parity.test_update_isolated_from_the_solve)."""
    w = X.window(name)
    lam = w.cfg.get("lambda_init", 1.0)
    o = orc.Oracle(w, early_stop=0)
    n_o, st_o = o.optimize(1)
    assert (n_o, st_o.trials) == (1, 1) and st_o.chi2_final < st_o.chi2_initial   # the first trial is accepted
    a = amc_lba.Problem(w)
    a.linearize()
    ok, dx = a.solve_step(lam)
    kf_a, lm_a = a.trial_state()
    a.close()
    b = amc_lba.Problem(w, early_stop=0)
    n, st = b.optimize(1)
    kf_b, lm_b = b.state()
    cams = b.cams()
    b.close()
    assert ok and (n, st.trials) == (1, 1)
    assert kf_b.tobytes() == kf_a.tobytes() and lm_b.tobytes() == lm_a.tobytes()
    q, t = X.oplus_cams(w, dx)
    dev = X.cam_deviation(cams["q"], cams["t"], q, t)
    oc = o.cams()
    # (the oracle applied its own dx: its figure is the two solves' difference, not an update error)
    own = X.cam_deviation(oc["q"], oc["t"], q, t)
    _say(f"upd  {name}: cameras vs long-double oplus of the device's dx, in u: q {dev['q']:.2f} t {dev['t']:.2f} "
         f"(limit 8) | oracle's cameras vs the same {own['q']:.2f} {own['t']:.2f}")
    assert dev["q"] <= 8 and dev["t"] <= 8, dev
    free = X.free_cams(w)
    assert np.all(np.abs(cams["t"][free] - w.cams["t"][free]).max(axis=1) > 0)


# ------------------------------------------------------------------ 6. shuffle equivariance on the device
@pytest.mark.parametrize("name", ["ext_base", "ext_fixed_scattered"])
def test_shuffle_equivariance_on_device(name):
    """test_gpu_window_structure.test_shuffle_equivariance_on_device with the extrinsic tail: (H, b, H_ll) of the
    shuffled window mapped back within 1e-11 and 100 x the oracle's own figure; optimize(10) with the same trial
    counts; keyframes, landmarks and cameras within max(1e-8, 8 x the oracle's own spread) (absolute; q sign-aligned)."""
    w, ref, sh, opt = X.window(name), X.ref_linearize(name), X.ref_shuffle(name), X.ref_optimize(name)
    ws_, pr = sh["win"], sh["perms"]
    own = [X.rel(a, b) for a, b in zip(sh["sys"], (ref["H"], ref["b"], ref["Hll"]))]
    p, ps = amc_lba.Problem(w), amc_lba.Problem(ws_)
    _, H, b, Hll = p.linearize()
    _, Hs, bs, Hlls = ps.linearize()
    dev = [X.rel(a, b) for a, b in zip(X.unshuffle_system(Hs, bs, Hlls, w, ws_, pr), (H, b, Hll))]
    _say(f"shuf {name}: (H, b, Hll) device " + " ".join(f"{v:.2e}" for v in dev) + " | oracle "
         + " ".join(f"{v:.2e}" for v in own) + " | limit min(1e-11, 100 x oracle)")
    for d, o_ in zip(dev, own):
        assert d <= 1e-11 and d <= 100 * max(o_, np.finfo(float).eps)
    n, st = p.optimize(10)
    ns, sts = ps.optimize(10)
    assert (n, st.trials, st.result) == (ns, sts.trials, sts.result)
    kf, lm = p.state()
    kfs, lms = wm.unshuffle_state(*ps.state(), pr)
    cams, cams_s = p.cams(), ps.cams()
    p.close()
    ps.close()

    def spread(a, b):   # (states a and b: (kf, lm, cams))
        return {"kf_t": np.abs(a[0]["t"] - b[0]["t"]).max(), "kf_vel": np.abs(a[0]["vel"] - b[0]["vel"]).max(),
                "kf_q": X.quat_diff(a[0]["q"], b[0]["q"]), "lm": np.abs(a[1] - b[1]).max(),
                "cam_t": np.abs(a[2]["t"] - b[2]["t"]).max(), "cam_q": X.quat_diff(a[2]["q"], b[2]["q"])}
    d = spread((kfs, lms, cams_s), (kf, lm, cams))
    o_ = spread((sh["kf"], sh["lm"], sh["cams"]), (opt["kf"], opt["lm"], opt["cams"]))
    _say(f"shuf {name}: optimize, device vs its shuffle | oracle vs its shuffle | limit: "
         + " ".join(f"{k} {d[k]:.2e} | {o_[k]:.2e} | {max(1e-8, 8 * o_[k]):.2e};" for k in d))
    for k in d:
        assert d[k] <= max(1e-8, 8 * o_[k]), (k, d[k], o_[k])


# ------------------------------------------------------------------ 7. engine reuse
def _lin_bytes(p):
    """(as tests/test_gpu_sweep_inputs.py: the dense H_pp of lba_linearize is left out, its mirrored stores race)"""
    res, _, b, Hll = p.linearize()
    ok, dx = p.solve_step(1.0)
    return res.tobytes(), b.tobytes(), Hll.tobytes(), bool(ok), dx.tobytes()


def _run_bytes(p):
    n, st = p.optimize(10)
    kf, lm = p.state()
    return n, st.trials, st.result, st.chi2_final, st.lambda_final, kf.tobytes(), lm.tobytes(), p.cams().tobytes()


def test_engine_reuse_across_fixed_and_free_extrinsics_is_bitwise_fresh():
    """One engine through fixed-extrinsic and free-extrinsic windows in turn, as the adapter calls it: the
    linearisation and an optimize(10) run, cams() included, are bit for bit a fresh engine's at every stop (a stale
    trial camera record, keyframe-to-camera map, prior count or prior data would show)."""
    wins = {"base": wm.base()}
    seq = ["base", "ext_base", "ext_one_cam", "base", "ext_cams_9", "ext_calib_only", "ext_base"]
    p = None
    for i, name in enumerate(seq):
        w = wins[name] if name in wins else X.window(name)
        if p is None:
            p = amc_lba.Problem(w, early_stop=0)
        else:
            p.set_window(replace(w, cfg=dict(w.cfg, early_stop=0)))
        got = _lin_bytes(p) + _run_bytes(p)
        f = amc_lba.Problem(w, early_stop=0)
        want = _lin_bytes(f) + _run_bytes(f)
        f.close()
        labels = ("res", "b", "Hll", "ok", "dx", "n", "trials", "result", "chi2_final", "lambda_final", "kf", "lm", "cams")
        diff = [l for l, x, y in zip(labels, got, want) if x != y]
        _say(f"reuse stop {i} {name}: differing outputs {diff or 'none'}")
        assert not diff, (i, name, diff)
    p.close()


# ------------------------------------------------------------------ 8. fp32 residuals
@pytest.mark.parametrize("name", ["ext_base", "ext_fixed_scattered", "ext_heavy"])
def test_f32_residual_within_tolerance(name):
    """LBA_FLAG_F32_RESIDUAL with free extrinsics at the tolerances of tests/test_gpu_f32_residual.py (residual 1e-3
    and above fp64 rounding, H 1e-5, b 1e-4, chi2 1e-4, step 1e-3; optimize(10) with early_stop = 0: chi2 1e-3,
    keyframe t and landmarks 1e-3), the cameras' q and t at the keyframe-state tolerance 1e-3."""
    w, ref = X.window(name), X.ref_linearize(name)
    p = amc_lba.Problem(w, flags=FLAG_F32_RESIDUAL)
    assert p.kernel_modes()["f32res"] == 1
    res, H, b, _ = p.linearize()
    dres = np.linalg.norm(res - ref["res"]) / np.linalg.norm(ref["res"])
    dH, db = X.rel(H, ref["H"]), X.rel(b, ref["b"])
    chi, _, _ = p.eval()
    dchi = abs(chi - ref["chi"]) / ref["chi"]
    ok, dx = p.solve_step(1.0)
    ok_o, dx_o = ref["steps"][1.0]
    ddx = X.rel(dx, dx_o)
    p.close()
    _say(f"f32  {name}: residual {dres:.2e} (1e-9 .. 1e-3) H {dH:.2e} (1e-5) b {db:.2e} (1e-4) chi2 {dchi:.2e} (1e-4) "
         f"dx {ddx:.2e} (1e-3)")
    assert 1e-9 < dres <= 1e-3, dres
    assert dH <= 1e-5 and db <= 1e-4, (dH, db)
    assert dchi <= 1e-4 and ok and ok_o and ddx <= 1e-3, (dchi, ddx)
    r = X._optimized(w, early_stop=0)
    p = amc_lba.Problem(w, early_stop=0, flags=FLAG_F32_RESIDUAL)
    n, st = p.optimize(10)
    kf, lm = p.state()
    cams = p.cams()
    p.close()
    st_o = r["st"]
    dchi = abs(st.chi2_final - st_o.chi2_final) / st_o.chi2_final
    f = X.state_figures(kf, lm, cams, r["kf"], r["lm"], r["cams"])
    _say(f"f32  {name}: optimize iterations {n}/{r['n']} trials {st.trials}/{st_o.trials} chi2 {dchi:.2e} kf t "
         f"{f['kf_t']:.2e} lm {f['lm']:.2e} cam q {f['cam_q']:.2e} cam t {f['cam_t']:.2e} (each 1e-3)")
    assert n == r["n"] and st.chi2_final < st.chi2_initial
    assert dchi <= 1e-3 and f["kf_t"] <= 1e-3 and f["lm"] <= 1e-3, (dchi, f)
    assert f["cam_q"] <= 1e-3 and f["cam_t"] <= 1e-3, f


# ------------------------------------------------------------------ 9. panel boundaries with the dense tail
BOUNDARY = {167: (2022, 64, 0), 168: (2034, 65, 1)}   # pose dimension, panels of 32 rows, substitution solve by default


@pytest.mark.parametrize("n", list(BOUNDARY))
def test_panel_switch_with_the_extrinsic_tail(n):
    """Either side of the panel count at which the substitution solve becomes the default, the last panel holding the
    three extrinsic blocks: linearisation as in test_linearize_matches_oracle (the scaled measures included) and one
    step of the default solve at the window's lambda_init, max-norm 1e-6."""
    w = X.boundary_window(n)
    np_, panels, band = BOUNDARY[n]
    assert [v[1:] for v in BOUNDARY.values()] == [(64, 0), (65, 1)]        # the two sizes straddle the switch
    p = amc_lba.Problem(w)
    info = p.solver_info()
    assert p.pose_dim == np_ and (info["panels"], info["band"]) == (panels, band), info
    o = orc.Oracle(w)
    chi, res, c2 = o.errors()
    H, b, Hll = o.build_system()
    ref = dict(chi=chi, res=res, c2=c2, H=H, b=b, Hll=Hll, ok=o.depth_ok(), np=o.pose_dim)
    sys_ = ws._check_linearize(p, ref, f"boundary {n}")
    lam = w.cfg["lambda_init"]
    ws._check_step(p, o.solve(lam), (f"boundary {n}", lam))
    p.close()
    w2, pr = wm.shuffled(w, seed=X.SHUFFLE_SEED)
    o2 = orc.Oracle(w2)
    o2.errors()
    own = _lin_scaled(w, X.unshuffle_system(*o2.build_system(), w, w2, pr), ref)
    v = _lin_scaled(w, sys_, ref)
    lim = tuple(max(S.T_LIN, 8 * x) for x in own)
    _say(f"lin  boundary {n}: panels {info['panels']} band {info['band']} scaled H {v[0]:.3e} Hll {v[1]:.3e} b {v[2]:.3e} "
         f"| oracle vs its shuffle {own[0]:.3e} {own[1]:.3e} {own[2]:.3e} | limits {lim[0]:.3e} {lim[1]:.3e} {lim[2]:.3e}")
    for a, l in zip(v, lim):
        assert a <= l, (v, lim)


@pytest.mark.parametrize("name,n_kf", [("ext_aligned_8", 8), ("ext_aligned_16", 16)])
def test_tail_starts_on_a_panel_edge(name, n_kf):
    """12 * 8 = 96 and 12 * 16 = 192 keyframe rows are whole panels, so the first extrinsic row is the first row of a
    panel.  The set-up's pose dimension counts each of the three extrinsic blocks 12 wide (V.np = 12 * n_pb), so
    96 + 36 = 132 rows make 5 panels and 192 + 36 = 228 rows make 8."""
    w = X.window(name)
    kf, _, free = X.active_vertices(w)
    assert len(kf) == n_kf and (12 * n_kf) % 32 == 0 and len(free) == 3
    panels = -(-12 * (n_kf + 3) // 32)
    assert panels == {8: 5, 16: 8}[n_kf]
    p = amc_lba.Problem(w)
    info = p.solver_info()
    p.close()
    _say(f"tail {name}: panels {info['panels']} (expected {panels}), band {info['band']}")
    assert info["panels"] == panels and info["band"] == 0
