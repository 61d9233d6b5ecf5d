"""The windows of tests/extrinsic_cases.py on the CPU: each has the property it is named for (counted in numpy), the
oracle gives it the pose dimension of the table, lba_setup_host_profile (lba_set_problem's host preprocessing, no
device) accepts it with the same pose blocks and device-landmark count, and the oracle agrees with itself on a shuffle
of the window within the limits tests/test_gpu_extrinsic_structure.py holds the GPU to (so those limits bound the
engine, not the conditioning of the case).  The spreads are printed (pytest -s;
profiles/extrinsic_structure_margins.log holds one run).
"""
import numpy as np
import pytest

import amc_lba
import extrinsic_cases as X
import orc
import test_gpu_window_structure as ws
import window_mutations as wm
from amc_lba.abi import MONO, MONO_GP, STEREO_GP

CASE_NAMES = list(X.CASES)
NO_REJECTED_TRIAL = {"ext_one_cam", "ext_shared_stamp_one", "ext_stereo_gp_mixed", "ext_cams_20", "ext_aligned_8",
                     "ext_aligned_16"}
CHOL_NB, ST_CAMS = 32, 8   # rows of a panel of the reduced system, cameras k_lin_schur stages in LDS


def test_tables_cover_the_cases():
    assert list(X.TABLE) == CASE_NAMES and len(CASE_NAMES) == 22


# ------------------------------------------------------------------ the property of each case
def _both_fixed_per_cam(win):
    o = win.obs
    fixed = win.kfs["fixed"] != 0
    gp = wm.is_gp(o)
    both = gp & fixed[np.maximum(o["kf_a"], 0)] & fixed[o["kf_b"]]
    return [int((both & (o["cam"] == c)).sum()) for c in range(len(win.cams))]


def _prop_ext_base(w):
    assert w.cams["ext_free"].tolist() == [1, 1, 1, 0] and list(np.nonzero(w.kfs["fixed"])[0]) == [0]
    b = wm.base()
    assert np.array_equal(w.obs, b.obs) and np.array_equal(w.kfs, b.kfs)
    assert not np.array_equal(w.cams["q"][:3], b.cams["q"][:3]) and np.array_equal(w.cams["rbc_ini"], b.cams["rbc_ini"])


def _prop_fixed_scattered(w):
    assert list(np.nonzero(w.kfs["fixed"])[0]) == [0, 4, 5, 10]
    # GP samples whose only optimisable vertex is the extrinsic, per free camera
    assert _both_fixed_per_cam(w) == [58, 47, 59, 0]
    assert np.all(w.obs["kind"][wm.is_gp(w.obs) & (w.obs["cam"] < 3)] == MONO_GP)


def _prop_fixed_only_landmarks(w):
    o = w.obs
    fixed = w.kfs["fixed"] != 0
    for l in range(12):
        s = o[o["lm"] == l]
        assert len(s) == 2 and np.all(s["kind"] == MONO) and np.all(fixed[s["kf_b"]])
        assert np.all(s["cam"] == 3) and w.cams["ext_free"][3] == 0        # no free keyframe, no free extrinsic
    assert np.all(ws._free_blocks_per_landmark(w)[:12] == 0)


def _prop_calib_only(w):
    assert np.all(w.kfs["fixed"] != 0) and len(wm.active_vertices(w)[0]) == 0
    assert len(w.priors) > 0 and len(w.vel_kfs) > 0    # listed, and inactive: every end of every one is fixed
    assert X.pose_dim(w) == 6 * 3 and sum(_both_fixed_per_cam(w)) == int(wm.is_gp(w.obs).sum())


def _prop_one_free(w):
    assert list(np.nonzero(w.kfs["fixed"] == 0)[0]) == [5]
    kf, _, cams = X.active_vertices(w)
    assert (len(kf), len(cams)) == (1, 3)


def _prop_one_cam(w):
    assert w.cams["ext_free"].tolist() == [0, 1, 0, 0]


def _prop_two_cams(w):
    assert w.cams["ext_free"].tolist() == [1, 0, 1, 0]


def _prop_unseen_cam(w):
    assert w.cams["ext_free"][0] == 1 and not np.any(w.obs["cam"] == 0) and np.any(X.ext_base().obs["cam"] == 0)
    o = orc.Oracle(w)
    o.errors()
    H, _, _ = o.build_system()
    zero = np.nonzero(np.diag(H) == 0.0)[0]
    assert list(zero) == list(X.ext_rows(w)[:3])       # [upsilon, omega]: the translation rows of camera 0's block


def _prop_unobserved(w):
    kf, lm, cams = X.active_vertices(w)
    assert 5 not in kf and w.kfs["fixed"][5] == 0 and len(kf) == 9
    assert list(np.setdiff1d(np.arange(len(w.lm)), lm)) == [0, 7, 150, 299] and len(cams) == 3


def _prop_shuffled(w):
    assert np.any(np.diff(w.obs["lm"]) < 0) and np.any(np.diff(w.kfs["time"]) < 0) and w.kfs["fixed"][0] == 0
    gp = wm.is_gp(w.obs)
    assert np.any(w.obs["kf_a"][gp] != w.obs["kf_b"][gp] - 1)
    assert np.array_equal(w.cams, X.ext_base().cams)


def _prop_skip_pairs(w):
    per_b = ws._pairs_per_kf_b(w)
    assert np.all(per_b[3:] == 2) and per_b.max() == 2


def _prop_endpoint_times(w):
    o = w.obs[wm.is_gp(w.obs)]
    c0, c1 = o[o["cam"] == 0], o[o["cam"] == 1]
    assert len(c0) > 100 and len(c1) > 100 and w.cams["ext_free"][0] and w.cams["ext_free"][1]
    assert np.array_equal(c0["t"], w.kfs["time"][c0["kf_b"]]) and np.array_equal(c1["t"], w.kfs["time"][c1["kf_a"]])


def _shared_times(w):
    """GP pairs on which cameras 0 and 1 have one time stamp in common: that time has two sample keys."""
    o = w.obs[wm.is_gp(w.obs)]
    n = 0
    for k in np.unique(o["kf_b"]):
        t0, t1 = (np.unique(o["t"][(o["kf_b"] == k) & (o["cam"] == c)]) for c in (0, 1))
        if len(t0) and len(t1):
            assert np.array_equal(t0, t1)
            n += 1
    return n


def _prop_shared_stamp(w):
    assert _shared_times(w) >= 8 and w.cams["ext_free"].tolist() == [1, 1, 1, 0]


def _prop_shared_stamp_one(w):
    assert _shared_times(w) >= 8 and w.cams["ext_free"].tolist() == [0, 1, 0, 0]


def _prop_stereo_gp_mixed(w):
    sgp = w.obs["kind"] == STEREO_GP
    assert w.cams["ext_free"].tolist() == [0, 1, 0, 0]
    assert int(sgp.sum()) == 412 and set(w.obs["cam"][sgp]) == {0, 2}
    c1 = w.obs[w.obs["cam"] == 1]
    assert len(c1) > 100 and np.all(c1["kind"] == MONO_GP) and np.all(c1["z"][:, 2] == 0.0)


def _prop_heavy(w):
    sh = amc_lba.setup_tile_shapes(w)
    assert sh["seg_tiles"] >= 2 and sh["seg_obs"] > 0, sh


def _prop_cams_9(w):
    assert len(w.cams) == ST_CAMS + 1 and int(w.cams["ext_free"].sum()) == 8 and w.cams["ext_free"][8] == 0
    assert len(np.unique(w.obs["cam"])) == 9


def _prop_cams_20(w):
    assert len(w.cams) == 20 and int(w.cams["ext_free"].sum()) == 19
    assert ws._max_times_per_pair_and_piece(w) > ws.KC_INLINE


def _prop_big_step(w):
    r = X.ref_optimize("ext_big_step")
    assert r["st"].trials > r["st"].iterations and r["st"].result == 1


def _prop_full_info(w):
    b = X.ext_base()
    for c in range(3):
        info = w.cams["rbc_info"][c].reshape(3, 3)
        assert np.array_equal(info, info.T) and np.all(np.linalg.eigvalsh(info) > 0)
        assert np.all(info[~np.eye(3, dtype=bool)] != 0.0)
        assert np.array_equal(info, (c + 1) * X.INFO)
        r = w.cams["rbc_ini"][c]
        assert np.array_equal(r, r.astype(np.float32).astype(np.float64)) and abs(np.linalg.norm(r) - 1) < 1e-6
        assert np.abs(r - b.cams["rbc_ini"][c]).max() > 1e-3
        # the prior's residual at entry is a rotation of more than 0.5 degrees
        q = w.cams["q"][c] / np.linalg.norm(w.cams["q"][c])
        assert 2 * np.arccos(min(1.0, abs(float(q @ r)) / np.linalg.norm(r))) > np.deg2rad(0.5)
    assert np.array_equal(w.cams["rbc_info"][3], b.cams["rbc_info"][3])


def _prop_aligned(n):
    def check(w):
        kf, _, cams = X.active_vertices(w)
        assert len(kf) == n and (12 * n) % CHOL_NB == 0 and len(cams) == 3
    return check


PROPERTIES = {
    "ext_base": _prop_ext_base, "ext_fixed_scattered": _prop_fixed_scattered,
    "ext_fixed_only_landmarks": _prop_fixed_only_landmarks, "ext_calib_only": _prop_calib_only,
    "ext_one_free": _prop_one_free, "ext_one_cam": _prop_one_cam, "ext_two_cams": _prop_two_cams,
    "ext_unseen_cam": _prop_unseen_cam, "ext_unobserved": _prop_unobserved, "ext_shuffled": _prop_shuffled,
    "ext_skip_pairs": _prop_skip_pairs, "ext_endpoint_times": _prop_endpoint_times,
    "ext_shared_stamp": _prop_shared_stamp, "ext_shared_stamp_one": _prop_shared_stamp_one,
    "ext_stereo_gp_mixed": _prop_stereo_gp_mixed, "ext_heavy": _prop_heavy, "ext_cams_9": _prop_cams_9,
    "ext_cams_20": _prop_cams_20, "ext_big_step": _prop_big_step, "ext_full_info": _prop_full_info,
    "ext_aligned_8": _prop_aligned(8), "ext_aligned_16": _prop_aligned(16),
}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_has_its_property(name):
    PROPERTIES[name](X.window(name))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_pose_dimension(name):
    w = X.window(name)
    o = orc.Oracle(w)
    _, lm, _ = X.active_vertices(w)
    assert o.pose_dim == X.pose_dim(w) == X.TABLE[name][0]
    assert o.lm_dim == 3 * len(lm)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_setup_accepts_the_window(name):
    """lba_setup_host_profile: no error code (raises LbaError otherwise), one pose block per active keyframe and per
    free extrinsic, the device-landmark count of the observed landmarks.  The set-up's own dimension counts every
    block 12 wide (an extrinsic's block has 6 rows that exist, pose_ext); less those 6 per extrinsic it is the pose
    dimension of the oracle and of lba_pose_dim."""
    w = X.window(name)
    _, cnt = amc_lba.setup_host_profile(w)
    kf, lm, cams = X.active_vertices(w)
    assert int(cnt[1]) == len(kf) + len(cams) and int(cnt[2]) == 12 * int(cnt[1])
    assert int(cnt[2]) - 6 * len(cams) == orc.Oracle(w).pose_dim == X.TABLE[name][0]
    assert int(cnt[0]) == len(lm) and int(cnt[3]) >= 1


@pytest.mark.parametrize("n,np_", [(167, 2022), (168, 2034)])
def test_boundary_windows(n, np_):
    w = X.boundary_window(n)
    _, cnt = amc_lba.setup_host_profile(w)
    assert X.pose_dim(w) == np_ and int(cnt[2]) - 18 == np_ and w.cfg["lambda_init"] == 1e-5


# ------------------------------------------------------------------ the oracle against its own shuffle
@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_agrees_with_itself_under_shuffle(name):
    """optimize(10) on the window and on wm.shuffled(window, seed=59): the same (iterations, trials, result), and
    every output the GPU test compares within that test's limit for it, in that test's measure (X.STATE_LIMITS).  A
    condition on the case: only the order of the sums and of the elimination differs between the two runs."""
    ref, sh = X.ref_optimize(name), X.ref_shuffle(name)
    st, sts = ref["st"], sh["st"]
    assert (sh["n"], sts.iterations, sts.trials, sts.result) == (ref["n"], st.iterations, st.trials, st.result)
    assert (ref["n"], st.trials) == X.TABLE[name][1]
    assert (st.trials > st.iterations) == (name not in NO_REJECTED_TRIAL)
    figs = X.state_figures(sh["kf"], sh["lm"], sh["cams"], ref["kf"], ref["lm"], ref["cams"])
    absolute = (np.abs(sh["lm"] - ref["lm"]).max(), np.abs(sh["cams"]["t"] - ref["cams"]["t"]).max())
    print(f"ext_cases: {name}: oracle vs its shuffle: iterations {ref['n']} trials {st.trials} result {st.result} | "
          + " ".join(f"{k} {v:.2e} (limit {X.STATE_LIMITS[k]:g})" for k, v in figs.items())
          + f" | absolute: lm {absolute[0]:.2e} cam t {absolute[1]:.2e}")
    for k, v in figs.items():
        assert v <= X.STATE_LIMITS[k], (k, v)


# ------------------------------------------------------------------ ext_unseen_cam on the oracle
def test_unseen_camera_rows_are_exactly_zero_on_the_oracle():
    """A free camera nothing observes has only its rotation prior: the three translation rows and columns of its
    block of H_pp and the three entries of b are exactly zero, the damped step leaves them exactly 0.0 at both
    lambdas, and after optimize(10) its t is bit for bit the input while its q moved."""
    w, r = X.window("ext_unseen_cam"), X.ref_linearize("ext_unseen_cam")
    rows = X.ext_rows(w)[:3]
    assert np.all(r["H"][rows, :] == 0.0) and np.all(r["H"][:, rows] == 0.0) and np.all(r["b"][rows] == 0.0)
    assert np.all(np.diag(r["H"])[X.ext_rows(w)[3:6]] > 0.0)
    for lam in X.LAMBDAS:
        ok, dx = r["steps"][lam]
        assert ok and np.all(dx[rows] == 0.0) and not np.any(np.signbit(dx[rows]))
        assert np.all(dx[X.ext_rows(w)[3:6]] != 0.0)
    cams = X.ref_optimize("ext_unseen_cam")["cams"]
    assert cams["t"][0].tobytes() == w.cams["t"][0].tobytes()
    assert not np.array_equal(cams["q"][0], w.cams["q"][0])


# ------------------------------------------------------------------ the helpers
def test_unshuffle_system_keeps_the_extrinsic_rows_in_camera_order():
    """The oracle's system on the shuffle, mapped back, is its system on the window up to the order of the sums;
    without the tail argument wm.unshuffle_system is what it was."""
    for name in ("ext_base", "ext_fixed_scattered", "ext_calib_only"):
        r, sh = X.ref_linearize(name), X.ref_shuffle(name)
        d = [X.rel(a, b) for a, b in zip(sh["sys"], (r["H"], r["b"], r["Hll"]))]
        print(f"ext_cases: {name}: oracle system vs its shuffle (H, b, Hll) " + " ".join(f"{v:.2e}" for v in d))
        assert max(d) <= 1e-11
        e = X.ext_rows(X.window(name))
        assert len(e) == 18 and X.rel(sh["sys"][0][np.ix_(e, e)], r["H"][np.ix_(e, e)]) <= 1e-11
    w = wm.base()
    w2, pr = wm.shuffled(w, seed=59)
    o, o2 = orc.Oracle(w), orc.Oracle(w2)
    o.errors(), o2.errors()
    H, b, Hll = o.build_system()
    back = wm.unshuffle_system(*o2.build_system(), w, w2, pr)
    assert back[0].shape == H.shape and max(X.rel(x, y) for x, y in zip(back, (H, b, Hll))) <= 1e-11


@pytest.mark.parametrize("name", ["ext_base", "ext_big_step", "ext_one_cam"])
def test_oplus_cams_is_the_oracles_update(name):
    """oplus_cams (long double) against the oracle's apply_step of the same step, in units of u, by
    scaled.state_deviation's rule for t and sign-aligned for q; fixed cameras bit for bit."""
    w = X.window(name)
    ok, dx = X.ref_linearize(name)["steps"][1.0]
    o = orc.Oracle(w)
    o.apply_step(dx)
    c = o.cams()
    q, t = X.oplus_cams(w, dx)
    free = X.free_cams(w)
    dev = X.cam_deviation(c["q"], c["t"], q, t)
    print(f"ext_cases: {name}: oracle apply_step vs long-double oplus_cams, in u: q {dev['q']:.2f} t {dev['t']:.2f}")
    assert dev["q"] <= 8 and dev["t"] <= 64     # (the oracle's c1 cancels: u |upsilon| / theta, scaled.oplus_ref)
    fixed = np.setdiff1d(np.arange(len(w.cams)), free)
    assert np.array_equal(t[fixed], w.cams["t"][fixed]) and np.array_equal(c["t"][fixed], w.cams["t"][fixed])
    assert np.all(np.abs(t[free] - w.cams["t"][free]).max(axis=1) > 0)


# ------------------------------------------------------------------ the solve layout's plan with the extrinsic tail
@pytest.mark.parametrize("NP,NPk", [(1, 0), (2, 0), (4, 3), (8, 6), (5, 3), (64, 63), (65, 64)])
def test_plan_orders_the_extrinsic_panels_last(plan_harness, NP, NPk):
    """lba_plan::make_plan as solve_layout calls it with free extrinsics: NPk = 12 * n_pb_kf / 32 keyframe panels in a
    band, then the panels holding extrinsic rows, coupled with every panel.  NPk = 0 is ext_calib_only and ext_one_free
    (no whole keyframe panel), (4, 3) and (8, 6) the aligned cases, (5, 3) ext_base (the tail starts inside panel 3),
    (64, 63) and (65, 64) the boundary windows."""
    import test_plan
    pairs = [(P, Q) for P in range(NPk) for Q in range(max(0, P - 2), P)]
    pairs += [(P, Q) for P in range(NPk, NP) for Q in range(P)]
    pl = test_plan.plan(plan_harness, NP, pairs, NPk=NPk)
    test_plan.check_plan(NP, pairs, pl, NPk=NPk)
