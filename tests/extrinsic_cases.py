"""Windows with free extrinsics (lba_cam.ext_free, LocalGPBA's bExtrinsic pass) at the structural edges of the
windowed LM path: plain numpy, no GPU.

Every case composes tests/window_mutations.py, amc_lba.synth.with_free_extrinsics and test_heavy_landmarks._spanning;
no generator code is restated here.  A free extrinsic has its own branch in the set-up (keyframe slots n_kf + e, the
sample key (time, camera slot), side-2 pairs), the sweep (side == 2), the sample expansion (36 columns), the edge
items (EdgeExtrinsicPrior), the solve layout (the panels with extrinsic rows last, as a dense tail), the update (the
trial camera record in the other buffer) and the evaluation; CASES bends the window under each of them:

  fixed keyframes anywhere, all but one, or all of them (no keyframe block at all: a pose system of the extrinsics
  alone); a GP sample whose only free vertex is the extrinsic; partly free and non-contiguous camera sets; a free
  camera nothing observes (its three translation rows structurally zero); inactive vertices; arbitrary array order;
  two GP pairs per keyframe; end-point and shared time stamps (two free cameras, and a free with a fixed one, at one
  time on one pair); LBA_STEREO_GP on the fixed cameras beside LBA_MONO_GP on the free one; heavy landmarks; more
  cameras than the sweep stages in LDS and more sample keys than the set-up's inline table; rejected trials; a
  non-diagonal prior information with a non-zero prior residual; an extrinsic tail that starts on a 32-row panel edge.

tests/test_extrinsic_cases.py shows on the CPU that every case has its property and is conditioned well enough;
tests/test_gpu_extrinsic_structure.py runs them on the device against the oracle.
"""
import functools
from dataclasses import replace

import numpy as np

import window_mutations as wm
from amc_lba.abi import MONO_GP, STEREO_GP
from amc_lba.synth import make_window, with_free_extrinsics


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def ext_base():
    return with_free_extrinsics(wm.base())


def _calib_only():
    w = ext_base()
    kfs = w.kfs.copy()
    kfs["fixed"] = 1
    return replace(w, kfs=kfs, name=w.name + "_calib_only")


def _unseen_cam(cam=0):
    w = ext_base()
    return replace(w, obs=w.obs[w.obs["cam"] != cam].copy(), name=w.name + "_unseen_cam")


def _stereo_gp_mixed(cam=1):
    w = with_free_extrinsics(wm.stereo_gp(wm.base()), cams=[cam])
    obs = w.obs.copy()
    sel = (obs["kind"] == STEREO_GP) & (obs["cam"] == cam)
    obs["kind"][sel] = MONO_GP
    obs["z"][sel, 2] = 0.0
    return replace(w, obs=obs, name=w.name + "_mixed")


def _heavy():
    from test_heavy_landmarks import _spanning
    return with_free_extrinsics(_spanning(n_opt_kf=11, n_lm=300, n_long=2, seed=9, cams=(0, 1, 2, 3), repeat=16))


INFO = np.array([[.3, .1, -.05], [.1, .2, .04], [-.05, .04, .25]])


def _full_info():
    w = ext_base()
    cams = w.cams.copy()
    for i in np.nonzero(cams["ext_free"])[0]:
        cams["rbc_info"][i] = ((i + 1) * INFO).ravel()
        q = cams["rbc_ini"][i].copy()
        q[:3] += 0.01 * (i + 1)
        cams["rbc_ini"][i] = _f32(q / np.linalg.norm(q))
    return replace(w, cams=cams, name=w.name + "_full_info")


def _aligned(n_opt_kf, seed):
    return with_free_extrinsics(make_window(n_opt_kf=n_opt_kf, n_fixed=1, n_lm=320, obs_per_lm=6, n_cam=4, gp=True,
                                            seed=seed))


CASES = {
    "ext_base": ext_base,
    "ext_fixed_scattered": lambda: with_free_extrinsics(wm.fixed_scattered(wm.base())),
    "ext_fixed_only_landmarks": lambda: with_free_extrinsics(wm.fixed_only_landmarks(wm.fixed_scattered(wm.base()))),
    "ext_calib_only": _calib_only,
    "ext_one_free": lambda: with_free_extrinsics(wm.one_free(wm.base())),
    "ext_one_cam": lambda: with_free_extrinsics(wm.base(), cams=[1]),
    "ext_two_cams": lambda: with_free_extrinsics(wm.base(), cams=[0, 2]),
    "ext_unseen_cam": _unseen_cam,
    "ext_unobserved": lambda: with_free_extrinsics(wm.unobserved(wm.base())),
    "ext_shuffled": lambda: wm.shuffled(ext_base())[0],
    "ext_skip_pairs": lambda: with_free_extrinsics(wm.skip_pairs(wm.base())),
    "ext_endpoint_times": lambda: with_free_extrinsics(wm.endpoint_times(wm.base())),
    "ext_shared_stamp": lambda: with_free_extrinsics(wm.shared_stamp(wm.base())),
    "ext_shared_stamp_one": lambda: with_free_extrinsics(wm.shared_stamp(wm.base()), cams=[1]),
    "ext_stereo_gp_mixed": _stereo_gp_mixed,
    "ext_heavy": _heavy,
    "ext_cams_9": lambda: with_free_extrinsics(make_window(n_opt_kf=6, n_lm=300, obs_per_lm=6, n_cam=9, gp=True,
                                                           seed=84)),
    "ext_cams_20": lambda: with_free_extrinsics(wm.many_cams()),
    "ext_big_step": lambda: with_free_extrinsics(wm.base(), rot_deg=10, trans=0.05),
    "ext_full_info": _full_info,
    "ext_aligned_8": lambda: _aligned(8, 68),
    "ext_aligned_16": lambda: _aligned(16, 76),
}

# pose dimension, (iterations, trials) of the oracle's optimize(10)
TABLE = {
    "ext_base": (138, (10, 17)), "ext_fixed_scattered": (102, (10, 15)), "ext_fixed_only_landmarks": (102, (10, 15)),
    "ext_calib_only": (18, (10, 12)), "ext_one_free": (30, (10, 14)), "ext_one_cam": (126, (10, 10)),
    "ext_two_cams": (132, (10, 16)), "ext_unseen_cam": (138, (10, 17)), "ext_unobserved": (126, (10, 15)),
    "ext_shuffled": (138, (10, 17)), "ext_skip_pairs": (138, (10, 16)), "ext_endpoint_times": (138, (10, 16)),
    "ext_shared_stamp": (138, (10, 15)), "ext_shared_stamp_one": (126, (10, 10)),
    "ext_stereo_gp_mixed": (126, (10, 10)), "ext_heavy": (150, (6, 10)), "ext_cams_9": (120, (8, 14)),
    "ext_cams_20": (234, (5, 5)), "ext_big_step": (138, (9, 16)), "ext_full_info": (138, (10, 17)),
    "ext_aligned_8": (114, (5, 5)), "ext_aligned_16": (210, (5, 5)),
}


def boundary_window(n):
    """The windows either side of the 64 / 65-panel switch of the reduced system's solve, with the three extrinsic
    blocks as the dense tail (n = 167, 168: pose dimensions 2022 and 2034)."""
    return with_free_extrinsics(make_window(n_opt_kf=n, n_fixed=1, n_lm=2500, obs_per_lm=5, n_cam=4, gp=True,
                                            global_ba=True, seed=50 + n))


# ------------------------------------------------------------------ the pose system's layout with extrinsics
def free_cams(win):
    return np.nonzero(win.cams["ext_free"] != 0)[0]


def active_vertices(win):
    """(keyframes, landmarks, cameras) with rows in H / b: wm.active_vertices' keyframe blocks (12 rows each), then
    the free cameras' 6 rows each in camera order (a free extrinsic is active through its prior edge, observed or
    not), then the landmarks."""
    kf, lm = wm.active_vertices(win)
    return kf, lm, free_cams(win)


def pose_dim(win):
    kf, _, cams = active_vertices(win)
    return 12 * len(kf) + 6 * len(cams)


def ext_rows(win):
    """The extrinsic rows of the pose system."""
    kf, _, cams = active_vertices(win)
    return 12 * len(kf) + np.arange(6 * len(cams))


def unshuffle_system(H, b, Hll, win, win_s, perms):
    """wm.unshuffle_system for a window with free extrinsics: the keyframe blocks and the landmarks permuted back,
    the 6 * n_free extrinsic rows left in camera order (wm.shuffled does not shuffle the cameras)."""
    assert np.array_equal(win.cams, win_s.cams)
    return wm.unshuffle_system(H, b, Hll, win, win_s, perms, n_tail=6 * len(free_cams(win)))


def oplus_cams(win, dx):
    """Tbc <- Tbc exp(d) (VertexExtrinsic::oplusImpl) of the extrinsic rows of a step dx in np.longdouble, rounded
    to float64: (q [x y z w], t) of every camera, the fixed ones as they are (q normalised).  The construction of
    scaled.oplus_ref: d = [upsilon, omega], V = I + c1 W + c2 W^2 with c1 = 2 sin^2(theta / 2) / theta^2 and the
    series of c1, c2 and sin(theta / 2) / theta below theta = 1e-2, the quaternion normalised on load and after the
    product."""
    ld = np.longdouble
    rows = ext_rows(win)
    free = free_cams(win)
    q = win.cams["q"].astype(ld)
    q /= np.sqrt((q * q).sum(1))[:, None]
    t = win.cams["t"].astype(ld)
    d = np.asarray(dx, ld)[rows].reshape(-1, 6)
    ups, w = d[:, 0:3], d[:, 3:6]
    th2 = (w * w).sum(1)
    th = np.sqrt(th2)
    small = th < ld(1e-2)
    ths = np.where(small, ld(1), th)
    c1 = np.where(small, ld(1) / 2 - th2 / 24 + th2 * th2 / 720 - th2 ** 3 / 40320, 2 * np.sin(ths / 2) ** 2 / ths ** 2)
    c2 = np.where(small, ld(1) / 6 - th2 / 120 + th2 * th2 / 5040 - th2 ** 3 / 362880, (ths - np.sin(ths)) / ths ** 3)
    wu = np.cross(w, ups)
    dt = ups + c1[:, None] * wu + c2[:, None] * np.cross(w, wu)
    im = np.where(small, ld(1) / 2 - th2 / 48 + th2 * th2 / 3840 - th2 ** 3 / 645120, np.sin(ths / 2) / ths)
    dq = np.concatenate([im[:, None] * w, np.cos(th / 2)[:, None]], axis=1)
    qf = q[free]
    v, s = qf[:, :3], qf[:, 3:4]
    uv = 2 * np.cross(v, dt)
    t[free] += dt + s * uv + np.cross(v, uv)
    dv, ds = dq[:, :3], dq[:, 3:4]
    qn = np.concatenate([s * dv + ds * v + np.cross(v, dv), s * ds - (v * dv).sum(1)[:, None]], axis=1)
    q[free] = qn / np.sqrt((qn * qn).sum(1))[:, None]
    return q.astype(float), t.astype(float)


# ------------------------------------------------------------------ windows and oracle references, once per case
LAMBDAS = (1.0, 1e-3)
U = float(np.finfo(np.float64).eps) / 2   # unit roundoff of fp64 (scaled.U)
SHUFFLE_SEED = 59


@functools.lru_cache(maxsize=None)
def window(name):
    """The case's window, built once; no test changes it."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def ref_linearize(name):
    """The oracle's errors, system and damped steps on the case (read-only)."""
    import orc
    o = orc.Oracle(window(name))
    chi, res, c2 = o.errors()
    H, b, Hll = o.build_system()
    steps = {lam: o.solve(lam) for lam in LAMBDAS}
    return dict(chi=chi, res=res, c2=c2, H=H, b=b, Hll=Hll, ok=o.depth_ok(), steps=steps, np=o.pose_dim)


def _optimized(win, iters=10, **cfg):
    import orc
    o = orc.Oracle(win, **cfg)
    n, st = o.optimize(iters)
    kf, lm = o.state()
    return dict(n=n, st=st, kf=kf, lm=lm, cams=o.cams(), c2=o.last_obs_chi2(), ok=o.depth_ok())


@functools.lru_cache(maxsize=None)
def ref_optimize(name):
    """The oracle's optimize(10) on the case (read-only)."""
    return _optimized(window(name))


@functools.lru_cache(maxsize=None)
def ref_shuffle(name):
    """The oracle on wm.shuffled(window, seed=59), everything mapped back to the window's order: its system
    (H_pp, b, H_ll) and its optimize(10) (n, st, kf, lm, cams)."""
    import orc
    win = window(name)
    ws, pr = wm.shuffled(win, seed=SHUFFLE_SEED)
    o = orc.Oracle(ws)
    o.errors()
    sys_ = unshuffle_system(*o.build_system(), win, ws, pr)
    r = _optimized(ws)
    r["kf"], r["lm"] = wm.unshuffle_state(r["kf"], r["lm"], pr)
    return dict(r, sys=sys_, win=ws, perms=pr)


def rel(a, b):
    """The measure of the max-norm parity tests: max|a - b| / max|b|."""
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def quat_diff(q, q_o):
    """max|q - q_o| of quaternions (n, 4) with w made positive, as the LM parity tests compare them."""
    return float(np.abs(q * np.sign(q[:, 3:4]) - q_o * np.sign(q_o[:, 3:4])).max())


# the LM-run limits of tests/test_gpu_window_structure.py and tests/test_extrinsic.py, per output
STATE_LIMITS = {"kf_t": 1e-6, "lm": 1e-6, "kf_vel": 1e-5, "kf_q": 1e-7, "cam_q": 1e-7, "cam_t": 1e-6}


def state_figures(kf, lm, cams, kf_o, lm_o, cams_o):
    """The deviation of an LM result from a reference one in the measure of each output's limit (STATE_LIMITS):
    max-norm relative for t, velocity, landmarks and the cameras' t, absolute for the quaternions."""
    return {"kf_t": rel(kf["t"], kf_o["t"]), "lm": rel(lm, lm_o), "kf_vel": rel(kf["vel"], kf_o["vel"]),
            "kf_q": quat_diff(kf["q"], kf_o["q"]), "cam_q": quat_diff(cams["q"], cams_o["q"]),
            "cam_t": rel(cams["t"], cams_o["t"])}


def cam_deviation(q, t, q_o, t_o):
    """Deviation of camera extrinsics from reference ones in units of u, by scaled.state_deviation's rule:
    |a - b| / (|b| + max|b|) per entry of t, |a - b| of the sign-aligned quaternions."""
    sgn = np.sign(np.sum(q * q_o, axis=1, keepdims=True))
    return {"q": float(np.abs(q * sgn - q_o).max() / U),
            "t": float((np.abs(t - t_o) / np.maximum(np.abs(t_o) + np.abs(t_o).max(), 1e-300)).max() / U)}
