"""Tracking problems at the edges of lba_track (k_track, amc-slam_amd/csrc/lba_track.hip) for the parity tests.

amc_lba.track.make_track_frames cuts one shape of problem out of a window: a few hundred observations of
every kind, one sample per asynchronous camera plus the frame's own pose, a start close to the truth from
which Levenberg-Marquardt never rejects a trial, every point in front of every camera, the observations of
a batch back to back in frame order.  Each builder below bends one of those regularities.  A case is a
function returning (cfg, frames, obs, cams): what Tracker(cfg).track(frames, obs, cams) takes, and what
orc.track_pose takes frame by frame.  Every seed is a constant; the starts of `rejected`, and the (keyframe,
seed) pairs in PICK, were searched once on the CPU oracle alone (a case must reject a trial where it says so,
keep its integer outputs and a tenth of the pose tolerances under a 1e-9 disturbance of the measurements and
under reordered rows, and take no LM decision at the rounding floor of chi2: tests/test_track_cases.py holds
all of it) and are not searched again at run time.

CASES maps "<family>[_<variant>]-fix" / "-free" (the previous frame fixed or free) to a builder;
tests/test_track_cases.py checks every case's claim and its conditioning on the CPU,
tests/test_gpu_track_edges.py runs every case on the GPU against the oracle.
"""
import functools

import numpy as np

import orc
from amc_lba.abi import MONO, MONO_GP, OBS_DTYPE, PRIOR_DTYPE, STEREO
from amc_lba.synth import Window, make_window, quat_to_rot
from amc_lba.track import make_track_frames, track_config

BASE_KW = dict(n_opt_kf=6, n_fixed=1, n_lm=400, obs_per_lm=6, n_cam=4, gp=True, seed=11, perturb=False)

# GPU-versus-oracle tolerances of tests/test_gpu_track.py
TOL_T, TOL_Q, TOL_V = 1e-6, 1e-7, 1e-5

# (keyframe, make_track_frames seed[, make_window seed]) per case where the default (3, 5) is not a test input
# (tests/test_track_cases.py, the conditioning tests):
# - six or seven observations with the previous frame free: under the disturbance the pose stays within the
#   GPU tolerances but not within a tenth of them;
# - the rest: an LM round that starts where the last one ended (no flag changed in between: usual in frames of
#   a few observations) or converges in two steps (a small user lambda) arrives at the rounding floor of chi2
#   before three bad iterations end it, and then rounding decides how many iterations it takes.  Of 7
#   observations with the previous frame fixed, 10 of 1920 (window, keyframe, seed) candidates do not.
DEFAULT_PICK = (3, 5)
PICK = {
    "sizes_6-free": (3, 9),
    "sizes_7-free": (3, 8),
    "sizes_7-fix": (1, 21, 16),
    "stereo_only-fix": (3, 7),
    "stereo_only-free": (3, 6),
    "mono_only-fix": (3, 9),
    "controller_lambda-fix": (3, 9),
    "controller_lambda-free": (3, 8),
}

# far starts (make_track_frames seed, sigma_t [m], sigma_r [deg], sigma_v, keyframe) from which the oracle
# rejects LM trials and still converges.  With the previous frame free the starts of REJECTED_FIX diverge
# (n_good 0 or 1); milder ones that reject and converge were found among 50 seeds of frame 4.
REJECTED_FIX = {"a": (4, 0.5, 90.0, 0.5, 3), "b": (3, 2.0, 45.0, 20.0, 3), "c": (5, 10.0, 120.0, 5.0, 3)}
REJECTED_FREE = {"a": (17, 0.5, 45.0, 2.0, 4), "b": (30, 0.2, 30.0, 5.0, 4)}

SIZES = (0, 1, 6, 7, 255, 256, 257)
SENTINEL = 7


def tag(fix_prev):
    return "fix" if fix_prev else "free"


@functools.lru_cache(maxsize=None)
def _window(**over):
    kw = dict(BASE_KW)
    kw.update(over)
    return make_window(**kw)


def window(**over):
    """The base window (6 optimisable keyframes, 400 landmarks, 4 cameras, at the truth) with `over`."""
    return _window(**over)


def pick(name, fix_prev):
    """(keyframe, make_track_frames seed, window keywords) of the case."""
    p = PICK.get(f"{name}-{tag(fix_prev)}", DEFAULT_PICK)
    return p[0], p[1], (dict(seed=p[2]) if len(p) > 2 else {})


def regular(fix_prev, name="regular", win_over=None, **mtf):
    """(win, k, cfg, frames, obs, cams): one frame as make_track_frames draws it."""
    k, seed, over = pick(name, fix_prev)
    over.update(win_over or {})
    win = window(**over)
    frames, obs = make_track_frames(win, [k], fix_prev=fix_prev, seed=seed, **mtf)
    return win, k, track_config(), frames, obs, win.cams.copy()


def take(frames, obs, mask):
    """The frame with the observations `mask` (a boolean mask or an index array) only."""
    obs = obs[mask].copy()
    frames = frames.copy()
    frames["n_obs"][0] = len(obs)
    return frames, obs


# ------------------------------------------------------------------ geometry at the true state
def cam_depth(kf, cam, Xw):
    """Depth of the points Xw in camera record `cam` of the body pose `kf` (isDepthPositive's zc)."""
    Rwb, Rbc = quat_to_rot(np.asarray(kf["q"])), quat_to_rot(np.asarray(cam["q"]))
    Xb = (np.asarray(Xw) - kf["t"]) @ Rwb
    return ((Xb - cam["t"]) @ Rbc)[..., 2]


def obs_depth(kf, cams, obs):
    return np.array([cam_depth(kf, cams[o["cam"]], o["Xw"]) for o in obs])


def true_projection(win, k, obs):
    """(u, v, u_r) of the tracking observations `obs` of keyframe k with both frames at the window's state
    (the truth, perturb=False), through the oracle's own edges: a GP observation is projected from the pose
    interpolated at its time stamp."""
    o = np.zeros(len(obs), OBS_DTYPE)
    gp = obs["kind"] == MONO_GP
    o["kind"] = np.where(gp, MONO_GP, STEREO)      # (all three components of the reference camera's projection)
    o["kf_a"] = np.where(gp, 0, -1)
    o["kf_b"] = 1
    o["lm"] = np.arange(len(obs))
    o["cam"] = obs["cam"]
    o["t"] = obs["t"]
    o["w"] = 1.0
    w2 = Window(kfs=win.kfs[k - 1:k + 1].copy(), lm=np.ascontiguousarray(obs["Xw"]), obs=o,
                priors=np.zeros(0, PRIOR_DTYPE), vel_kfs=np.zeros(0, np.int32), cams=win.cams, cfg=dict(win.cfg))
    _, res, _ = orc.Oracle(w2).errors()
    return -res                                     # e = z - proj at z = 0


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def remeasure(win, k, obs, rows, rng):
    """z of the observations `rows` re-projected at the true state plus the generator's pixel noise
    (N(0, 1.2^octave) with w = 1.2^(-2 octave)), rounded to float like every stored measurement."""
    proj = true_projection(win, k, obs[rows])
    sig = 1.0 / np.sqrt(obs["w"][rows])
    z = proj + rng.normal(0, 1, proj.shape) * sig[:, None]
    z[obs["kind"][rows] != STEREO, 2] = 0.0
    obs["z"][rows] = _f32(z)


# ------------------------------------------------------------------ the families
def case_regular(fix_prev, n_cam):
    """n_cam = 1: the reference camera alone (no GP observation, one sample); 2: one asynchronous camera; 4."""
    over = dict(n_cam=n_cam, gp=n_cam > 1)
    _, _, cfg, frames, obs, cams = regular(fix_prev, f"regular_c{n_cam}", over)
    return cfg, frames, obs, cams


KIND_FILTERS = {
    "gp_only": lambda o: o["kind"] == MONO_GP,        # no own-pose sample
    "ref_only": lambda o: o["kind"] != MONO_GP,       # one sample, the frame's own pose
    "stereo_only": lambda o: o["kind"] == STEREO,
    "mono_only": lambda o: o["kind"] == MONO,
}


def case_kind(fix_prev, family):
    _, _, cfg, frames, obs, cams = regular(fix_prev, family)
    frames, obs = take(frames, obs, KIND_FILTERS[family](obs))
    return cfg, frames, obs, cams


def n_samples(obs):
    """Pose samples of a frame: the distinct time stamps of its GP observations, and its own pose if the
    reference camera observes."""
    gp = obs["kind"] == MONO_GP
    return len(np.unique(obs["t"][gp])) + int((~gp).any())


def case_samples(fix_prev, n_cam):
    """n_cam - 1 asynchronous stamps plus the own pose: 16 samples (TR_MAXS) at n_cam = 16, 17 at 17."""
    _, _, cfg, frames, obs, cams = regular(fix_prev, f"samples{n_cam}", dict(n_cam=n_cam, n_lm=1500))
    assert n_samples(obs) == n_cam
    return cfg, frames, obs, cams


def endpoint_rows(obs, n_cur=6, n_prev=4):
    """The GP observations moved to cur.time (the first n_cur of camera 0) and prev.time (n_prev of camera 1)."""
    c0 = np.nonzero((obs["kind"] == MONO_GP) & (obs["cam"] == 0))[0][:n_cur]
    c1 = np.nonzero((obs["kind"] == MONO_GP) & (obs["cam"] == 1))[0][:n_prev]
    assert len(c0) == n_cur and len(c1) == n_prev
    return c0, c1


def case_endpoint_stamps(fix_prev):
    """A handful of GP observations stamped exactly at cur.time and at prev.time (tau = dt and tau = 0), their
    z re-projected from that keyframe's true pose: a GP sample and the own-pose sample share a stamp."""
    win, k, cfg, frames, obs, cams = regular(fix_prev, "endpoint_stamps")
    rc, rp = endpoint_rows(obs)
    obs["t"][rc] = frames[0]["cur"]["time"]
    obs["t"][rp] = frames[0]["prev"]["time"]
    rows = np.concatenate([rc, rp])
    remeasure(win, k, obs, rows, np.random.default_rng(101))
    obs["outlier"][rows] = 0
    assert (obs_depth(win.kfs[k], cams, obs[rows]) > 1.0).all() and (obs_depth(win.kfs[k - 1], cams, obs[rows]) > 1.0).all()
    assert (obs["kind"] != MONO_GP).any()
    return cfg, frames, obs, cams


def case_sizes(fix_prev, n):
    """The first n observations of a regular frame (the rows are in landmark order: the kinds interleave)."""
    _, _, cfg, frames, obs, cams = regular(fix_prev, f"sizes_{n}")
    assert len(obs) >= n
    frames, obs = take(frames, obs, np.arange(n))
    return cfg, frames, obs, cams


def behind_rows(obs, every=40, first=3):
    """Every 40th observation of each kind (GP, mono, stereo), from that kind's fourth on."""
    return np.sort(np.concatenate([np.nonzero(obs["kind"] == kd)[0][first::every] for kd in (MONO_GP, MONO, STEREO)]))


def case_behind(fix_prev):
    """About 1 in 40 points mirrored through the current frame's position (Xw -> 2 t_cur - Xw), GP, mono and
    stereo alike, and measured where they project from there: small chi2, negative depth, so that isDepthPositive
    alone decides (mono, GP) or nothing does (stereo, which has no depth test)."""
    win, k, cfg, frames, obs, cams = regular(fix_prev, "behind")
    rows = behind_rows(obs)
    obs["Xw"][rows] = _f32(2.0 * win.kfs[k]["t"] - obs["Xw"][rows])
    remeasure(win, k, obs, rows, np.random.default_rng(103))
    obs["outlier"][rows] = 0
    assert len(rows) >= 5 and len(set(obs["kind"][rows])) == 3
    assert (obs_depth(win.kfs[k], cams, obs[rows]) < -1.0).all()
    return cfg, frames, obs, cams


def case_all_outlier(fix_prev):
    """Every observation flagged on entry: the first round runs on the prior alone."""
    _, _, cfg, frames, obs, cams = regular(fix_prev, "all_outlier")
    obs["outlier"] = 1
    return cfg, frames, obs, cams


CONTROLLER = {"nostop": dict(early_stop=0), "lambda": dict(lambda_init=1e-2), "trials1": dict(max_trials=1),
              "trials2": dict(max_trials=2)}


def case_controller(fix_prev, variant):
    _, _, _, frames, obs, cams = regular(fix_prev, f"controller_{variant}")
    return track_config(**CONTROLLER[variant]), frames, obs, cams


def case_rejected(fix_prev, variant, **cfg_over):
    """A far start from which the oracle rejects LM trials (lambda *= ni; ni *= 2)."""
    seed, st, sr, sv, k = (REJECTED_FIX if fix_prev else REJECTED_FREE)[variant]
    win = window()
    frames, obs = make_track_frames(win, [k], fix_prev=fix_prev, seed=seed, sigma_t=st, sigma_r=sr, sigma_v=sv)
    return track_config(**cfg_over), frames, obs, win.cams.copy()


def case_cur_fixed_flag(fix_prev):
    """cur.fixed = 1 on entry: the reference frees the vertex regardless (setFixed(false))."""
    _, _, cfg, frames, obs, cams = regular(fix_prev, "cur_fixed_flag")
    frames["cur"]["fixed"] = 1
    return cfg, frames, obs, cams


def shuffle_perm(n, seed=107):
    return np.random.default_rng(seed).permutation(n)


def case_shuffled_obs(fix_prev, shuffle=True):
    """A regular frame's rows under a fixed permutation (shuffle=False: the same frame as drawn), so kinds and
    time stamps interleave: new row i is old row shuffle_perm(n)[i]."""
    _, _, cfg, frames, obs, cams = regular(fix_prev, "shuffled_obs")
    if shuffle:
        obs = obs[shuffle_perm(len(obs))].copy()
    return cfg, frames, obs, cams


def case_ranges(fix_prev, ks=(2, 3, 4), pads=(3, 5, 2, 4)):
    """Three frames whose observation ranges lie in the array in reverse frame order, with unused rows before,
    between and after them that carry outlier = SENTINEL."""
    win = window()
    seed = pick("ranges", fix_prev)[1]
    frames, obs = make_track_frames(win, list(ks), fix_prev=fix_prev, seed=seed)
    parts, at = [], 0
    for j, f in enumerate(reversed(range(len(ks)))):
        pad = obs[:pads[j]].copy()
        pad["outlier"] = SENTINEL
        parts.append(pad)
        at += len(pad)
        s = slice(frames[f]["obs0"], frames[f]["obs0"] + frames[f]["n_obs"])
        parts.append(obs[s].copy())
        frames[f]["obs0"] = at
        at += frames[f]["n_obs"]
    pad = obs[:pads[-1]].copy()
    pad["outlier"] = SENTINEL
    parts.append(pad)
    return track_config(), frames, np.concatenate(parts), win.cams.copy()


def used_rows(frames, n):
    used = np.zeros(n, bool)
    for F in frames:
        used[F["obs0"]:F["obs0"] + F["n_obs"]] = True
    return used


def _cases():
    c = {}
    for fix in (True, False):
        t = tag(fix)
        for n_cam in (1, 2, 4):
            c[f"regular_c{n_cam}-{t}"] = functools.partial(case_regular, fix, n_cam)
        for fam in KIND_FILTERS:
            c[f"{fam}-{t}"] = functools.partial(case_kind, fix, fam)
        c[f"samples16-{t}"] = functools.partial(case_samples, fix, 16)
        c[f"endpoint_stamps-{t}"] = functools.partial(case_endpoint_stamps, fix)
        for n in SIZES:
            c[f"sizes_{n}-{t}"] = functools.partial(case_sizes, fix, n)
        c[f"behind-{t}"] = functools.partial(case_behind, fix)
        c[f"all_outlier-{t}"] = functools.partial(case_all_outlier, fix)
        for v in CONTROLLER:
            c[f"controller_{v}-{t}"] = functools.partial(case_controller, fix, v)
        for v in (REJECTED_FIX if fix else REJECTED_FREE):
            c[f"rejected_{v}-{t}"] = functools.partial(case_rejected, fix, v)
        c[f"cur_fixed_flag-{t}"] = functools.partial(case_cur_fixed_flag, fix)
        c[f"shuffled_obs-{t}"] = functools.partial(case_shuffled_obs, fix)
        c[f"ranges-{t}"] = functools.partial(case_ranges, fix)
    return c


CASES = _cases()


def frame_slice(F):
    return slice(int(F["obs0"]), int(F["obs0"]) + int(F["n_obs"]))


def run_oracle(cfg, frames, obs, cams):
    """orc.track_pose frame by frame on copies: (frames, obs) as Tracker.track returns them."""
    fr, ob = frames.copy(), obs.copy()
    for f in range(len(fr)):
        a = fr[f:f + 1].copy()
        s = frame_slice(fr[f])
        o = ob[s].copy()
        orc.track_pose(cfg, a, o, cams)
        fr[f] = a[0]
        ob[s] = o
    return fr, ob


def pose_diff(a, b):
    """(translation difference relative to max(1, |t|), sign-aligned quaternion difference, velocity
    difference) of two `cur` records, the quantities TOL_T, TOL_Q and TOL_V bound."""
    dt = np.abs(a["t"] - b["t"]).max() / max(1.0, np.abs(b["t"]).max())
    qa, qb = a["q"] * np.sign(a["q"][3]), b["q"] * np.sign(b["q"][3])
    return float(dt), float(np.abs(qa - qb).max()), float(np.abs(a["vel"] - b["vel"]).max())


DISTURB_SEEDS = (201, 202, 203)
REORDER_SEEDS = (211, 212, 213, 214, 215, 216)


def _same_integers(fr, ob, fr0, ob0):
    return bool((ob["outlier"] == ob0["outlier"]).all() and (fr["n_good"] == fr0["n_good"]).all()
                and (fr["iterations"] == fr0["iterations"]).all())


def stability(cfg, frames, obs, cams, rel=1e-9):
    """The oracle on the case as it is, and again
    - with every z multiplied by 1 + rel N(0, 1), under each of DISTURB_SEEDS;
    - with the rows of every frame in another order (the measurements untouched: only the order of the
      oracle's sums over the edges changes, which is how the device differs from it), under each of
      REORDER_SEEDS.
    Returns (whether every run reproduced the outlier flags, n_good and iterations; the largest pose_diff to
    the first run over frames and runs; the LM iterations of all these runs whose accept / reject decision lay
    within rounding of the chi2 sum and changes the iteration count, orc.track_floor_iterations)."""
    orc.track_floor_iterations(reset=True)
    fr0, ob0 = run_oracle(cfg, frames, obs, cams)
    same, worst = True, np.zeros(3)
    runs = []
    for seed in DISTURB_SEEDS:
        o = obs.copy()
        o["z"] *= 1.0 + rel * np.random.default_rng(seed).normal(0, 1, o["z"].shape)
        runs.append(run_oracle(cfg, frames, o, cams))
    for seed in REORDER_SEEDS:
        rng = np.random.default_rng(seed)
        src = np.arange(len(obs))
        for F in frames:
            s = frame_slice(F)
            src[s] = src[s][rng.permutation(int(F["n_obs"]))]
        fr, ob = run_oracle(cfg, frames, obs[src], cams)
        back = np.empty_like(ob)
        back[src] = ob
        runs.append((fr, back))
    for fr, ob in runs:
        same = same and _same_integers(fr, ob, fr0, ob0)
        for f in range(len(fr)):
            worst = np.maximum(worst, pose_diff(fr[f]["cur"], fr0[f]["cur"]))
    return same, tuple(float(v) for v in worst), orc.track_floor_iterations(reset=True)


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, frames, obs, cams) of CASES[name], built once; the arrays are read-only, a test passes copies on."""
    cfg, frames, obs, cams = CASES[name]()
    for a in (frames, obs, cams):
        a.setflags(write=False)
    return cfg, frames, obs, cams


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's (frames, obs) of case(name), computed once and shared by the tests; read-only."""
    fr, ob = run_oracle(*case(name))
    fr.setflags(write=False)
    ob.setflags(write=False)
    return fr, ob
