"""Windows of irregular structure for the parity tests: pure functions Window -> Window.

amc_lba.synth.make_window draws one shape of graph: the fixed keyframes first, every GP observation
between array neighbours (kf_a == kf_b - 1), every landmark seen at least twice, every keyframe observed,
observations sorted by landmark, no two cameras at one time stamp, and no LBA_STEREO_GP edge.  LocalGPBA's
windows are less regular (src/Optimizer.cc:713-1208: the fixed covisible keyframes sit anywhere in the
list, mPrevKF need not be the array neighbour), and the C ABI (include/amc_lba.h) takes any such graph.
Each function below bends one of those regularities and leaves everything else as it was; none of them
changes its argument (dataclasses.replace on copies of the arrays).

CASES maps a name to a builder of the mutated window; tests/test_gpu_window_structure.py runs every case
on the CPU (properties, host set-up, the oracle against itself under `shuffled`) and on the GPU against
the oracle.
"""
from dataclasses import replace

import numpy as np

import orc
from amc_lba.abi import MONO, MONO_GP, STEREO_GP
from amc_lba.synth import make_window

BASE_KW = dict(n_opt_kf=10, n_fixed=1, n_lm=300, obs_per_lm=6, n_cam=4, gp=True, seed=41)
IMG_W, IMG_H = 960.0, 600.0


def base():
    """11 keyframes, 1703 observations, a pose system of 120."""
    return make_window(**BASE_KW)


def is_gp(obs):
    return (obs["kind"] == MONO_GP) | (obs["kind"] == STEREO_GP)


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------ fixed keyframes anywhere
def fixed_scattered(win, extra=(4, 5, 10)):
    """The keyframes `extra` fixed as well: fixed vertices in the middle and at the end of the array, GP
    observations with (a free, b fixed), (a fixed, b free) and both fixed, a motion prior between two fixed
    keyframes (inactive) and velocity edges listed on fixed keyframes (inactive)."""
    kfs = win.kfs.copy()
    kfs["fixed"][list(extra)] = 1
    return replace(win, kfs=kfs, name=(win.name or "window") + "_fixed_scattered")


def one_free(win, keep=5):
    """Every keyframe fixed except `keep`: a pose system of one block."""
    kfs = win.kfs.copy()
    kfs["fixed"] = 1
    kfs["fixed"][keep] = 0
    return replace(win, kfs=kfs, name=(win.name or "window") + "_one_free")


def fixed_only_landmarks(win, lms=tuple(range(12)), seed=43):
    """The landmarks `lms` keep exactly two LBA_MONO observations, both on fixed keyframes, through the
    reference camera: landmarks with no free pose vertex (no H_pl block; still in H_ll, b_l and chi2, and LM
    moves them).  Of the fixed keyframes the two are the ones that see the landmark best (inside the image
    before merely in front of the camera before the rest), the second as far from the first as it can be;
    the measurements are the oracle's projection at the window's estimate plus one pixel of noise, like
    test_heavy_landmarks._consistent.  `win` must have at least two fixed keyframes (fixed_scattered)."""
    rng = np.random.default_rng(seed)
    fixed = np.nonzero(win.kfs["fixed"] != 0)[0]
    assert len(fixed) >= 2
    lms = np.asarray(lms)
    ref = len(win.cams) - 1
    cand = np.zeros(len(lms) * len(fixed), win.obs.dtype)
    cand["kind"] = MONO
    cand["kf_a"] = -1
    cand["kf_b"] = np.tile(fixed, len(lms))
    cand["lm"] = np.repeat(lms, len(fixed))
    cand["cam"] = ref
    cand["t"] = win.kfs["time"][cand["kf_b"]]
    cand["w"] = 1.0
    kept = win.obs[~np.isin(win.obs["lm"], lms)]
    o = orc.Oracle(replace(win, obs=np.concatenate([kept, cand])))
    _, res, _ = o.errors()
    proj = -res[len(kept):, :2]                       # e = z - proj at z = 0
    front = o.depth_ok()[len(kept):].astype(bool)
    inside = front & (proj[:, 0] >= 0) & (proj[:, 0] < IMG_W) & (proj[:, 1] >= 0) & (proj[:, 1] < IMG_H)
    score = np.where(inside, 0, np.where(front, 1, 2)).reshape(len(lms), len(fixed))
    rows = []
    for j in range(len(lms)):
        first = int(np.argmin(score[j]))              # (the first of the best class)
        rest = [k for k in range(len(fixed)) if k != first]
        best = min(score[j][k] for k in rest)
        second = max((k for k in rest if score[j][k] == best), key=lambda k: abs(int(fixed[k]) - int(fixed[first])))
        for k in sorted((first, second)):
            r = cand[j * len(fixed) + k: j * len(fixed) + k + 1].copy()
            r["z"][0, :2] = _f32(proj[j * len(fixed) + k] + rng.normal(0, 1.0, 2))
            rows.append(r)
    obs = np.concatenate([kept] + rows)
    obs = obs[np.argsort(obs["lm"], kind="stable")]
    return replace(win, obs=obs, name=(win.name or "window") + "_fixed_only_lm")


# ------------------------------------------------------------------ thin and missing vertices
def single_obs(win, lms=tuple(range(20, 32))):
    """The landmarks `lms` keep their first observation only (rank-2 H_ll)."""
    o = win.obs
    drop = np.zeros(len(o), bool)
    for l in lms:
        idx = np.nonzero(o["lm"] == l)[0]
        drop[idx[1:]] = True
    return replace(win, obs=o[~drop].copy(), name=(win.name or "window") + "_single_obs")


def unobserved(win, lms=(0, 7, 150, 299), kf=5):
    """The landmarks `lms` lose every observation, and keyframe `kf` loses every edge (observations that
    have it as kf_b or as a GP kf_a, motion priors, its velocity edge): inactive vertices.  They stay in the
    caller's arrays; the outputs are compressed to the active ones."""
    o = win.obs
    drop = np.isin(o["lm"], lms) | (o["kf_b"] == kf) | (is_gp(o) & (o["kf_a"] == kf))
    pri = win.priors[(win.priors["kf_a"] != kf) & (win.priors["kf_b"] != kf)].copy()
    vel = np.ascontiguousarray(win.vel_kfs[win.vel_kfs != kf])
    return replace(win, obs=o[~drop].copy(), priors=pri, vel_kfs=vel, name=(win.name or "window") + "_unobserved")


# ------------------------------------------------------------------ array order
def shuffled(win, seed=47):
    """The same problem with every array in another order: seeded permutations of the observations, the
    landmarks, the keyframes (all references remapped), the priors and vel_kfs.  Returns (window, perms);
    perms["kf"][i] is the original index of the new keyframe i, likewise "lm", "obs", "priors", "vel"."""
    rng = np.random.default_rng(seed)
    pk, pl, po = rng.permutation(len(win.kfs)), rng.permutation(len(win.lm)), rng.permutation(len(win.obs))
    pp, pv = rng.permutation(len(win.priors)), rng.permutation(len(win.vel_kfs))
    new_kf = np.empty(len(pk), np.int64)
    new_kf[pk] = np.arange(len(pk))
    new_lm = np.empty(len(pl), np.int64)
    new_lm[pl] = np.arange(len(pl))
    obs = win.obs[po].copy()
    obs["kf_b"] = new_kf[obs["kf_b"]]
    gp = is_gp(obs)
    obs["kf_a"][gp] = new_kf[obs["kf_a"][gp]]
    obs["lm"] = new_lm[obs["lm"]]
    pri = win.priors[pp].copy()
    pri["kf_a"], pri["kf_b"] = new_kf[pri["kf_a"]], new_kf[pri["kf_b"]]
    vel = np.ascontiguousarray(new_kf[win.vel_kfs[pv]], dtype=np.int32)
    w = replace(win, kfs=win.kfs[pk].copy(), lm=np.ascontiguousarray(win.lm[pl]), obs=obs, priors=pri, vel_kfs=vel,
                truth_lm=None if win.truth_lm is None else win.truth_lm[pl],
                name=(win.name or "window") + "_shuffled")
    return w, {"kf": pk, "lm": pl, "obs": po, "priors": pp, "vel": pv}


def unshuffle_state(kfs, lm, perms):
    """A state of the shuffled window in the original order."""
    k0 = np.empty_like(kfs)
    k0[perms["kf"]] = kfs
    l0 = np.empty_like(lm)
    l0[perms["lm"]] = lm
    return k0, l0


def active_vertices(win):
    """(keyframes, landmarks) with rows in H / b, in array order: the non-fixed keyframes an observation, a
    motion prior that is not all-fixed or a velocity edge touches, and the landmarks with an observation
    (SparseOptimizer::initializeOptimization, sparse_optimizer.cpp:197-267)."""
    o = win.obs
    fixed = win.kfs["fixed"] != 0
    act = np.zeros(len(win.kfs), bool)
    act[o["kf_b"]] = True
    act[o["kf_a"][is_gp(o)]] = True
    for a, b in zip(win.priors["kf_a"], win.priors["kf_b"]):
        if not (fixed[a] and fixed[b]):
            act[a] = act[b] = True
    act[win.vel_kfs] = True
    return np.nonzero(act & ~fixed)[0], np.unique(o["lm"])


def unshuffle_system(H, b, Hll, win, win_s, perms, n_tail=0):
    """(H_pp, b, H_ll) of the shuffled window win_s in the vertex order of the original window `win`.  The last
    n_tail pose rows (the free extrinsics' 6 each, in camera order: `shuffled` leaves the cameras alone) stay where
    they are, behind the keyframe blocks."""
    kf0, lm0 = active_vertices(win)
    kfs, lms = active_vertices(win_s)
    pos_k = {int(perms["kf"][k]): i for i, k in enumerate(kfs)}     # original keyframe -> block in the shuffle
    pos_l = {int(perms["lm"][l]): i for i, l in enumerate(lms)}
    ip = np.concatenate([12 * pos_k[int(k)] + np.arange(12) for k in kf0] + [12 * len(kfs) + np.arange(n_tail)])
    ip = ip.astype(np.int64)
    il = np.concatenate([3 * pos_l[int(l)] + np.arange(3) for l in lm0]) if len(lm0) else np.zeros(0, np.int64)
    np_ = 12 * len(kfs) + n_tail
    assert H.shape == (np_, np_) and b.shape == (np_ + 3 * len(lms),)
    Hll0 = np.empty_like(Hll)
    Hll0[perms["lm"]] = Hll
    return H[np.ix_(ip, ip)], np.concatenate([b[ip], b[np_ + il]]), Hll0


# ------------------------------------------------------------------ edge kinds, pairs and times
def stereo_gp(win, frac=0.5, seed=53):
    """About `frac` of the LBA_MONO_GP observations become LBA_STEREO_GP (EdgeStereoGP): z[2] is the oracle's
    projected u_r at the window's estimate plus N(0, 1), rounded to float32 like every stored measurement."""
    rng = np.random.default_rng(seed)
    obs = win.obs.copy()
    sel = (obs["kind"] == MONO_GP) & (rng.random(len(obs)) < frac)
    obs["kind"][sel] = STEREO_GP
    obs["z"][sel, 2] = 0.0
    _, res, _ = orc.Oracle(replace(win, obs=obs)).errors()
    obs["z"][sel, 2] = _f32(-res[sel, 2] + rng.normal(0, 1.0, int(sel.sum())))
    return replace(win, obs=obs, name=(win.name or "window") + "_stereo_gp")


def skip_pairs(win, cam=0, min_b=3):
    """The GP observations of camera `cam` with kf_b >= min_b interpolate from kf_b - 2: a kf_a that is not
    the array neighbour, and two GP pairs ending in the same keyframe."""
    obs = win.obs.copy()
    sel = is_gp(obs) & (obs["cam"] == cam) & (obs["kf_b"] >= min_b)
    obs["kf_a"][sel] = obs["kf_b"][sel] - 2
    return replace(win, obs=obs, name=(win.name or "window") + "_skip_pairs")


def shared_stamp(win, cam=1, like=0):
    """Camera `cam`'s observation times set to camera `like`'s of the same keyframe: one pose sample of a GP
    pair serves two cameras."""
    obs = win.obs.copy()
    gp = is_gp(obs)
    for k in np.unique(obs["kf_b"][gp & (obs["cam"] == like)]):
        t = np.unique(obs["t"][gp & (obs["cam"] == like) & (obs["kf_b"] == k)])
        assert len(t) == 1
        obs["t"][gp & (obs["cam"] == cam) & (obs["kf_b"] == k)] = t[0]
    return replace(win, obs=obs, name=(win.name or "window") + "_shared_stamp")


def endpoint_times(win, cam_b=0, cam_a=1):
    """The GP observations of camera cam_b at t = time[kf_b] and of camera cam_a at t = time[kf_a]: the end
    points of the GP interpolation (tau = dt and tau = 0)."""
    obs = win.obs.copy()
    gp = is_gp(obs)
    sb, sa = gp & (obs["cam"] == cam_b), gp & (obs["cam"] == cam_a)
    obs["t"][sb] = win.kfs["time"][obs["kf_b"][sb]]
    obs["t"][sa] = win.kfs["time"][obs["kf_a"][sa]]
    return replace(win, obs=obs, name=(win.name or "window") + "_endpoint_times")


def many_cams():
    """20 cameras: 19 distinct time stamps per GP pair, more than the 16 inline slots of the set-up's
    sample-key pass hold per sixteenth of the observation array."""
    return make_window(n_opt_kf=10, n_lm=600, obs_per_lm=8, n_cam=20, seed=41)


def _spanning_fixed():
    from test_heavy_landmarks import _spanning
    return fixed_scattered(_spanning())


CASES = {
    "base": base,
    "fixed_scattered": lambda: fixed_scattered(base()),
    "one_free": lambda: one_free(base()),
    "fixed_only_landmarks": lambda: fixed_only_landmarks(fixed_scattered(base())),
    "single_obs": lambda: single_obs(base()),
    "unobserved": lambda: unobserved(base()),
    "shuffled": lambda: shuffled(base())[0],
    "stereo_gp": lambda: stereo_gp(base()),
    "skip_pairs": lambda: skip_pairs(base()),
    "shared_stamp": lambda: shared_stamp(base()),
    "endpoint_times": lambda: endpoint_times(base()),
    "many_cams": many_cams,
    # heavy landmarks (more keyframes than one tile of k_lin_schur holds) across fixed keyframes
    "spanning_fixed": _spanning_fixed,
    "stereo_gp_shuffled": lambda: shuffled(stereo_gp(base()))[0],
}
