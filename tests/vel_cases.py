"""MCRansac inputs at the edges of lba_track_vel_ransac (k_vel_hyp / k_vel_select, amc-slam_amd/csrc/lba_track_vel.hip)
for the parity tests: tests/test_vel_cases.py shows on the CPU that each case has the property it is named for and
keeps the settled cap of tests/vel_oracle.py, tests/test_gpu_vel_ransac.py compares the GPU with the oracle on them.

Every case is one frame of at most 200 observations and 23 hypotheses from amc_lba.track.make_vel_frames
(4 cameras, 0.7 px noise, 10 % gross outliers unless the case says otherwise).  `case(name)` returns
(frames, obs, samples, cams, params) with params an LbaVelParams or None; `reference(name)` the oracle's result
per frame (vel_oracle.reference), computed once per process.
"""
import functools

import numpy as np

import vel_oracle as vo
from amc_lba.track import make_vel_frames, track_config, vel_params

N_OBS_EDGES = (3, 63, 64, 65, 129)      # the scoring pass's lane edges (64 lanes)
N_HYP_EDGES = (1, 4, 5, 23)
MAX_UNSETTLED = 0.10
TOL = 1e-6                               # the project's LM-run tolerance, relative to max(1, |v|_inf)
HUBER2 = 5.991 ** 2


def _plain(**kw):
    fr, ob, sm, cams, truth = make_vel_frames(**kw)
    return fr, ob, sm, cams, None, truth


def _nobs(n):
    return _plain(n_obs=n, n_hyp=2 if n == 3 else 6, outlier_frac=0.0 if n == 3 else 0.1, seed=100 + n)


def _nhyp(n):
    return _plain(n_obs=100, n_hyp=n, seed=200 + n)


def _dup_tie():
    fr, ob, sm, cams, _, truth = _plain(n_obs=120, n_hyp=6, seed=31)
    sm = np.concatenate([sm, sm[:, ::-1]])          # every triple again, in another order: ties for best
    fr["n_hyp"] = 12
    return fr, ob, sm, cams, None, truth


def _one_cam_triples():
    fr, ob, sm, cams, _, truth = _plain(n_obs=160, n_hyp=8, seed=32)
    rng = np.random.default_rng(320)
    rows = np.nonzero(ob["cam"] == 1)[0]
    sm[:] = [rng.choice(rows, 3, replace=False) for _ in range(len(sm))]
    return fr, ob, sm, cams, None, truth


def _one_dt():
    return _plain(n_obs=120, n_hyp=8, dts=0.1, seed=33)


def _zero_start():
    fr, ob, sm, cams, _, truth = _plain(n_obs=120, n_hyp=8, seed=34)
    fr["vel"] = 0.0
    return fr, ob, sm, cams, None, truth


def _sampled_outlier():
    fr, ob, sm, cams, _, truth = _plain(n_obs=120, n_hyp=8, n_octaves=2, seed=35)
    gross = np.nonzero(truth["gross"])[0]
    sm[:, 0] = gross[np.arange(len(sm)) % len(gross)]
    for h in range(len(sm)):                          # (keep the triples' indices distinct)
        while len(set(sm[h])) < 3:
            sm[h, 1:] = (sm[h, 1:] + 1) % len(ob)
    return fr, ob, sm, cams, None, truth


def _dt0_cam():
    fr, ob, sm, cams, _, truth = _plain(n_obs=160, n_hyp=10, dts=[0.0, 0.09, 0.1, 0.11], seed=36)
    rng = np.random.default_rng(360)
    rows = np.nonzero(ob["cam"] == 0)[0]
    sm[:3] = [rng.choice(rows, 3, replace=False) for _ in range(3)]     # H = 0: the velocity stays the start
    sm[3] = [rows[0], np.nonzero(ob["cam"] == 1)[0][0], np.nonzero(ob["cam"] == 2)[0][0]]   # and mixed with the others
    return fr, ob, sm, cams, None, truth


BEHIND = 10


def _behind():
    fr, ob, sm, cams, _, truth = _plain(n_obs=120, n_hyp=8, seed=37)
    rig = vo.Rig(cams)
    R, t = vo.quat_rot(fr[0]["q"]), fr[0]["t"]
    for i in range(BEHIND):                           # mirror the point through the camera centre: depth < 0
        c, dt = int(ob["cam"][i]), float(ob["dt"][i])
        Re, te = vo.se3_exp(truth["vel"][0] * dt)
        centre = R @ (Re @ rig.tbc[c] + te) + t
        ob["Xw"][i] = (2 * centre - ob["Xw"][i]).astype(np.float32)
    sm[0] = [0, 50, 90]
    sm[1] = [1, 2, 70]
    return fr, ob, sm, cams, None, truth


def shuffle_perm(n):
    return np.random.default_rng(380).permutation(n)


def _shuffled(shuffle=True):
    fr, ob, sm, cams, _, truth = _plain(n_obs=150, n_hyp=8, seed=38)
    if shuffle:
        perm = shuffle_perm(len(ob))                  # new row i is old row perm[i]
        inv = np.argsort(perm)
        ob, sm = ob[perm], inv[sm].astype(np.int32)
    return fr, ob, sm, cams, None, truth


def _params():
    fr, ob, sm, cams, _, truth = _plain(n_obs=120, n_hyp=8, seed=39)
    return fr, ob, sm, cams, vel_params(threshold=3.5, huber_delta=5.991, iterations=1), truth


def _all_zero():
    fr, ob, sm, cams, _, truth = _plain(n_obs=100, n_hyp=6, seed=40)
    return fr, ob, sm, cams, vel_params(threshold=1e-6, iterations=0), truth    # no LM: scored at the start velocity


def _nhyp0():
    return _plain(n_obs=50, n_hyp=0, seed=41)


BUILDERS = {"plain": lambda: _plain(n_obs=200, n_hyp=23, seed=1)}
BUILDERS.update({f"nobs_{n}": functools.partial(_nobs, n) for n in N_OBS_EDGES})
BUILDERS.update({f"nhyp_{n}": functools.partial(_nhyp, n) for n in N_HYP_EDGES})
BUILDERS.update({"dup_tie": _dup_tie, "one_cam_triples": _one_cam_triples, "one_dt": _one_dt, "zero_start": _zero_start,
                 "sampled_outlier": _sampled_outlier, "dt0_cam": _dt0_cam, "behind": _behind, "shuffled": _shuffled,
                 "params": _params, "all_zero": _all_zero, "nhyp_0": _nhyp0})
CASES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def _case(name):
    return BUILDERS[name]()


def case(name):
    """(frames, obs, samples, cams, params): fresh copies of the arrays."""
    fr, ob, sm, cams, prm, _ = _case(name)
    return fr.copy(), ob.copy(), np.ascontiguousarray(sm, np.int32).copy(), cams.copy(), prm


def truth(name):
    return _case(name)[5]


def oracle_kw(params, cfg=None):
    cfg = cfg if cfg is not None else track_config()
    kw = dict(tau=cfg.tau, max_trials=cfg.max_trials, early_stop=cfg.early_stop)
    if params is not None:
        kw.update(threshold=params.threshold, huber_delta=params.huber_delta, iterations=params.iterations)
    return kw


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's result per frame, with the settled masks.  Shared and never modified."""
    fr, ob, sm, cams, prm = case(name)
    return vo.reference(fr, ob, sm, cams, **oracle_kw(prm))
