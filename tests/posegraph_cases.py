"""The pose graphs that tests/test_posegraph_cases.py (CPU) and tests/test_gpu_posegraph.py (GPU) share (TEST
INFRASTRUCTURE).  case(name) -> (v, e, fix_scale); reference(name, ...) -> the restatement's run, computed once.

A graph is made from true Sim3 poses S_i: an edge (i, j) measures C = Sim3(noise) S_j S_i^-1, so its error at the truth
is `noise`; the start is Sim3(start noise) S_i for the free vertices.  Under fix_scale every scale is 1 and no noise has
a sigma, except where a case says so.
"""
import functools

import numpy as np

import posegraph_oracle as po
import sim3_oracle as so
from amc_lba.posegraph import PG_EDGE_DTYPE, PG_VERTEX_DTYPE, essential_graph, make_pose_graph


def _unit(S):
    S.r = S.r / np.linalg.norm(S.r)
    return S


def _put(rec, S):
    rec["q"], rec["t"], rec["s"] = S.r / np.linalg.norm(S.r), S.t, S.s


def _noise(rng, rot, trans, sigma):
    return np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3), [rng.normal(0, sigma) if sigma else 0.0]])


def _truth(n, rng, scale_spread=0.0):
    """A walk: a step of about 1.5 m and 0.15 rad of yaw per vertex."""
    out, S = [], so.Sim3([0, 0, 0, 1], [0, 0, 0], 1.0)
    for _ in range(n):
        out.append(_unit(S.copy()))
        step = np.array([rng.normal(0, 0.03), rng.normal(0, 0.03), 0.15 + rng.normal(0, 0.05), 1.5, rng.normal(0, 0.2),
                         rng.normal(0, 0.1), rng.normal(0, scale_spread) if scale_spread else 0.0])
        S = so.sim3_exp(step) * S
    return out


def build(n, pairs, seed, fixed=(0,), start=(0.05, 0.3, 0.0), meas=(0.01, 0.05, 0.0), scale_spread=0.0, noises=None):
    """pairs: (v0, v1) per edge; noises: per-edge error at the truth (overrides `meas`)."""
    rng = np.random.default_rng(seed)
    T = _truth(n, rng, scale_spread)
    v = np.zeros(n, PG_VERTEX_DTYPE)
    for i in range(n):
        free = i not in fixed
        _put(v[i], so.sim3_exp(_noise(rng, *start)) * T[i] if free else T[i])
        v[i]["fixed"] = int(not free)
    e = np.zeros(len(pairs), PG_EDGE_DTYPE)
    for k, (i, j) in enumerate(pairs):
        nz = _noise(rng, *meas) if noises is None else np.asarray(noises[k], float)
        e[k]["v0"], e[k]["v1"] = i, j
        _put(e[k], so.sim3_exp(nz) * T[j] * T[i].inverse())
    return v, e


def _ring(n, extra=()):
    return [(i + 1, i) for i in range(n - 1)] + [(n - 1, 0)] + list(extra)


def _zero_error():
    """Integer translations, no rotation, scale 1: C S0 S1^-1 is the identity in floating point for the chain's edges,
    so their e = 0 exactly; the closing edge is off by (1, 0, 0)."""
    n = 6
    v = np.zeros(n, PG_VERTEX_DTYPE)
    v["q"][:, 3] = 1.0
    v["s"] = 1.0
    v["t"][:, 0] = np.arange(n) * 2.0
    v["fixed"][0] = 1
    pairs = [(i + 1, i) for i in range(n - 1)] + [(n - 1, 0)]
    e = np.zeros(len(pairs), PG_EDGE_DTYPE)
    e["q"][:, 3] = 1.0
    e["s"] = 1.0
    for k, (i, j) in enumerate(pairs):
        e[k]["v0"], e[k]["v1"] = i, j
        e[k]["t"] = v[j]["t"] - v[i]["t"]            # C = S_j S_i^-1: x -> x + t_j - t_i
    e[-1]["t"][0] += 1.0
    return v, e


# the errors at the truth that take Sim3::log through its four branches (|sigma| and d on either side of the thresholds)
BRANCH_NOISES = [
    [1e-3, -2e-3, 1.5e-3, 0.04, -0.02, 0.03, 0.0],        # 0
    [3e-3, -2e-3, 3e-3, 0.04, -0.02, 0.03, 6e-6],         # 1, just below d = 1 - eps
    [0.0, 0.0, 0.0, 0.03, 0.01, -0.02, 0.02],             # 2 (no rotation: the reference's B is wrong there otherwise)
    [0.02, -0.03, 0.05, 0.04, -0.01, 0.02, 0.01],         # 3
    [0.02, -0.03, 0.05, 0.04, -0.01, 0.02, 0.0],          # 1
]


REJECTING_TRIALS = 3


def _rejecting(seed):
    return build(12, _ring(12, [(7, 2), (10, 4)]), seed, start=(0.9, 6.0, 0.0))


def search_rejecting(seeds=range(60)):
    """The search behind "rejecting": the first seed from whose start the Gauss-Newton step (lambda = 1e-16) makes chi2
    worse, so that the LM refuses every trial of its first iteration.

    At the reference's lambda a refusal cannot be repaired inside the iteration: lambda grows by 2, 4, 8, ... from
    1e-16 and reaches 3.5e-3 at the tenth trial, so the trials repeat the same step.  Over the grids searched (starts
    of 0.5 to 1.8 rad and 3 to 12 m on this graph and on complete graphs, 40 to 60 seeds each, also from the default
    lambda) every run that refused a trial in its first three iterations either ended right there or took its tenth
    trial (the only damped one) from a state far from the minimum, where the weak modes of H amplify the numeric
    Jacobian's noise: the numeric and the analytic runs then ended 1e-4 to 1e-2 apart, and condition 2 of
    tests/test_posegraph_cases.py cannot hold.  The case therefore runs with max_trials = REJECTING_TRIALS: all trials
    of the first iteration are refused, the LM stops, and the state must come back untouched -- in the analytic, the
    disturbed and the numeric run alike, which is what the search checks (REJECTING_SEED is its result)."""
    for seed in seeds:
        v, e = _rejecting(seed)
        runs = (po.optimize(v, e, True, 1, 1e-16, max_trials=REJECTING_TRIALS, **kw)
                for kw in (dict(), dict(seed=1), dict(jac="numeric")))   # (lazy: most seeds fail the first run)
        if all(r["rejected"] == REJECTING_TRIALS and r["solve_failures"] == 0 for r in runs):
            return seed
    return None


REJECTING_SEED = 38


def _converged():
    v, e = build(10, _ring(10, [(6, 1)]), 31)
    for _ in range(3):
        v = po.optimize(v, e, True, 20, 1e-16)["v"]
    # (unit quaternions again: the restatement, like g2o, never renormalises, and after 3 runs its own drift of 1e-12
    # would be the largest term of every comparison at this start)
    v["q"] /= np.linalg.norm(v["q"], axis=1, keepdims=True)
    return v, e


def _loop(n, **kw):
    v, e, _ = essential_graph(make_pose_graph(n_kf=n, seed=3, **kw))
    return v, e


def _isolated():
    # vertex 6 has no edge; 0 and 4 are fixed and share an edge (inactive); 7 hangs on the fixed 4 alone
    v, e = build(8, [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (4, 0), (7, 4), (5, 1)], 17, fixed=(0, 4))
    return v, e


_CASES = {
    # name: (maker, fix_scale[, the LM settings that differ from lba_config's defaults])
    "two_one": (lambda: build(2, [(1, 0)], 1), 1),
    "four_active": (lambda: build(5, _ring(5), 2), 1),
    "five_active": (lambda: build(6, _ring(6), 3), 1),
    "fixed_middle": (lambda: build(9, _ring(9), 4, fixed=(4,)), 1),
    "two_fixed": (lambda: build(9, _ring(9), 5, fixed=(0, 5)), 1),
    "isolated_and_fixed_pair": (_isolated, 1),
    "parallel_reversed": (lambda: build(7, _ring(7, [(3, 2), (2, 3), (0, 6), (5, 1), (5, 1)]), 6), 1),
    # (small measurement noise: with 5 cm / 0.01 rad on every one of the hub's 43 edges the residual at the minimum,
    # times the numeric Jacobian's 1e-7 relative noise, put the numeric run 1.05e-6 from the analytic one)
    "hub": (lambda: build(46, _ring(46, [(i, 1) for i in range(3, 46)]), 7, start=(0.02, 0.1, 0.0), meas=(0.002, 0.01, 0.0)), 1),
    "zero_error": (_zero_error, 1),
    # under fix_scale with unit scales sigma stays 0: only the two |sigma| < eps branches can be met
    "log_branches": (lambda: build(6, _ring(6), 8, start=(1e-3, 0.01, 0.0),
                                   noises=[BRANCH_NOISES[0], BRANCH_NOISES[4], [1e-3, 1e-3, -1e-3, 0.0, 0.02, 0.0, 0.0],
                                           [4e-3, -2e-3, 3e-3, 0.01, 0.0, 0.0, 0.0], BRANCH_NOISES[0], BRANCH_NOISES[4]]), 1),
    "log_branches_free": (lambda: build(6, _ring(6), 8, noises=BRANCH_NOISES + [[0.01, 0.0, 0.02, 0.1, 0.0, 0.0, 0.03]],
                                        start=(0.0, 0.0, 0.0), scale_spread=0.05), 0),
    # a start with errors above 1 rad and 30 m from which the Gauss-Newton steps still descend (one closing edge that
    # far off alone is refused outright: the run ends where it began and shows nothing)
    "far": (lambda: build(8, _ring(8), 9, start=(0.45, 14.0, 0.0)), 1),
    "free_scale": (lambda: _loop(40, loop_scale=1.05), 0),
    "loop150": (lambda: _loop(150), 1),
    "rejecting": (lambda: _rejecting(REJECTING_SEED), 1, dict(max_trials=REJECTING_TRIALS)),
    "converged": (_converged, 1),
}
CASES = list(_CASES)
FIXED_SCALE_CASES = [n for n in CASES if _CASES[n][1]]


@functools.lru_cache(maxsize=None)
def _case(name):
    maker, fix = _CASES[name][:2]
    v, e = maker()
    return v, e, fix


def options(name):
    """The LM settings of a case that differ from lba_config's defaults (a tracker for it is made with them)."""
    return dict(_CASES[name][2]) if len(_CASES[name]) > 2 else {}


def case(name):
    v, e, fix = _case(name)
    return v.copy(), e.copy(), fix


@functools.lru_cache(maxsize=None)
def reference(name, jac="analytic", seed=None):
    """The restatement's optimize(20) at the reference's lambda (1e-16), computed once per process."""
    v, e, fix = case(name)
    return po.optimize(v, e, fix, 20, 1e-16, jac=jac, seed=seed, **options(name))


@functools.lru_cache(maxsize=None)
def reference_step(name, lam):
    v, e, fix = case(name)
    return po.step(v, e, fix, lam)
