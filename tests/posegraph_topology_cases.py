"""Pose graphs whose elimination structure goes beyond the rings with chords of tests/posegraph_cases.py (TEST
INFRASTRUCTURE): open chains and trees, grids, complete graphs, laps that revisit their places, random connected graphs,
several components, and the same graphs with an array order unrelated to the graph order.  Shared by
tests/test_posegraph_topology_cases.py and tests/test_plan.py (CPU) and tests/test_gpu_posegraph_topologies.py (GPU).

case(name) -> (v, e, fix_scale); reference(name, ...) and reference_step(name, lam): the restatement's runs, computed
once per process.  Every graph is built by posegraph_cases.build with seed 11, a start 0.02 rad / 0.1 m from the truth
and a measurement noise of 0.002 rad / 0.01 m.  A permuted case is the built case with its vertex array and edge
indices permuted: the same truth, start and measurements under another labelling.
"""
import functools

import numpy as np

import posegraph_cases as pc
import posegraph_oracle as po

SEED = 11
START = (0.02, 0.1, 0.0)
MEAS = (0.002, 0.01, 0.0)


# ---------------------------------------------------------------------------------------------- pair lists
def chain_pairs(n):
    return [(i + 1, i) for i in range(n - 1)]


def tree_pairs(n):
    """A binary tree in heap order: vertex i hangs on (i - 1) // 2."""
    return [(i, (i - 1) // 2) for i in range(1, n)]


def grid_pairs(rows, cols):
    """A 4-connected grid, vertices row-major."""
    out = []
    for r in range(rows):
        for c in range(cols):
            i = r * cols + c
            if c + 1 < cols:
                out.append((i + 1, i))
            if r + 1 < rows:
                out.append((i + cols, i))
    return out


def complete_pairs(n):
    return [(i, j) for i in range(n) for j in range(i)]


def laps_pairs(laps, per, every=3):
    """A chain of laps * per vertices; every `every`-th vertex is tied to its place on each earlier lap."""
    n = laps * per
    out = chain_pairs(n)
    for i in range(0, n, every):
        out += [(i, j) for j in range(i - per, -1, -per)]
    return out


def random_connected_pairs(n, n_edges, seed):
    """A random spanning tree (vertex i hangs on a random earlier one) and random further pairs, none twice."""
    rng = np.random.default_rng(seed)
    have = {(i, int(rng.integers(0, i))) for i in range(1, n)}
    while len(have) < n_edges:
        a, b = (int(x) for x in rng.choice(n, 2, replace=False))
        have.add((max(a, b), min(a, b)))
    return sorted(have)


def offset_pairs(pairs, by):
    return [(a + by, b + by) for a, b in pairs]


# the three components: a ring of 30 with one chord, a 3 x 3 grid, one edge
COMPONENT_SIZES = (30, 9, 2)
COMPONENT_FIXED = (0, 30, 39)


def component_pairs():
    return chain_pairs(30) + [(29, 0), (17, 4)] + offset_pairs(grid_pairs(3, 3), 30) + [(40, 39)]


def component_labels():
    """The component of each of the 41 vertices of component_pairs(), in the unpermuted array order."""
    return np.repeat(np.arange(len(COMPONENT_SIZES)), COMPONENT_SIZES)


def permutation(n, seed=5):
    """p[i]: the new index of vertex i."""
    return np.random.default_rng(seed).permutation(n)


def permute(v, e, p):
    """The same graph with vertex i at index p[i] (vertex records and edge measurements untouched)."""
    p = np.asarray(p)
    vp = np.empty_like(v)
    vp[p] = v
    ep = e.copy()
    ep["v0"], ep["v1"] = p[e["v0"]], p[e["v1"]]
    return vp, ep


def _build(n, pairs, fixed=(0,), **kw):
    return pc.build(n, pairs, SEED, fixed=fixed, start=START, meas=MEAS, **kw)


def _permuted(name):
    v, e, _ = _case(name)
    return permute(v, e, permutation(len(v)))


def _floating():
    v, e = _build(41, component_pairs(), fixed=COMPONENT_FIXED)
    v["fixed"][COMPONENT_FIXED[1]] = 0              # the 3 x 3 grid: no gauge
    return v, e


_CASES = {
    # name: (maker, fix_scale)
    "chain41": (lambda: _build(41, chain_pairs(41)), 1),
    "tree63": (lambda: _build(63, tree_pairs(63)), 1),
    "grid6x6": (lambda: _build(36, grid_pairs(6, 6)), 1),
    "grid12x12": (lambda: _build(144, grid_pairs(12, 12)), 1),
    "complete21": (lambda: _build(21, complete_pairs(21)), 1),
    "complete26": (lambda: _build(26, complete_pairs(26)), 1),
    "laps3x40": (lambda: _build(120, laps_pairs(3, 40)), 1),
    "random100_180": (lambda: _build(100, random_connected_pairs(100, 180, 1)), 1),
    "random60_400": (lambda: _build(60, random_connected_pairs(60, 400, 2)), 1),
    "grid12x12_permuted": (lambda: _permuted("grid12x12"), 1),
    "laps3x40_permuted": (lambda: _permuted("laps3x40"), 1),
    "components": (lambda: _build(41, component_pairs(), fixed=COMPONENT_FIXED), 1),
    "components_permuted": (lambda: _permuted("components"), 1),
    "grid6x6_free": (lambda: _build(36, grid_pairs(6, 6), scale_spread=0.05), 0),
    "random60_400_free": (lambda: _build(60, random_connected_pairs(60, 400, 2), scale_spread=0.05), 0),
    "floating": (_floating, 1),
}
CASES = list(_CASES)
# `floating` has a component without a fixed vertex: its undamped system is singular; only the damped step is run
SOLVED_CASES = [n for n in CASES if n != "floating"]
COMPONENT_CASES = ["components", "components_permuted"]
SINGLE_COMPONENT_CASES = [n for n in SOLVED_CASES if n not in COMPONENT_CASES]
# (permuted case, the case it relabels)
RELABELLED = [("grid12x12_permuted", "grid12x12"), ("laps3x40_permuted", "laps3x40")]


@functools.lru_cache(maxsize=None)
def _case(name):
    maker, fix = _CASES[name]
    v, e = maker()
    return v, e, fix


def case(name):
    v, e, fix = _case(name)
    return v.copy(), e.copy(), fix


@functools.lru_cache(maxsize=None)
def reference(name, jac="analytic", seed=None):
    """The restatement's optimize(20) at the reference's lambda (1e-16), computed once per process."""
    v, e, fix = case(name)
    return po.optimize(v, e, fix, 20, 1e-16, jac=jac, seed=seed)


@functools.lru_cache(maxsize=None)
def reference_step(name, lam):
    v, e, fix = case(name)
    return po.step(v, e, fix, lam)
