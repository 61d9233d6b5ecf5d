"""Ordering and symbolic factorisation of the reduced camera system (amc-slam_amd/csrc/lba_plan.hpp, the
replacement of LinearSolverEigen's AMD-ordered SimplicialLDLT, Thirdparty/g2o/g2o/solvers/
linear_solver_eigen.h:60-124, at 32-row panel granularity), on the host: the order is a permutation with
the extrinsic panels last, the stored tiles of L are exactly the fill of a boolean elimination of the
permuted pattern, the update order is topological, and the dependent chain of band, loop-closure and
multi-revisit patterns is far below the panel count."""
import ctypes

import numpy as np
import pytest

I = ctypes.POINTER(ctypes.c_int)


def _p(a):
    return a.ctypes.data_as(I)


def plan(h, NP, pairs, NPk=None, levels=64, tail=True, method=0):
    NPk = NP if NPk is None else NPk
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    info = np.zeros(4, np.int32)
    ppos, uord = np.zeros(NP, np.int32), np.zeros(NP, np.int32)
    rowptr = np.zeros(NP + 1, np.int32)
    cap = NP * NP
    cols = np.zeros(cap, np.int32)
    nt = h.plan_probe(NP, NPk, len(pr), _p(pr), levels, int(tail), method, _p(info), _p(ppos), _p(uord), _p(rowptr),
                      _p(cols), cap)
    assert nt == info[3] >= NP
    return dict(chain=int(info[0]), tail=int(info[1]), levels=int(info[2]), ntile=int(nt), ppos=ppos, uord=uord,
                rowptr=rowptr, cols=cols[:nt])


def band_pairs(NP, w):
    return [(P, Q) for P in range(NP) for Q in range(max(0, P - w + 1), P)]


def revisit_pairs(NP, w, laps):
    """Panels of a trajectory of `laps` laps: a panel couples every panel within w of its position on
    the lap, on any lap (a place revisited laps - 1 times)."""
    per = NP / laps
    pos = np.arange(NP) % per
    d = np.abs(pos[:, None] - pos[None, :])
    d = np.minimum(d, per - d)
    P, Q = np.nonzero(np.tril(d < w, -1))
    return np.stack([P, Q], 1)


def check_plan(NP, pairs, pl, NPk=None):
    NPk = NP if NPk is None else NPk
    ppos = pl["ppos"]
    assert sorted(ppos.tolist()) == list(range(NP))
    assert sorted(pl["uord"].tolist()) == list(range(NP))
    assert all(ppos[P] == P for P in range(NPk, NP))   # extrinsic panels last, in order
    # boolean elimination of the permuted pattern
    M = np.eye(NP, dtype=bool)
    for P, Q in pairs:
        i, j = ppos[P], ppos[Q]
        M[max(i, j), min(i, j)] = True
    for j in range(NP):
        rows = j + 1 + np.nonzero(M[j + 1:, j])[0]
        if rows.size:
            M[np.ix_(rows, rows)] |= np.tril(np.ones((rows.size, rows.size), bool))
    L = np.tril(M)
    got = np.zeros((NP, NP), bool)
    for i in range(NP):
        cs = pl["cols"][pl["rowptr"][i]:pl["rowptr"][i + 1]]
        assert cs[-1] == i and np.all(np.diff(cs) > 0) if cs.size > 1 else cs[-1] == i
        got[i, cs] = True
    np.testing.assert_array_equal(got, L)
    # elimination-tree depth = reported chain; the update order is topological
    rank = np.empty(NP, int)
    rank[pl["uord"]] = np.arange(NP)
    depth = np.ones(NP, int)
    for j in range(NP):
        below = np.nonzero(L[j + 1:, j])[0]
        if below.size:
            par = j + 1 + below[0]
            depth[par] = max(depth[par], depth[j] + 1)
            assert np.all(rank[j + 1 + below] > rank[j])
    assert depth.max() == pl["chain"]


@pytest.mark.parametrize("NP,w", [(19, 5), (60, 3), (188, 4), (300, 2)])
def test_band(plan_harness, NP, w):
    pr = band_pairs(NP, w)
    pl = plan(plan_harness, NP, pr)
    check_plan(NP, pr, pl)
    assert pl["tail"] == 0
    if NP >= 60:
        assert pl["chain"] <= NP // 3 and pl["levels"] >= 2, pl["chain"]
    nat = plan(plan_harness, NP, pr, levels=0)
    check_plan(NP, pr, nat)
    assert nat["chain"] == NP and nat["ntile"] == sum(min(P + 1, w) for P in range(NP))


@pytest.mark.parametrize("laps", [1, 2, 3, 4])
def test_revisits(plan_harness, laps):
    """One loop closure (laps=1: the end meets the start) and two or three revisits of the same places:
    the interval dissection of the time order cannot separate laps that couple each other, the graph
    dissection (breadth-first level structures) can; the plan keeps the shorter chain."""
    NP, w = 240, 3
    pr = revisit_pairs(NP, w, laps)
    pl = plan(plan_harness, NP, pr)
    check_plan(NP, pr, pl)
    g = plan(plan_harness, NP, pr, method=2)
    iv = plan(plan_harness, NP, pr, method=1)
    check_plan(NP, pr, g)
    check_plan(NP, pr, iv)
    assert pl["chain"] == min(g["chain"], iv["chain"])
    assert pl["chain"] <= NP // 3, (pl["chain"], g["chain"], iv["chain"])
    if laps >= 3:
        assert g["chain"] < iv["chain"]


def test_extrinsic_panels_last(plan_harness):
    NP, NPk = 70, 66
    pr = band_pairs(NPk, 3) + [(P, Q) for P in range(NPk, NP) for Q in range(P)]
    for method in (0, 1, 2):
        pl = plan(plan_harness, NP, pr, NPk=NPk, method=method)
        check_plan(NP, pr, pl, NPk=NPk)


def flow(h, NP, pairs, band, nranks=1, me=0, which=0):
    """One task list of lba_plan::flow_tasks for the plan `plan(h, NP, pairs)` makes."""
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    sizes = np.zeros(2, np.int32)
    args = (NP, NP, len(pr), _p(pr), int(band), nranks, me, which, _p(sizes))
    assert h.flow_probe(*args, None, None, None, None, None, None) == 0
    nt, ne = int(sizes[0]), int(sizes[1])
    tasks, task_i, task_t = np.zeros(nt, np.int32), np.zeros(nt, np.int32), np.zeros((nt, 5), np.int32)
    pl0, plist, plist_t = np.full(nt + 2, -7, np.int32), np.zeros(ne, np.int32), np.zeros((ne, 3), np.int32)
    assert h.flow_probe(*args, _p(tasks), _p(task_i), _p(task_t), _p(pl0), _p(plist), _p(plist_t)) == 0
    assert pl0[nt + 1] == -7   # pl0 has exactly one more element than tasks (the probe checks its length too)
    return dict(j=tasks & 0xffffff, kind=(tasks >> 24) & 15, i=task_i, t=task_t, pl0=pl0[:nt + 1], pp=plist & 0xffffff,
                pt=plist_t)


def split_own(h, NP, pairs, nranks):
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    own, parent = np.zeros(NP, np.int32), np.zeros(NP, np.int32)
    h.split_probe(NP, NP, len(pr), _p(pr), nranks, _p(own), _p(parent))
    return own


def check_lists(lists, ntile):
    """What holds for the lists of one rank's launches, in launch order: pl0, the tile ids, the diagonal first, and
    the topological order (an entry's source panel has all its factor tasks earlier)."""
    for fl in lists:
        nt = len(fl["j"])
        assert fl["pl0"][0] == 0 and np.all(np.diff(fl["pl0"]) >= 0) and fl["pl0"][nt] == len(fl["pp"])
        for ids in (fl["t"], fl["pt"]):
            assert np.all(ids >= -1) and np.all(ids < ntile)
    j = np.concatenate([fl["j"] for fl in lists])
    i = np.concatenate([fl["i"] for fl in lists])
    kind = np.concatenate([fl["kind"] for fl in lists])
    entries = []
    for fl in lists:
        entries += [fl["pp"][fl["pl0"][t]:fl["pl0"][t + 1]] for t in range(len(fl["j"]))]
    last_factor, diag_at = {}, {}
    for t in np.nonzero(kind == 0)[0]:
        last_factor[int(j[t])] = int(t)
        if i[t] == j[t]:
            diag_at.setdefault(int(j[t]), int(t))
        assert diag_at.get(int(j[t]), t + 1) <= t, (t, j[t], i[t])   # the diagonal task before the off-diagonal ones
    for t, pps in enumerate(entries):
        for pp in pps:
            assert last_factor.get(int(pp), len(j)) < t, (t, int(j[t]), int(i[t]), int(kind[t]), int(pp))


FLOW_PATTERNS = {
    "band8": (8, band_pairs(8, 3)),
    "band19": (19, band_pairs(19, 5)),
    "band24": (24, band_pairs(24, 2)),
    "revisit24": (24, revisit_pairs(24, 3, 2)),
    "tail20": (20, band_pairs(20, 3) + [(19, 0), (19, 1), (18, 0)]),
}


@pytest.mark.parametrize("band", [0, 1])
@pytest.mark.parametrize("name", sorted(FLOW_PATTERNS))
def test_flow_tasks(plan_harness, name, band):
    """k_chol_flow's task lists (lba_plan::flow_tasks), unsplit, with L^-1 tiles and as a substitution solve."""
    NP, pr = FLOW_PATTERNS[name]
    pl = plan(plan_harness, NP, pr)
    fl = flow(plan_harness, NP, pr, band)
    assert len(flow(plan_harness, NP, pr, band, which=1)["j"]) == 0   # unsplit: everything in the first list
    check_lists([fl], pl["ntile"])
    # every stored tile (i, c) of L is the target of exactly one factor task
    f = fl["kind"] == 0
    target = np.where(fl["i"][f] == fl["j"][f], fl["t"][f, 0], fl["t"][f, 1])
    assert sorted(target.tolist()) == list(range(pl["ntile"]))
    row_of = np.repeat(np.arange(NP), np.diff(pl["rowptr"]))
    np.testing.assert_array_equal(row_of[target], fl["i"][f])
    np.testing.assert_array_equal(pl["cols"][target], fl["j"][f])
    # one solution per panel: kind 2 (L^-1 tiles) or kind 5 (back substitution)
    assert sorted(fl["j"][fl["kind"] == (5 if band else 2)].tolist()) == list(range(NP))


@pytest.mark.parametrize("me", [0, 1])
@pytest.mark.parametrize("name", sorted(FLOW_PATTERNS))
def test_flow_tasks_split(plan_harness, name, me):
    """The distributed factorisation's two lists on each of 2 ranks."""
    NP, pr = FLOW_PATTERNS[name]
    pl = plan(plan_harness, NP, pr)
    own = split_own(plan_harness, NP, pr, 2)
    A = flow(plan_harness, NP, pr, 1, nranks=2, me=me, which=0)
    B = flow(plan_harness, NP, pr, 1, nranks=2, me=me, which=1)
    check_lists([A, B], pl["ntile"])
    row_of = np.repeat(np.arange(NP), np.diff(pl["rowptr"]))
    mine = (own == me) | (own < 0)
    # list A touches only this rank's subtree and the top tiles
    assert np.all(mine[A["j"]]) and np.all(mine[A["i"]]) and np.all(mine[A["pp"]])
    for ids in (A["t"], A["pt"]):
        ids = ids[ids >= 0]
        assert np.all(mine[row_of[ids]]) and np.all(mine[pl["cols"][ids]])
    fa = A["kind"] == 0
    assert np.all(own[A["j"][fa]] == me)            # it factors the subtree's columns ...
    assert np.all(own[A["j"][A["kind"] >= 6]] < 0)  # ... and sums its contributions into top tiles / panels
    # list B targets only top columns (factor and forward tasks), updated from top panels only
    fb = (B["kind"] == 0) | (B["kind"] == 4)
    assert np.all(own[B["j"][fb]] < 0)
    for t in np.nonzero(fb)[0]:
        assert np.all(own[B["pp"][B["pl0"][t]:B["pl0"][t + 1]]] < 0)
    # together the two ranks' lists A and every rank's list B factor each tile once
    fac = [(int(j), int(i)) for L in (A, B) for j, i in zip(L["j"][L["kind"] == 0], L["i"][L["kind"] == 0])]
    want = [(int(pl["cols"][q]), int(row_of[q])) for q in range(pl["ntile"]) if mine[pl["cols"][q]]]
    assert sorted(fac) == sorted(want)


def plan_leaf(h, NP, pairs, leaf, diagonal, method=0):
    """plan() through plan_probe_leaf: make_plan at another leaf size, with or without the diagonal in lower[P]."""
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    info = np.zeros(4, np.int32)
    ppos, uord = np.zeros(NP, np.int32), np.zeros(NP, np.int32)
    rowptr = np.zeros(NP + 1, np.int32)
    cap = NP * NP
    cols = np.zeros(cap, np.int32)
    nt = h.plan_probe_leaf(NP, NP, len(pr), _p(pr), 64, 1, method, leaf, int(diagonal), _p(info), _p(ppos), _p(uord),
                           _p(rowptr), _p(cols), cap)
    assert nt == info[3] >= NP
    return dict(chain=int(info[0]), tail=int(info[1]), levels=int(info[2]), ntile=int(nt), ppos=ppos, uord=uord,
                rowptr=rowptr, cols=cols[:nt])


def _posegraph_topology_cases():
    import posegraph_topology_cases as tc
    return tc.SINGLE_COMPONENT_CASES + tc.COMPONENT_CASES


@pytest.mark.parametrize("name", _posegraph_topology_cases())
def test_posegraph_settings(plan_harness, name):
    """make_plan as the pose graph calls it (lba_posegraph.hip's pg_plan: leaf 2, no diagonal in lower[P], 64 levels,
    tail search) on the panel graphs of tests/posegraph_topology_cases.py: a panel is four active free vertices in array
    order.  Every method's plan is the boolean elimination's; method 0's tile count and chain are what
    lba_posegraph_plan_info reports for the graph."""
    import posegraph_oracle as po
    import posegraph_topology_cases as tc
    from amc_lba.posegraph import posegraph_plan_info
    v, e, _ = tc.case(name)
    ea, slot = po.activity(v, e)
    s0, s1 = slot[e["v0"][ea]], slot[e["v1"][ea]]
    both = (s0 >= 0) & (s1 >= 0)
    P, Q = s0[both] // 4, s1[both] // 4
    pr = sorted({(int(max(a, b)), int(min(a, b))) for a, b in zip(P, Q) if a != b})
    info = posegraph_plan_info(v, e)
    NP = info["panels"]
    assert NP == (int((slot >= 0).sum()) + 3) // 4 and pr
    for method in (0, 1, 2):
        pl = plan_leaf(plan_harness, NP, pr, 2, False, method)
        check_plan(NP, pr, pl)
        if method == 0:
            assert (pl["ntile"], pl["chain"]) == (info["tiles"], info["chain"])


def test_random_sparse(plan_harness):
    rng = np.random.default_rng(3)
    for NP in (40, 120):
        pr = band_pairs(NP, 2) + [tuple(sorted(rng.choice(NP, 2, replace=False)))[::-1] for _ in range(NP // 8)]
        pl = plan(plan_harness, NP, pr)
        check_plan(NP, pr, pl)
