"""Loop closing's pose-graph optimisation (Optimizer::OptimizeEssentialGraph, src/Optimizer.cc:1434-1717) through the C
ABI (lba_posegraph_* on an lba_tracker): a Sim3 pose graph under g2o's Levenberg, a sparse tile Cholesky on the GPU.

`Tracker.posegraph_optimize` is the call; `posegraph_linearize`, `posegraph_step` and `posegraph_plan_info` expose one
linearisation, one damped step and the host's plan.  Around it, on plain arrays: `essential_graph` restates the
reference's graph construction (:1465-1660), `write_back` its write-back (:1669-1713), and `make_pose_graph` makes a
synthetic map: a lap with drift, a loop, the corrected neighbourhood of the current keyframe.

A Sim3 is (R, t, s) here: x -> s R x + t; records carry it as q (x, y, z, w), t, s.
"""
import ctypes

import numpy as np

from . import LbaError, lib
from .abi import LBA_E_SOLVE, ptr
from .sim3 import quat_of
from .track import Tracker, _bind as _bind_track

PG_VERTEX_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("fixed", "<i4"), ("pad", "<i4")],
                           align=True)
PG_EDGE_DTYPE = np.dtype([("v0", "<i4"), ("v1", "<i4"), ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")], align=True)
assert PG_VERTEX_DTYPE.itemsize == 72
assert PG_EDGE_DTYPE.itemsize == 72
PLAN_INFO_FIELDS = ("na", "panels", "tiles", "fill_tiles", "levels", "chain", "tail", "depth")
MIN_FEAT = 100   # minFeat (:1463)


class LbaPgStats(ctypes.Structure):
    """lba_pg_stats"""
    _fields_ = [("iterations", ctypes.c_int32), ("trials", ctypes.c_int32), ("solve_failures", ctypes.c_int32),
                ("result", ctypes.c_int32), ("chi2_initial", ctypes.c_double), ("chi2_final", ctypes.c_double),
                ("lambda_final", ctypes.c_double), ("panels", ctypes.c_int32), ("tiles", ctypes.c_int32),
                ("fill_tiles", ctypes.c_int32), ("levels", ctypes.c_int32), ("chain", ctypes.c_int32),
                ("launches_per_solve", ctypes.c_int32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


_dp = ctypes.POINTER(ctypes.c_double)


def _bind_host():
    L = lib()
    if not getattr(L, "_pg_host_bound", False):
        vp = ctypes.c_void_p
        L.lba_posegraph_plan_info.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
        L._pg_host_bound = True
    return L


def _bind():
    L = _bind_track()
    _bind_host()
    if not getattr(L, "_pg_bound", False):
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.lba_posegraph_optimize.argtypes = [vp, vp, i32, vp, i32, i32, i32, ctypes.c_double, ctypes.POINTER(LbaPgStats)]
        L.lba_posegraph_linearize.argtypes = [vp, vp, i32, vp, i32, i32, _dp, _dp, _dp]
        L.lba_posegraph_step.argtypes = [vp, vp, i32, vp, i32, i32, ctypes.c_double, _dp, vp, _dp]
        L.lba_posegraph_profile.argtypes = [vp, _dp]
        L._pg_bound = True
    return L


def _arrays(v, e):
    return np.ascontiguousarray(v, PG_VERTEX_DTYPE), np.ascontiguousarray(e, PG_EDGE_DTYPE)


def _d(a):
    return a.ctypes.data_as(_dp)


def posegraph_plan_info(v, e):
    """lba_posegraph_plan_info (host only, no device): dict of PLAN_INFO_FIELDS."""
    v, e = _arrays(v, e)
    info = np.zeros(8, np.int32)
    rc = _bind_host().lba_posegraph_plan_info(ptr(v), len(v), ptr(e), len(e), info.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc < 0:
        raise LbaError(rc, "lba_posegraph_plan_info failed")
    return dict(zip(PLAN_INFO_FIELDS, (int(x) for x in info)))


def posegraph_optimize(tracker, v, e, fix_scale=True, iterations=20, lambda_init=1e-16):
    """optimize(iterations) of the pose graph; the reference's user lambda is 1e-16 (:1447), lambda_init <= 0 means
    tau max|H_ii|.  An array of PG_VERTEX_DTYPE is updated in place (active free vertices only) and returned with
    the lba_pg_stats as a dict."""
    v, e = _arrays(v, e)
    st = LbaPgStats()
    rc = _bind().lba_posegraph_optimize(tracker.h, ptr(v), len(v), ptr(e), len(e), int(bool(fix_scale)), int(iterations),
                                        float(lambda_init), ctypes.byref(st))
    if rc < 0:
        raise LbaError(rc, "lba_posegraph_optimize failed")
    return v, st.as_dict()


def posegraph_linearize(tracker, v, e, fix_scale=True):
    """(errors [n_e, 7], dense H [7 na, 7 na] without lambda, b [7 na]) at the vertices' estimates."""
    v, e = _arrays(v, e)
    na = posegraph_plan_info(v, e)["na"]
    err, H, b = np.zeros((len(e), 7)), np.zeros((7 * na, 7 * na)), np.zeros(7 * na)
    rc = _bind().lba_posegraph_linearize(tracker.h, ptr(v), len(v), ptr(e), len(e), int(bool(fix_scale)), _d(err), _d(H), _d(b))
    if rc < 0:
        raise LbaError(rc, "lba_posegraph_linearize failed")
    return err, H, b


def posegraph_step(tracker, v, e, fix_scale=True, lam=1e-16):
    """One damped step: (ok, dx [7 na], trial vertices, chi2 of the trial); ok False (nothing else valid) when the
    factorisation meets a pivot that is not positive."""
    v, e = _arrays(v, e)
    na = posegraph_plan_info(v, e)["na"]
    dx, trial, chi = np.zeros(7 * na), np.zeros(len(v), PG_VERTEX_DTYPE), ctypes.c_double(0.0)
    rc = _bind().lba_posegraph_step(tracker.h, ptr(v), len(v), ptr(e), len(e), int(bool(fix_scale)), float(lam), _d(dx),
                                    ptr(trial), ctypes.byref(chi))
    if rc == LBA_E_SOLVE:
        return False, dx, trial, float("nan")
    if rc < 0:
        raise LbaError(rc, "lba_posegraph_step failed")
    return True, dx, trial, chi.value


def posegraph_ms(tracker):
    """Measurement: (host planning, upload, device) milliseconds of the tracker's last posegraph_optimize."""
    ms = np.zeros(3)
    rc = _bind().lba_posegraph_profile(tracker.h, _d(ms))
    if rc != 0:
        raise LbaError(rc, "lba_posegraph_profile failed")
    return tuple(float(x) for x in ms)


Tracker.posegraph_optimize = posegraph_optimize
Tracker.posegraph_linearize = posegraph_linearize
Tracker.posegraph_step = posegraph_step
Tracker.posegraph_ms = posegraph_ms


# ---------------------------------------------------------------------------------------------- Sim3 on (R, t, s)
def s_mul(a, b):
    return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]


def s_inv(a):
    return a[0].T, a[0].T @ ((-1.0 / a[2]) * a[1]), 1.0 / a[2]


def s_map(a, x):
    return a[2] * (a[0] @ x) + a[1]


def s_of(rec):
    from .synth import quat_to_rot
    q = np.asarray(rec["q"], float)
    return quat_to_rot(q / np.linalg.norm(q)), np.array(rec["t"], float), float(rec["s"])


def _put(rec, S):
    rec["q"], rec["t"], rec["s"] = quat_of(S[0]), S[1], S[2]


# ---------------------------------------------------------------------------------------------- the caller's side
def essential_graph(m):
    """The graph of OptimizeEssentialGraph (:1465-1660) from a map given as a dict of plain containers:
      ids [n]            mnId of every keyframe, ascending       bad [n]      isBad()
      pose [n]           GetPose() as (R, t), Tiw                init_id      pMap->GetInitKFid()
      parent [n]         mnId of GetParent(), or -1              loop_edges   {id: set of ids}, GetLoopEdges()
      covis [n]          GetCovisiblesByWeight(0): [(id, weight)] by falling weight (GetWeight reads it too)
      corrected, non_corrected   {id: (R, t, s)}: CorrectedSim3, NonCorrectedSim3
      loop_connections   {id: set of ids}                        cur_id, loop_id   pCurKF, pLoopKF
    Vertices: the keyframes that are not bad, in id order, CorrectedSim3 where there is one, else (GetPose(), 1); the
    initial keyframe fixed.  Edges, in the reference's order: the loop connections (weight >= minFeat, or the pair
    (current, loop) itself), recorded in sInsertedEdges; then per keyframe its spanning-tree edge, its earlier loop
    edges with a lower id, and its covisibles of weight >= minFeat with a lower id that are not bad, not its parent,
    not a child and not in sInsertedEdges.  A measurement is Sjw Swi with the non-corrected pose of either end where
    there is one (the loop connections: always the vertices' estimates).  An edge with a keyframe that has no vertex is
    skipped, as g2o refuses it.  Returns (v, e, vertex_ids)."""
    ids = [int(i) for i in m["ids"]]
    row = {k: i for i, k in enumerate(ids)}
    alive = [k for k in ids if not m["bad"][row[k]]]
    vid = {k: i for i, k in enumerate(alive)}
    vS = {}
    v = np.zeros(len(alive), PG_VERTEX_DTYPE)
    for k in alive:
        S = m["corrected"].get(k)
        if S is None:
            R, t = m["pose"][row[k]]
            S = (np.asarray(R, float), np.asarray(t, float), 1.0)
        vS[k] = S
        _put(v[vid[k]], S)
        v[vid[k]]["fixed"] = int(k == m["init_id"])
    children = {k: set() for k in ids}
    for k in ids:
        p = int(m["parent"][row[k]])
        if p >= 0 and p in children:
            children[p].add(k)

    def weight(a, b):
        return next((w for k, w in m["covis"][row[a]] if k == b), 0)

    edges, inserted = [], set()

    def add(i, j, Sji):
        if i in vid and j in vid:
            edges.append((vid[i], vid[j], Sji))

    for i in sorted(m["loop_connections"]):
        if i not in vS:
            continue
        Swi = s_inv(vS[i])
        for j in sorted(m["loop_connections"][i]):
            if (i != m["cur_id"] or j != m["loop_id"]) and weight(i, j) < MIN_FEAT:
                continue
            if j not in vS:
                continue
            add(i, j, s_mul(vS[j], Swi))
            inserted.add((min(i, j), max(i, j)))

    def old(k):
        S = m["non_corrected"].get(k)
        return S if S is not None else vS.get(k)

    for i in ids:
        if old(i) is None:
            continue
        Swi = s_inv(old(i))
        p = int(m["parent"][row[i]])
        if p >= 0 and old(p) is not None:
            add(i, p, s_mul(old(p), Swi))
        for l in sorted(m["loop_edges"].get(i, ())):
            if l < i and old(l) is not None:
                add(i, l, s_mul(old(l), Swi))
        for n, w in m["covis"][row[i]]:
            if w < MIN_FEAT:
                break
            if n == p or n in children[i]:
                continue
            if n in row and not m["bad"][row[n]] and n < i:
                if (min(i, n), max(i, n)) in inserted:
                    continue
                add(i, n, s_mul(old(n), Swi))
    e = np.zeros(len(edges), PG_EDGE_DTYPE)
    for k, (a, b, S) in enumerate(edges):
        e[k]["v0"], e[k]["v1"] = a, b
        _put(e[k], S)
    return v, e, np.array(alive, np.int64)


def write_back(m, v0, v_opt, vertex_ids):
    """The write-back (:1669-1713).  v0: the vertices as passed to the optimiser (vScw), v_opt: as returned.
    Returns (poses {id: (R float32, t float32)}: SetPose([R, t / s]), points [n, 3] float32: every point that is not
    bad moved through its reference keyframe, correctedSwr.map(Srw.map(Xw)); a bad one is left as it is).
    m adds: points [n, 3] float32, point_bad [n], point_ref [n] (mnId of GetReferenceKeyFrame()), point_corrected_by
    [n] (mnCorrectedByKF), point_corrected_ref [n] (mnCorrectedReference)."""
    vid = {int(k): i for i, k in enumerate(vertex_ids)}
    poses, swc = {}, {}
    for k, i in vid.items():
        S = s_of(v_opt[i])
        swc[k] = s_inv(S)
        poses[k] = (S[0].astype(np.float32), S[1].astype(np.float32) / np.float32(S[2]))
    pts = np.array(m["points"], np.float32)
    for n in range(len(pts)):
        if m["point_bad"][n]:
            continue
        r = int(m["point_corrected_ref"][n]) if m["point_corrected_by"][n] == m["cur_id"] else int(m["point_ref"][n])
        X = s_map(swc[r], s_map(s_of(v0[vid[r]]), pts[n].astype(np.float64)))
        pts[n] = X.astype(np.float32)
    return poses, pts


def make_pose_graph(n_kf=60, seed=0, radius=20.0, drift_rot=0.004, drift_trans=0.03, n_corrected=5, covis_reach=4,
                    loop_scale=1.0, n_points=0, old_loop=False):
    """A synthetic map for essential_graph: `n_kf` keyframes on one lap of a circle of `radius` metres whose odometry
    drifts (per step a rotation of `drift_rot` rad and `drift_trans` m of noise), so the last keyframe, which stands
    again where the first one stood, is off by the accumulated drift.  The loop (current = last keyframe, loop
    keyframe = the first) corrects the current keyframe and its `n_corrected` - 1 predecessors: CorrectedSim3 =
    Sic S_cur_corrected with scale `loop_scale`, NonCorrectedSim3 their poses; LoopConnections link them with the loop
    keyframe and its neighbours.  Spanning tree: the previous keyframe (every fifth: the one before it); covisibility
    weights fall with the distance in time, `covis_reach` deep, around minFeat = 100 at its end.  old_loop: an earlier
    loop edge between keyframes n_kf // 3 and 2.  n_points: map points with reference keyframes.  Poses are float
    values, as GetPose() returns them.  Returns the dict essential_graph takes."""
    from .synth import _expso3, _f32, _rotz
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n_kf) / (n_kf - 1)
    Twi = [(_rotz(a + np.pi / 2), radius * np.array([np.cos(a), np.sin(a), 0.0])) for a in ang]
    drift = [Twi[0]]
    for i in range(1, n_kf):
        Ra, ta = Twi[i - 1]
        Rb, tb = Twi[i]
        Rr, tr = Ra.T @ Rb, Ra.T @ (tb - ta)                      # the true step, then its noise
        Rr = Rr @ _expso3(rng.normal(0, drift_rot, 3))
        tr = tr + rng.normal(0, drift_trans, 3)
        Rp, tp = drift[-1]
        drift.append((Rp @ Rr, Rp @ tr + tp))
    pose = [(_f32(R.T), _f32(-R.T @ t)) for R, t in drift]      # Tiw
    ids = np.arange(n_kf) * 2 + 1                                 # (ids with gaps: a vertex index is not an id)
    parent = np.full(n_kf, -1, np.int64)
    for i in range(1, n_kf):
        parent[i] = ids[i - 2] if i % 5 == 0 and i >= 2 else ids[i - 1]
    covis = []
    for i in range(n_kf):
        c = []
        for d in range(1, covis_reach + 1):
            w = int(330 - 70 * d + rng.integers(-25, 26))
            for j in (i - d, i + d):
                if 0 <= j < n_kf:
                    c.append((int(ids[j]), w))
        covis.append(sorted(c, key=lambda kw: -kw[1]))
    cur, loop = n_kf - 1, 0
    # the loop's Sim3: the current keyframe seen from the loop keyframe, truth plus a little noise
    Rt, tt = Twi[cur]
    Rl, tl = Twi[loop]
    Rcl = Rt.T @ Rl @ _expso3(rng.normal(0, 1e-3, 3))
    tcl = Rt.T @ (tl - tt) + rng.normal(0, 0.01, 3)
    S_lw = (pose[loop][0], pose[loop][1], 1.0)
    S_cw_new = s_mul((Rcl, loop_scale * tcl, loop_scale), S_lw)
    S_cw_old = (pose[cur][0], pose[cur][1], 1.0)
    corrected, non_corrected = {}, {}
    for i in range(n_kf - n_corrected, n_kf):
        S_iw = (pose[i][0], pose[i][1], 1.0)
        non_corrected[int(ids[i])] = S_iw
        corrected[int(ids[i])] = s_mul(s_mul(S_iw, s_inv(S_cw_old)), S_cw_new)
    # after the fusion the corrected keyframes see the loop keyframe's neighbourhood
    loop_connections = {int(ids[cur]): {int(ids[loop]), int(ids[loop + 1])}, int(ids[cur - 1]): {int(ids[loop])}}
    for a, bs in loop_connections.items():
        for b in bs:
            w = 180 if (a, b) != (int(ids[cur - 1]), int(ids[loop])) else 60   # (the last one: below minFeat)
            covis[(a - 1) // 2].append((b, w))
            covis[(b - 1) // 2].append((a, w))
    covis = [sorted(c, key=lambda kw: -kw[1]) for c in covis]
    loop_edges = {}
    if old_loop:
        a, b = int(ids[n_kf // 3]), int(ids[2])
        loop_edges = {a: {b}, b: {a}}
    m = dict(ids=ids, bad=np.zeros(n_kf, bool), pose=pose, init_id=int(ids[0]), parent=parent, loop_edges=loop_edges,
             covis=covis, corrected=corrected, non_corrected=non_corrected, loop_connections=loop_connections,
             cur_id=int(ids[cur]), loop_id=int(ids[loop]))
    if n_points:
        ref = rng.integers(0, n_kf, n_points)
        pts = np.zeros((n_points, 3), np.float32)
        for n, i in enumerate(ref):
            R, t = drift[i]
            pts[n] = (R @ np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(4, 15)]) + t).astype(np.float32)
        m.update(points=pts, point_bad=rng.random(n_points) < 0.1, point_ref=ids[ref],
                 point_corrected_by=np.where(ref >= n_kf - n_corrected, ids[cur], -1),
                 point_corrected_ref=ids[ref])
    return m
