"""Tracking::MCRansac's hypotheses restated in numpy: the checker of lba_track_vel_ransac (TEST INFRASTRUCTURE).

Independent of the product: nothing of amc-slam_amd/csrc is used, only the oracle's exported primitives
orc.se3_exp, orc.right_jac_pose3 and orc.ldlt_solve.  What is restated, with the reference's lines:

  vertex   VertexVel, 6-d, additive update (include/G2oTypes.h:128-145), started at pF1->GetVelocity()
  edge     EdgeVelReproj (include/G2oTypes.h:521-547): Xc = (T exp(v dt) Tbc)^-1 Xw, e = z - project(Xc) with the
           pinhole in double (src/CameraModels/Pinhole.cpp:35-41), no depth test;
           linearizeOplus (src/G2oTypes.cc:497-510): Tcb1 = Tcb exp(-v dt), Xb = T^-1 Xw, Xc = Tcb1 Xb,
           J = -P(Xc) (-Tcb1 CircleDot(Xb) RightJacobianPose3(-v dt) dt)[0:3] (src/Pose3utils.cc:32-34, 75-80);
           information w I_2, Huber delta 5.991 (src/Optimizer.cc:2400-2415)
  graph    only the three sampled edges at level 0, in the order of `indices` (ascending observation index)
  LM       optimize(40): g2o's Levenberg (optimization_algorithm_levenberg.cpp:61-194) as oracle/lba_oracle.c
           restates it for tracking (trk_lm_iteration): lambda = tau max|H_ii| (no user lambda), a failed
           factorisation is a trial with chi2 = DBL_MAX, max_trials, the three-bad-iterations stop, early_stop;
           the linear solve is the oracle's Eigen LDLT (LinearSolverDense)
  scoring  computeError() on every edge, inlier iff ||e||_2 <= threshold in unweighted pixels
           (src/Optimizer.cc:2425-2440); a NaN error is an outlier
  best     the first hypothesis with strictly more inliers than every earlier one, from 0 (src/Tracking.cc:1978-1984)

Conditioning.  Three edges fit six unknowns exactly: chi2 falls to rounding level, the stop rules then fire on
noise, and `iterations` is decided by rounding (not compared anywhere).  Every hypothesis is therefore run twice,
plain and with H and b multiplied entrywise by 1 + 1e-12 N(0, 1) (fixed seed): it is *settled* when both runs
give the same inlier flags and velocities within 1e-8 max(1, |v|_inf); a frame is settled when its best hypothesis
is the same in both runs and is settled.  Only settled hypotheses and frames are compared with the GPU.
"""
import numpy as np

import orc

DBL_MAX = float(np.finfo(np.float64).max)
PERTURB = 1e-12
SETTLED_TOL = 1e-8


def quat_rot(q):
    """Eigen toRotationMatrix of the normalised quaternion (x, y, z, w)."""
    x, y, z, w = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def hat(p):
    return np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])


def se3_exp(xi):
    q, t = orc.se3_exp(xi)
    return quat_rot(q), t


class Rig:
    def __init__(self, cams):
        self.Rbc = [quat_rot(c["q"]) for c in cams]
        self.tbc = [np.array(c["t"], float) for c in cams]
        self.K = [(float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"])) for c in cams]


def project(K, Xc):
    fx, fy, cx, cy = K
    Xc = np.asarray(Xc)
    return np.stack([fx * Xc[..., 0] / Xc[..., 2] + cx, fy * Xc[..., 1] / Xc[..., 2] + cy], axis=-1)


def errors(rig, R, t, v, cam, dt, z, Xw):
    """computeError() of the rows (all of one camera `cam` and one `dt`): [n, 2]."""
    Re, te = se3_exp(np.asarray(v) * dt)
    Rwc = R @ Re @ rig.Rbc[cam]                           # T exp(v dt) Tbc
    twc = R @ (Re @ rig.tbc[cam] + te) + t
    Xc = (np.atleast_2d(Xw) - twc) @ Rwc                  # its inverse on Xw
    return np.atleast_2d(z) - project(rig.K[cam], Xc)


def jacobian(rig, R, t, v, cam, dt, Xw):
    """linearizeOplus(): 2 x 6."""
    dxi = np.asarray(v) * dt
    Rm, tm = se3_exp(-dxi)
    Rcb = rig.Rbc[cam].T
    tcb = -Rcb @ rig.tbc[cam]
    R1, t1 = Rcb @ Rm, Rcb @ tm + tcb                     # Tcb1 = Tcb exp(-dxi)
    Xb = R.T @ (Xw - t)
    Xc = R1 @ Xb + t1
    fx, fy, _, _ = rig.K[cam]
    P = np.array([[fx / Xc[2], 0.0, -fx * Xc[0] / Xc[2] ** 2], [0.0, fy / Xc[2], -fy * Xc[1] / Xc[2] ** 2]])
    circle = np.hstack([np.eye(3), -hat(Xb)])
    deriv = -R1 @ circle @ orc.right_jac_pose3(-dxi) * dt
    return -P @ deriv


def _huber(c, delta):
    d2 = delta * delta
    if c <= d2:
        return c, 1.0
    s = np.sqrt(c)
    return 2 * s * delta - d2, delta / s


def _chi(rig, R, t, v, edges, delta):
    """activeRobustChi2 over the three edges; also the errors and the Huber weights."""
    chi, es, ws = np.float64(0.0), [], []
    for o in edges:
        e = errors(rig, R, t, v, int(o["cam"]), float(o["dt"]), o["z"], o["Xw"])[0]
        c = e[0] * (o["w"] * e[0]) + e[1] * (o["w"] * e[1])
        r0, r1 = _huber(c, delta)
        chi = chi + r0
        es.append(e)
        ws.append(r1 * o["w"])
    return chi, es, ws


def optimize_vel(rig, R, t, v0, edges, tau, max_trials, early_stop, iterations, delta, rng=None):
    """optimize(iterations) on the three level-0 edges; returns (v, LM iterations)."""
    v = np.array(v0, np.float64)
    lam, ni, nbad, iters = 0.0, 2.0, 0, 0
    with np.errstate(all="ignore"):
        for k in range(iterations):
            current, es, ws = _chi(rig, R, t, v, edges, delta)
            ini = current
            H, b = np.zeros((6, 6)), np.zeros(6)
            for o, e, sw in zip(edges, es, ws):
                J = jacobian(rig, R, t, v, int(o["cam"]), float(o["dt"]), o["Xw"])
                H += J.T @ (sw * J)
                b -= J.T @ (sw * e)
            if rng is not None:
                P = 1.0 + PERTURB * rng.standard_normal((6, 6))
                H = H * (np.triu(P) + np.triu(P, 1).T)        # (symmetric)
                b = b * (1.0 + PERTURB * rng.standard_normal(6))
            if k == 0:
                lam, ni, nbad = tau * np.abs(np.diag(H)).max(), 2.0, 0
            rho, qmax = np.float64(0.0), 0
            while True:
                ok, x = orc.ldlt_solve(H + lam * np.eye(6), b)
                vt = v + x if ok else v
                temp = _chi(rig, R, t, vt, edges, delta)[0]
                if not ok:
                    temp = np.float64(DBL_MAX)
                scale = np.float64(1e-3)
                if ok:
                    scale = scale + np.sum(x * (lam * x + b))
                rho = (current - temp) / scale
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current = temp
                    v = vt
                else:
                    lam *= ni
                    ni *= 2
                qmax += 1
                if not (rho < 0 and qmax < max_trials):
                    break
            iters += 1
            stop = qmax == max_trials or rho == 0
            if not stop:
                nbad = nbad + 1 if (ini - current) * 1e3 < ini else 0
                stop = nbad >= 3
            if stop and early_stop:
                break
    return v, iters


def score(rig, R, t, v, obs, threshold):
    """(inlier flags, ||e||) of every observation at the velocity v."""
    norm = np.zeros(len(obs))
    with np.errstate(all="ignore"):
        for cam, dt in sorted(set(zip(obs["cam"].tolist(), obs["dt"].tolist()))):
            rows = np.nonzero((obs["cam"] == cam) & (obs["dt"] == dt))[0]
            e = errors(rig, R, t, v, cam, dt, obs["z"][rows], obs["Xw"][rows])
            norm[rows] = np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2)
        return norm <= threshold, norm


def run_frame(frame, obs, triples, cams, tau=1e-5, max_trials=10, early_stop=1, threshold=2.0, huber_delta=5.991,
              iterations=40, seed=None):
    """One frame's MCRansac with the given triples (frame-local indices).  `obs`: the frame's rows.
    seed: perturb H and b (the second run of the settled rule).  Returns a dict."""
    rig = Rig(cams)
    R, t = quat_rot(frame["q"]), np.array(frame["t"], float)
    rng = np.random.default_rng(seed) if seed is not None else None
    n_hyp = len(triples)
    out = dict(hyp_vel=np.zeros((n_hyp, 6)), hyp_inliers=np.zeros(n_hyp, np.int32), hyp_iterations=np.zeros(n_hyp, np.int32),
               hyp_flags=np.zeros((n_hyp, len(obs)), bool), hyp_norm=np.zeros((n_hyp, len(obs))))
    best, best_n = -1, 0
    for h, tri in enumerate(triples):
        edges = [obs[i] for i in sorted(int(i) for i in tri)]
        v, it = optimize_vel(rig, R, t, frame["vel"], edges, tau, max_trials, early_stop, iterations, huber_delta, rng)
        flags, norm = score(rig, R, t, v, obs, threshold)
        out["hyp_vel"][h], out["hyp_iterations"][h] = v, it
        out["hyp_flags"][h], out["hyp_norm"][h], out["hyp_inliers"][h] = flags, norm, flags.sum()
        if flags.sum() > best_n:
            best, best_n = h, int(flags.sum())
    out["best_hyp"], out["n_inliers"] = best, best_n
    out["vel"] = out["hyp_vel"][best].copy() if best >= 0 else np.array(frame["vel"], float)
    out["inlier"] = out["hyp_flags"][best].astype(np.int32) if best >= 0 else np.zeros(len(obs), np.int32)
    return out


def vel_close(a, b, tol):
    return bool(np.abs(np.asarray(a) - np.asarray(b)).max(initial=0.0) <= tol * max(1.0, np.abs(a).max(initial=0.0)))


def reference(frames, obs, samples, cams, seed=12345, **kw):
    """Per frame: the plain run with `settled` [n_hyp] and `frame_settled` added (the settled rule above)."""
    res = []
    for f, F in enumerate(frames):
        rows = obs[int(F["obs0"]):int(F["obs0"] + F["n_obs"])]
        tri = np.asarray(samples).reshape(-1, 3)[int(F["hyp0"]):int(F["hyp0"] + F["n_hyp"])]
        a = run_frame(F, rows, tri, cams, **kw)
        p = run_frame(F, rows, tri, cams, seed=seed + f, **kw)
        a["settled"] = np.array([bool((a["hyp_flags"][h] == p["hyp_flags"][h]).all()) and
                                 vel_close(a["hyp_vel"][h], p["hyp_vel"][h], SETTLED_TOL) for h in range(len(tri))], bool)
        a["frame_settled"] = a["best_hyp"] == p["best_hyp"] and (a["best_hyp"] < 0 or bool(a["settled"][a["best_hyp"]]))
        a["perturbed"] = p
        res.append(a)
    return res
