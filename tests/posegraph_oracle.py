"""Optimizer::OptimizeEssentialGraph's optimisation restated in numpy / scipy: the checker of lba_posegraph_*
(TEST INFRASTRUCTURE).  Independent of the product: nothing of amc-slam_amd/csrc is used.  It builds on
tests/sim3_oracle.py (Sim3, Sim3(update), oplus).  What is restated, with the reference's lines:

  log      Sim3::log, Thirdparty/g2o/g2o/types/sim3.h:148-230, line for line: the four branches at eps = 1e-5 on |sigma|
           and d = (tr R - 1) / 2, upsilon = W^-1 t (numpy.linalg.solve for W.lu().solve)
  vertex   VertexSim3Expmap (types_seven_dof_expmap.h:48-94): update[6] = 0 under _fix_scale, S <- Sim3(update) S
  edge     EdgeSim3 (:99-126): e = log(C S[v0] S[v1]^-1), information I, no robust kernel
  jac      "numeric": g2o's central differences of 1e-9 through oplus (base_binary_edge.hpp:147-197), a fixed vertex's
           block skipped -- the reference-faithful run;
           "analytic": J0 = Jl^-1(e) Ad(C), J1 = -Jl^-1(e) Ad(E), Jl the top right block of expm([[ad e, I], [0, 0]])
           (scipy), what the device computes by another route
  system   dense H and b over the active free vertices in array order, edge by edge in edge order
  LM       g2o's Levenberg as tests/sim3_oracle._optimize: lambda = user lambda, or tau max|H_ii|, at iteration 0, rho's
           denominator x.(lambda x + b) + 1e-3, the lambda update, max_trials, the three-bad-iterations stop; a failed
           solve (a non-positive pivot of the Cholesky factorisation, as LinearSolverEigen's) is a trial with
           chi2 = DBL_MAX
  activity an edge between two fixed vertices is inactive; a vertex no active edge touches is inactive

Vertices and edges are numpy structured arrays with the fields of lba_pg_vertex / lba_pg_edge.
"""
import numpy as np
import scipy.linalg
import scipy.sparse
import scipy.sparse.linalg

import sim3_oracle as so
from sim3_oracle import DBL_MAX, EPS, Sim3, oplus, skew

PERTURB = 1e-12


def delta_r(R):
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def log_coeffs(S):
    """The branch taken, omega and W of Sim3::log."""
    sigma = np.log(S.s)
    r = S.r / np.sqrt(S.r @ S.r)
    R = so.quat_matrix(r)
    d = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1)
    I = np.eye(3)
    if abs(sigma) < EPS:
        C = 1.0
        if d > 1 - EPS:
            branch = 0
            omega = 0.5 * delta_r(R)
            A, B = 1.0 / 2.0, 1.0 / 6.0
        else:
            branch = 1
            theta = np.arccos(d)
            theta2 = theta * theta
            omega = theta / (2 * np.sqrt(1 - d * d)) * delta_r(R)
            A = (1 - np.cos(theta)) / theta2
            B = (theta - np.sin(theta)) / (theta2 * theta)
    else:
        C = (S.s - 1) / sigma
        if d > 1 - EPS:
            branch = 2
            sigma2 = sigma * sigma
            omega = 0.5 * delta_r(R)
            A = ((sigma - 1) * S.s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma)
        else:
            branch = 3
            theta = np.arccos(d)
            omega = theta / (2 * np.sqrt(1 - d * d)) * delta_r(R)
            theta2 = theta * theta
            a, b = S.s * np.sin(theta), S.s * np.cos(theta)
            c = theta2 + sigma * sigma
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2
    Omega = skew(omega)
    W = A * Omega + B * Omega @ Omega + C * I
    return branch, omega, W, sigma


def sim3_log(S):
    _, omega, W, sigma = log_coeffs(S)
    return np.concatenate([omega, np.linalg.solve(W, S.t), [sigma]])


def Ad(S):
    r = S.r / np.sqrt(S.r @ S.r)
    R = so.quat_matrix(r)
    A = np.zeros((7, 7))
    A[:3, :3] = R
    A[3:6, :3] = skew(S.t) @ R
    A[3:6, 3:6] = S.s * R
    A[3:6, 6] = -S.t
    A[6, 6] = 1.0
    return A


def ad(e):
    A = np.zeros((7, 7))
    A[:3, :3] = skew(e[:3])
    A[3:6, :3] = skew(e[3:6])
    A[3:6, 3:6] = skew(e[:3]) + e[6] * np.eye(3)
    A[3:6, 6] = -e[3:6]
    return A


def left_jac(e):
    M = np.zeros((14, 14))
    M[:7, :7] = ad(e)
    M[:7, 7:] = np.eye(7)
    return scipy.linalg.expm(M)[:7, 7:]


def as_sim3(rec):
    return Sim3(rec["q"], rec["t"], rec["s"])


def edge_error(C, S0, S1):
    return sim3_log(C * S0 * S1.inverse())


def analytic_jac(C, S0, S1, fix_scale):
    E = C * S0 * S1.inverse()
    Ji = np.linalg.inv(left_jac(sim3_log(E)))
    J0, J1 = Ji @ Ad(C), -Ji @ Ad(E)
    if fix_scale:
        J0[:, 6] = 0.0
        J1[:, 6] = 0.0
    return J0, J1


def numeric_jac(C, S0, S1, fix_scale, delta=1e-9, which=(True, True)):
    """base_binary_edge.hpp:147-197: per vertex and dof, (e(oplus(+delta)) - e(oplus(-delta))) / (2 delta)."""
    scalar = 1.0 / (2 * delta)
    out = []
    for side in (0, 1):
        J = np.zeros((7, 7))
        if which[side]:
            add = np.zeros(7)
            for d in range(7):
                add[d] = delta
                P = oplus(S1 if side else S0, add, fix_scale)
                ep = edge_error(C, S0, P) if side else edge_error(C, P, S1)
                add[d] = -delta
                M = oplus(S1 if side else S0, add, fix_scale)
                em = edge_error(C, S0, M) if side else edge_error(C, M, S1)
                add[d] = 0.0
                J[:, d] = scalar * (ep - em)
        out.append(J)
    return out


def activity(v, e):
    """(edge active [n_e], slot [n_v]: index among the active free vertices in array order, or -1)."""
    fixed = np.asarray(v["fixed"]) != 0
    ea = ~(fixed[e["v0"]] & fixed[e["v1"]]) if len(e) else np.zeros(0, bool)
    touched = np.zeros(len(v), bool)
    touched[e["v0"][ea]] = True
    touched[e["v1"][ea]] = True
    free = touched & ~fixed
    slot = np.full(len(v), -1, np.int64)
    slot[free] = np.arange(int(free.sum()))
    return ea, slot


class Graph:
    def __init__(self, v, e, fix_scale):
        self.v, self.e, self.fix = v, e, bool(fix_scale)
        self.active, self.slot = activity(v, e)
        self.na = int((self.slot >= 0).sum())
        self.C = [as_sim3(x) for x in e]

    def states(self, v=None):
        return [as_sim3(x) for x in (self.v if v is None else v)]

    def errors(self, S):
        """[n_e, 7], zero rows for inactive edges."""
        out = np.zeros((len(self.e), 7))
        for k, ed in enumerate(self.e):
            if self.active[k]:
                out[k] = edge_error(self.C[k], S[int(ed["v0"])], S[int(ed["v1"])])
        return out

    def chi2(self, S):
        err = self.errors(S)
        chi = np.float64(0.0)
        for k in range(len(err)):
            chi = chi + err[k] @ err[k]
        return chi

    def build_system(self, S, jac="analytic", sparse=False):
        n = 7 * self.na
        H = scipy.sparse.lil_matrix((n, n)) if sparse else np.zeros((n, n))
        b = np.zeros(n)
        babs = np.zeros(n)        # sum of the terms' magnitudes: the scale of b's rounding error where b cancels to 0
        err = self.errors(S)
        for k, ed in enumerate(self.e):
            if not self.active[k]:
                continue
            i0, i1 = int(ed["v0"]), int(ed["v1"])
            s0, s1 = int(self.slot[i0]), int(self.slot[i1])
            if jac == "numeric":
                J0, J1 = numeric_jac(self.C[k], S[i0], S[i1], self.fix, which=(s0 >= 0, s1 >= 0))
            else:
                J0, J1 = analytic_jac(self.C[k], S[i0], S[i1], self.fix)
            for sa, Ja in ((s0, J0), (s1, J1)):
                if sa < 0:
                    continue
                b[7 * sa:7 * sa + 7] -= Ja.T @ err[k]
                babs[7 * sa:7 * sa + 7] += np.abs(Ja).T @ np.abs(err[k])
                for sb, Jb in ((s0, J0), (s1, J1)):
                    if sb >= 0:
                        H[7 * sa:7 * sa + 7, 7 * sb:7 * sb + 7] += Ja.T @ Jb
        self.b_abs, self.b_scale = babs, float(babs.max()) if n else 0.0
        return H, b, err

    def apply(self, S, dx):
        out = [s.copy() for s in S]
        for i, sl in enumerate(self.slot):
            if sl >= 0:
                out[i] = oplus(S[i], dx[7 * sl:7 * sl + 7], self.fix)
        return out


def solve(H, lam, b):
    """(H + lambda I) x = b by an unpivoted Cholesky factorisation; (False, 0) when a pivot is not positive."""
    try:
        c = scipy.linalg.cho_factor(H + lam * np.eye(len(b)), lower=True)
    except np.linalg.LinAlgError:
        return False, np.zeros(len(b))
    x = scipy.linalg.cho_solve(c, b)
    return bool(np.isfinite(x).all()), x


def solve_sparse(H, lam, b):
    """The same system through scipy's sparse LU (for timing context in scripts/bench_posegraph.py)."""
    A = scipy.sparse.csc_matrix(H) + lam * scipy.sparse.identity(len(b), format="csc")
    return scipy.sparse.linalg.spsolve(A, b)


def step(v, e, fix_scale, lam, jac="analytic"):
    """One damped step: dict(ok, dx [7 na], trial (vertex array), chi2_trial, errors, H, b, na, b_scale, dx_scale)."""
    G = Graph(v, e, fix_scale)
    S = G.states()
    H, b, err = G.build_system(S, jac)
    ok, dx = solve(H, lam, b)
    if ok and G.fix:
        dx[6::7] = 0.0
    St = G.apply(S, dx) if ok else S
    # the step's scale where b cancels (at a minimum dx is the solve of b's rounding error): |H^-1| |terms of b|
    dx_scale = float(np.linalg.norm(np.abs(np.linalg.inv(H + lam * np.eye(len(b)))) @ G.b_abs)) if ok else 0.0
    return dict(ok=ok, dx=dx, trial=pack(v, St), chi2_trial=float(G.chi2(St)), errors=err, H=H, b=b, na=G.na,
                b_scale=G.b_scale, dx_scale=dx_scale)


def pack(v, S):
    out = v.copy()
    for i, s in enumerate(S):
        out[i]["q"], out[i]["t"], out[i]["s"] = s.r, s.t, s.s
    return out


def optimize(v, e, fix_scale=True, iterations=20, lambda_init=1e-16, jac="analytic", tau=1e-5, max_trials=10,
             early_stop=1, seed=None):
    """g2o's Levenberg on the pose graph.  seed: disturb H and b by PERTURB relative.  Returns dict(v (vertex array,
    inactive and fixed vertices as passed), iterations, trials, rejected, solve_failures, chi2_initial, chi2_final,
    lambda_final)."""
    G = Graph(v, e, fix_scale)
    if not G.active.any():
        raise ValueError("no active edge")
    S = G.states()
    rng = np.random.default_rng(seed) if seed is not None else None
    lam, ni, nbad, iters, trials, rejected, failures = 0.0, 2.0, 0, 0, 0, 0, 0
    chi0 = None
    n = 7 * G.na
    with np.errstate(all="ignore"):
        for k in range(iterations):
            current = G.chi2(S)
            if chi0 is None:
                chi0 = float(current)
            ini = current
            H, b, _ = G.build_system(S, jac)
            if rng is not None:
                Pm = 1.0 + PERTURB * rng.standard_normal((n, n))
                H = H * (np.triu(Pm) + np.triu(Pm, 1).T)
                b = b * (1.0 + PERTURB * rng.standard_normal(n))
            if k == 0:
                lam = lambda_init if lambda_init > 0 else tau * np.abs(np.diag(H)).max()
                ni, nbad = 2.0, 0
            rho, qmax = np.float64(0.0), 0
            while True:
                ok, x = solve(H, lam, b)
                if ok and G.fix:
                    x[6::7] = 0.0
                St = G.apply(S, x) if ok else S
                temp = G.chi2(St)
                trials += 1
                if not ok:
                    temp = np.float64(DBL_MAX)
                    failures += 1
                scale = np.float64(1e-3)
                if ok:
                    scale = scale + np.sum(x * (lam * x + b))
                rho = (current - temp) / scale
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current = temp
                    S = St
                else:
                    lam *= ni
                    ni *= 2
                    rejected += 1
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
    return dict(v=pack(v, S), iterations=iters, trials=trials, rejected=rejected, solve_failures=failures,
                chi2_initial=chi0, chi2_final=float(G.chi2(S)), lambda_final=float(lam))


def vertex_gap(a, b):
    """Largest (q up to sign, t, s) gap of two vertex arrays, each relative to max(1, |.|_inf), as
    tests/test_sim3_math_host._gap measures it."""
    worst = 0.0
    for x, y in zip(a, b):
        qa, qb = x["q"] / np.linalg.norm(x["q"]), y["q"] / np.linalg.norm(y["q"])
        gq = min(np.abs(qa - qb).max(), np.abs(qa + qb).max())
        gt = np.abs(x["t"] - y["t"]).max() / max(1.0, np.abs(y["t"]).max())
        gs = abs(x["s"] - y["s"]) / max(1.0, abs(y["s"]))
        worst = max(worst, gq, gt, gs)
    return float(worst)
