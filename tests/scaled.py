"""Scale-aware measures for the windowed LM solver's H, b and damped step (plain numpy, no GPU).

The GPU parity tests compare with max|a - b| / max|b|.  H_pp spans many decades (pose rows near 4e7,
velocity and motion-prior rows five orders below), b's velocity rows are a small fraction of its pose rows and the
landmark steps' median is two orders under their maximum, so that measure holds most entries to 1e-3 relative or
worse and some not at all.  The measures here put every entry in units in which fp64 rounding is about 1e-16:

  scaled_sym   |dH_ij| / sqrt(H_ii H_jj)                  H_pp, and each landmark's 3x3 H_ll
  scaled_rhs   |db_i| / sqrt(H_ii chi2)                   b
  scaled_step  max|D (dx - x)| / max|D x|, D = sqrt(diag(H + lambda I)), against refined_solve's x; a correct
               fp64 solve stays within a small multiple of kappa_scaled(H + lambda I) u

T_LIN and M_STEP are the limits tests/test_gpu_scaled_parity.py holds the kernels to (DESIGN.md section 2 has
the measured values they come from); tests/test_scaled_measures.py checks on the CPU that the measures see what
max-norm misses.
"""
import numpy as np

U = float(np.finfo(np.float64).eps) / 2   # unit roundoff of fp64, 1.1e-16

# Limits of the GPU tests: 8 x the largest value the fp64 path measured over CASES (DESIGN.md section 2,
# profiles/scaled_parity.log), within the conditions T_LIN <= 1e-10 and M_STEP <= 1000.
T_LIN = 8 * 8.275e-14     # largest: gp_small's H_ll (H_pp <= 2.1e-14, b <= 1.8e-15); fp32 residuals give >= 9e-8
M_STEP = 8 * 2.587        # largest: heavy at lambda = 1, landmark part; fp32 residuals give >= 1.1e4

PARITY_LIMIT_H = 1e-9      # the max-norm limits of tests/test_gpu_parity.py, for comparison
PARITY_LIMIT_STEP = 1e-6


def rel(a, b):
    """The measure of the max-norm parity tests: max|a - b| / max|b|."""
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def scaled_sym(H, H_o):
    """max_ij |H_ij - Ho_ij| / sqrt(Ho_ii Ho_jj) for a symmetric positive semi-definite Ho; (n, n), or a stack
    (..., k, k) of blocks each scaled by its own diagonal (the landmarks' (n_lm, 9) H_ll reshaped to 3 x 3).

    Why these units: H = sum_e J_e^T (rho'_e Omega_e) J_e with every edge weight positive semi-definite, so by
    Cauchy-Schwarz sum_e |term_e(i, j)| <= sqrt(H_ii H_jj).  The rounding accumulated in any entry, one whose
    terms cancel included, is therefore bounded by (number of terms) u in these units, whatever the entry's own
    size.  (It does not hold with an indefinite weight, e.g. a Qc with a negative entry.)

    A row with Ho_ii = 0 has every term zero, so H must be exactly zero there (row and column); if it is
    not, the result is inf."""
    H, H_o = np.asarray(H, float), np.asarray(H_o, float)
    assert H.shape == H_o.shape and H.shape[-1] == H.shape[-2]
    d = np.sqrt(np.diagonal(H_o, axis1=-2, axis2=-1))
    s = d[..., :, None] * d[..., None, :]
    diff = np.abs(H - H_o)
    zero = s == 0.0
    if np.any(diff[zero] != 0.0):
        return np.inf
    q = np.divide(diff, s, out=np.zeros_like(diff), where=~zero)
    return float(q.max()) if q.size else 0.0


def scaled_rhs(b, b_o, diagH_o, chi_o):
    """max_i |b_i - bo_i| / sqrt(Ho_ii chi2), chi2 the robust chi2 of Oracle.errors(); diagH_o is H's
    diagonal over b's rows (H_pp's, then each active landmark's H_ll diagonal).

    b_i = -sum_e J_e(:, i)^T (rho'_e Omega_e) e_e, so Cauchy-Schwarz gives sum_e |term_e(i)| <=
    sqrt(H_ii sum_e rho'_e e_e^T Omega_e e_e), and for Huber rho'(s) s <= rho(s), so the second factor is at most
    the robust chi2.  Rows with Ho_ii = 0 must be exactly zero (inf otherwise)."""
    b, b_o, dg = np.asarray(b, float), np.asarray(b_o, float), np.asarray(diagH_o, float)
    assert b.shape == b_o.shape == dg.shape
    s = np.sqrt(dg * chi_o)
    diff = np.abs(b - b_o)
    zero = s == 0.0
    if np.any(diff[zero] != 0.0):
        return np.inf
    q = np.divide(diff, s, out=np.zeros_like(diff), where=~zero)
    return float(q.max()) if q.size else 0.0


def active_landmarks(win):
    """Landmarks with an observation, ascending: landmark block h of b / dx is landmark active[h]."""
    return np.unique(win.obs["lm"])


def full_diag(win, H_o, Hll_o):
    """H's diagonal over b's rows from build_system()'s H_pp and H_ll."""
    act = active_landmarks(win)
    return np.concatenate([np.diag(H_o), np.asarray(Hll_o).reshape(-1, 3, 3)[act][:, (0, 1, 2), (0, 1, 2)].ravel()])


_systems = {}


def system(o, lam, key=None):
    """(A, rhs): the full A = H + lambda I of size (pose_dim + lm_dim)^2 and the right-hand side b of the oracle's
    last build_system(), probed through Oracle.normal_residual r(x) = A x - b with unit vectors: column i =
    r(e_i) - r(0), rhs = -r(0).  Cached per (key, lambda) when a key (the window's name) is given."""
    if key is not None and (key, lam) in _systems:
        return _systems[key, lam]
    n = o.pose_dim + o.lm_dim
    e = np.zeros(n)
    r0 = o.normal_residual(lam, e)
    A = np.empty((n, n))
    # the unit vectors are scaled by a power of two (exact): r(s e_i) = s A e_i - b holds one product per row, and
    # taking -b off again costs u max(s |A_ji|, |b_j|) / s, i.e. an entry far below |b_j| keeps its digits
    s = 2.0 ** 40
    for i in range(n):
        e[i] = s
        A[:, i] = (o.normal_residual(lam, e) - r0) / s
        e[i] = 0.0
    assert np.abs(A - A.T).max() <= 1e-9 * np.abs(A).max()
    A = 0.5 * (A + A.T)
    out = (A, -r0)
    if key is not None:
        _systems[key, lam] = out
    return out


def jacobi(A):
    """D = sqrt(diag(A))."""
    return np.sqrt(np.diag(A))


def kappa_scaled(A):
    """Condition number of the Jacobi-scaled D^-1 A D^-1, D = sqrt(diag(A)) (2-norm, A symmetric positive definite)."""
    D = jacobi(A)
    w = np.linalg.eigvalsh(A / D[:, None] / D[None, :])
    return float(w[-1] / w[0])


def scaled_step(dx, x_ref, D):
    """max|D (dx - x_ref)| / max|D x_ref|."""
    dx, x_ref, D = np.asarray(dx, float), np.asarray(x_ref, float), np.asarray(D, float)
    return float(np.abs(D * (dx - x_ref)).max() / max(np.abs(D * x_ref).max(), 1e-300))


def scaled_step_parts(dx, x_ref, D, pose_dim):
    """scaled_step of (the whole vector, the pose part, the landmark part), each part over its own rows."""
    p = pose_dim
    return (scaled_step(dx, x_ref, D), scaled_step(dx[:p], x_ref[:p], D[:p]), scaled_step(dx[p:], x_ref[p:], D[p:]))


def refined_solve(A, rhs):
    """The high-precision reference: numpy's LU solve and five steps of iterative refinement, the residual
    rhs - A x and the sum x + dx in np.longdouble (x87 extended where the platform has it).  Returns float64."""
    Al = A.astype(np.longdouble)
    rl = rhs.astype(np.longdouble)
    x = np.linalg.solve(A, rhs).astype(np.longdouble)
    for _ in range(5):
        r = rl - Al @ x
        x = x + np.linalg.solve(A, r.astype(np.float64)).astype(np.longdouble)
    return x.astype(np.float64)


def oplus_ref(win, dx):
    """x (+) dx of the window's keyframes and landmarks in np.longdouble, rounded to float64: (q [x y z w], t, vel)
    of every keyframe and the landmarks.  Keyframe block h (the h-th keyframe that is not fixed) holds [upsilon,
    omega, dvel]: T <- T exp(upsilon, omega) with the quaternion normalised on load and after the product, as
    Sophus does; vel += dvel; landmark block h is added to the h-th observed landmark.

    exp's V = I + c1 W + c2 W^2 uses c1 = 2 sin^2(theta / 2) / theta^2 and, below theta = 1e-2, the series of c1 and
    c2: Sophus' (1 - cos theta) / theta^2, which the oracle restates, loses u / theta^2 of c1 to cancellation, i.e.
    u |upsilon| / theta of t, so for small rotation steps the oracle's own apply_step is not a reference at the
    level of a few u."""
    ld = np.longdouble
    kfs = win.kfs
    free = np.nonzero(kfs["fixed"] == 0)[0]
    n_ext = int(np.count_nonzero(win.cams["ext_free"]))
    np_ = 12 * len(free) + 6 * n_ext
    act = active_landmarks(win)
    assert len(dx) == np_ + 3 * len(act)
    q = kfs["q"].astype(ld)
    q /= np.sqrt((q * q).sum(1))[:, None]
    t, vel = kfs["t"].astype(ld), kfs["vel"].astype(ld)
    d = np.asarray(dx[:12 * len(free)], ld).reshape(-1, 12)
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
    vel[free] += d[:, 6:12]
    lm = win.lm.astype(ld)
    lm[act] += np.asarray(dx[np_:], ld).reshape(-1, 3)
    return q.astype(float), t.astype(float), vel.astype(float), lm.astype(float)


def state_deviation(q, t, vel, lm, q_o, t_o, vel_o, lm_o):
    """Deviation of a state from a reference state in units of u: per entry |a - b| / (|b| + max|b|) for t, velocity
    and landmarks, |a - b| for the sign-aligned quaternions."""
    out = {}
    for key, a, b in (("t", t, t_o), ("vel", vel, vel_o), ("lm", lm, lm_o)):
        out[key] = float((np.abs(a - b) / np.maximum(np.abs(b) + np.abs(b).max(), 1e-300)).max() / U)
    sgn = np.sign(np.sum(q * q_o, axis=1, keepdims=True))
    out["q"] = float(np.abs(q * sgn - q_o).max() / U)
    return out


# ------------------------------------------------------------------------------------------------ the cases
def _cases():
    from amc_lba.synth import make_window
    import test_extrinsic
    import test_gpu_parity
    import test_heavy_landmarks

    def parity(name):
        return lambda: make_window(**test_gpu_parity.WINDOWS[name])
    c = {n: parity(n) for n in ("gp_small", "gp_stereo", "mono_only", "two_fixed", "global_shape")}
    # the straight-line window of test_gpu_numerics_edges.py (small-angle branches of the Jacobians)
    c["straight"] = lambda: make_window(n_opt_kf=8, n_lm=400, obs_per_lm=6, n_cam=4, gp=True, seed=11, straight=True)
    c["ext_small"] = lambda: test_extrinsic._ext_win(**test_extrinsic.EXT_WINDOWS["ext_small"])
    # test_heavy_landmarks' spanning window shrunk to 12 keyframes / 300 landmarks: two landmarks viewed from every
    # keyframe through all four cameras, sixteen times each; about a quarter of the views pass the visibility rule,
    # which leaves each with more than 128 observations (segment tiles, k_expand)
    c["heavy"] = lambda: test_heavy_landmarks._spanning(n_opt_kf=11, n_lm=300, n_long=2, seed=9, cams=(0, 1, 2, 3),
                                                        repeat=16)
    return c


CASES = _cases()
# the cases' lambda_init where it is not 1.0 (global BA: 1e-5), known without building the window so that the tests
# can be parametrised by it; reference() checks it against the window
LAMBDA_INIT = {"global_shape": 1e-5}
CASE_LAMBDAS = [(n, lam) for n in CASES for lam in dict.fromkeys((1.0, 1e-3, LAMBDA_INIT.get(n, 1.0)))]
_windows = {}


def window(name):
    """The case's window, built once (read-only: Oracle and Problem copy what they change)."""
    if name not in _windows:
        _windows[name] = CASES[name]()
    return _windows[name]


def lambdas(name):
    """1.0, 1e-3 and the case's lambda_init, without repeats."""
    return [lam for n, lam in CASE_LAMBDAS if n == name]


_refs = {}


def reference(name):
    """Everything the tests need from the oracle on one case, computed once and left unchanged: dict(win, o, chi,
    H, b, Hll, diag, act, and per lambda: A, rhs, D, kappa, x (refined_solve), ok_o, dx_o (the oracle's own LDLT))."""
    if name in _refs:
        return _refs[name]
    import orc
    win = window(name)
    assert win.cfg.get("lambda_init", 1.0) == LAMBDA_INIT.get(name, 1.0)
    o = orc.Oracle(win)
    chi, _, _ = o.errors()
    H, b, Hll = o.build_system()
    r = dict(win=win, o=o, chi=chi, H=H, b=b, Hll=Hll, diag=full_diag(win, H, Hll), act=active_landmarks(win),
             pose_dim=o.pose_dim, lam={})
    for lam in lambdas(name):
        A, rhs = system(o, lam, key=name)
        ok_o, dx_o = o.solve(lam)
        r["lam"][lam] = dict(A=A, rhs=rhs, D=jacobi(A), kappa=kappa_scaled(A), x=refined_solve(A, rhs), ok_o=ok_o,
                             dx_o=dx_o)
    _refs[name] = r
    return r
