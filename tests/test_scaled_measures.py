"""The scale-aware measures of tests/scaled.py are sound (CPU, oracle only).

- The reference alone stays inside the bound the GPU step is held to: the oracle's own pivoted-LDLT step against
  refined_solve, in scaled_step, is a small multiple of kappa_s u on every case and lambda.
- The measures see what max|a - b| / max|b| misses: mutations made in numpy on the oracle's own outputs pass the
  max-norm limits of tests/test_gpu_parity.py (1e-9 for H, b, H_ll; 1e-6 for a step) and exceed T_LIN or
  M_STEP kappa_s u at least tenfold.
- Hand-checkable cases of every function.
"""
import numpy as np
import pytest

import orc
import scaled as S
import test_heavy_landmarks

GP_CASES = [n for n in S.CASES if n != "mono_only"]   # (mono_only has no velocity edges: those rows of H, b are zero)

# The reference-alone bound is 4 kappa_s u; measured <= 1.2 on seven cases.  ext_small needs more: the oracle's
# own step is 2.0 (lambda = 1) and 7.1 (1e-3) kappa_s u from refined_solve over the whole vector (its pose part 2.5 and
# 25.9), while the GPU's unpivoted Cholesky on the same system is at 0.32 and 0.07: the
# three weakly observed free extrinsics make the oracle's Schur complement, formed through explicit 3 x 3 inverses
# and solved by a diagonally pivoted LDLT, lose more than the scaled condition number accounts for.
REF_FACTOR = {"ext_small": 16.0}


def _velocity_rows(win):
    nk = int((win.kfs["fixed"] == 0).sum())
    return [np.arange(12 * k + 6, 12 * k + 12) for k in range(nk)]


@pytest.mark.parametrize("name,lam", S.CASE_LAMBDAS)
def test_reference_alone_stays_inside_the_bound(name, lam):
    ref = S.reference(name)
    L = ref["lam"][lam]
    assert L["ok_o"]
    whole, pose, lm = S.scaled_step_parts(L["dx_o"], L["x"], L["D"], ref["pose_dim"])
    ku = L["kappa"] * S.U
    print(f"scaled_parity: ref  {name:12s} lambda {lam:<6g} N {len(L['x'])} kappa_s {L['kappa']:.3e} oracle LDLT vs "
          f"refined_solve, err/(kappa_s u): whole {whole / ku:.3f} pose {pose / ku:.3f} lm {lm / ku:.3f}")
    assert len(L["x"]) <= 2100
    assert whole <= REF_FACTOR.get(name, 4.0) * ku, whole / ku
    # refined_solve itself: its residual, evaluated in long double, is at rounding level of |A| |x| + |b|
    A, x = L["A"].astype(np.longdouble), L["x"].astype(np.longdouble)
    r = np.abs(L["rhs"].astype(np.longdouble) - A @ x).astype(float)
    assert np.all(r <= 2 * S.U * (np.abs(L["A"]) @ np.abs(L["x"]) + np.abs(L["rhs"])))


@pytest.mark.parametrize("name", list(S.CASES))
def test_system_reproduces_build_system(name):
    ref = S.reference(name)
    n = ref["pose_dim"]
    for lam, L in ref["lam"].items():
        assert S.scaled_sym(L["A"][:n, :n] - lam * np.eye(n), ref["H"]) <= 1e-12
        dl = np.diag(L["A"])[n:]
        dl_o = ref["diag"][n:] + lam
        assert np.abs(dl - dl_o).max() <= 1e-12 * dl_o.min() and np.all(np.abs(dl - dl_o) <= 1e-12 * dl_o)
        assert np.array_equal(L["rhs"], ref["b"])
        # the landmark blocks do not couple to each other
        Al = L["A"][n:, n:].reshape(-1, 3, len(dl) // 3, 3)
        off = Al.copy()
        for h in range(len(dl) // 3):
            off[h, :, h, :] = 0.0
        assert not off.any()


def test_cases_are_small_and_heavy_is_heavy():
    for name in S.CASES:
        win = S.window(name)
        assert len(win.kfs) <= 12
    win = S.window("heavy")
    assert len(win.lm) <= 300 and test_heavy_landmarks._heavy_count(win) >= 1
    assert np.bincount(win.obs["lm"]).max() > test_heavy_landmarks.TILE_OBS


# ------------------------------------------------------------------------------------------------ mutations
@pytest.mark.parametrize("name", GP_CASES)
def test_mutation_velocity_block_of_H(name):
    """One velocity-velocity 6 x 6 block of H_pp (the smallest) off by 1e-6 relative."""
    ref = S.reference(name)
    H = ref["H"]
    rows = min(_velocity_rows(ref["win"]), key=lambda r: np.abs(H[np.ix_(r, r)]).max())
    Hm = H.copy()
    Hm[np.ix_(rows, rows)] *= 1.0 + 1e-6
    old, new = S.rel(Hm, H), S.scaled_sym(Hm, H)
    print(f"scaled_parity: mut  {name:12s} velocity block 1e-6: max-norm {old:.2e} scaled_sym {new:.2e}")
    assert old < S.PARITY_LIMIT_H
    assert new >= 10 * S.T_LIN


@pytest.mark.parametrize("name", GP_CASES)
def test_mutation_small_entries_of_H_in_float32(name):
    """The entries of H_pp below 1e-6 max|H| rounded to float32."""
    ref = S.reference(name)
    H = ref["H"]
    small = (np.abs(H) < 1e-6 * np.abs(H).max()) & (H != 0.0)
    assert small.sum() > 0.1 * np.count_nonzero(H)   # (a fifth to a third of the nonzero entries)
    Hm = H.copy()
    Hm[small] = H[small].astype(np.float32)
    old, new = S.rel(Hm, H), S.scaled_sym(Hm, H)
    print(f"scaled_parity: mut  {name:12s} small H in float32 ({small.sum()} entries): max-norm {old:.2e} "
          f"scaled_sym {new:.2e}")
    assert old < S.PARITY_LIMIT_H
    assert new >= 10 * S.T_LIN


@pytest.mark.parametrize("name", GP_CASES)
def test_mutation_velocity_rows_of_b(name):
    """b's velocity rows off by a relative error.

    At 1e-6 the scaled measure is far outside T_LIN, but so is the max-norm one outside its 1e-9: b's velocity
    rows reach 0.7 .. 4 % of its largest entry (|b| max 1.8e5 .. 5.2e5, velocity rows 2.8e3 .. 2.0e4), so max-norm
    lets through a relative error of 2.5e-8 .. 1.3e-7 there, not 1e-6.  The second mutation is the largest one that
    max-norm still passes (half its limit); the scaled measure is still tenfold outside T_LIN."""
    ref = S.reference(name)
    b = ref["b"]
    rows = np.concatenate(_velocity_rows(ref["win"]))
    frac = np.abs(b[rows]).max() / np.abs(b).max()
    for eps in (1e-6, 0.5 * S.PARITY_LIMIT_H / frac):
        bm = b.copy()
        bm[rows] *= 1.0 + eps
        old, new = S.rel(bm, b), S.scaled_rhs(bm, b, ref["diag"], ref["chi"])
        print(f"scaled_parity: mut  {name:12s} b velocity rows {eps:.2e} (rows at {frac:.2e} of max|b|): "
              f"max-norm {old:.2e} scaled_rhs {new:.2e}")
        assert new >= 10 * S.T_LIN
        if eps == 1e-6:
            assert old >= S.PARITY_LIMIT_H   # (max-norm sees this one too)
        else:
            assert old < S.PARITY_LIMIT_H


@pytest.mark.parametrize("name,lam", S.CASE_LAMBDAS)
def test_mutation_small_landmark_steps(name, lam):
    """The steps of the landmarks below the median step off by 1e-6 relative: 566 .. 5.5e5 kappa_s u at lambda = 1
    and 1e-3, i.e. 27 times M_STEP kappa_s u or more.

    At global_shape's lambda_init = 1e-5 the tenfold margin does not exist: kappa_s is 1.3e6, so the limit
    M_STEP kappa_s u is 3.0e-9, while the mutation moves the scaled step by 1e-6 times the small landmarks' share
    of max|D x|, 2.2e-8 = 152 kappa_s u = 7.3 limits.  There the test asks only that the mutation is outside the
    limit; an error of 1e-6 on half the landmarks at that damping is within one decade of what fp64 is allowed."""
    ref = S.reference(name)
    L = ref["lam"][lam]
    n = ref["pose_dim"]
    size = np.abs(L["dx_o"][n:]).reshape(-1, 3).max(axis=1)
    below = np.repeat(size < np.median(size), 3)
    dm = L["dx_o"].copy()
    dm[n:][below] *= 1.0 + 1e-6
    old = S.rel(dm[n:], L["dx_o"][n:])
    _, _, new = S.scaled_step_parts(dm, L["x"], L["D"], n)
    ku = L["kappa"] * S.U
    print(f"scaled_parity: mut  {name:12s} lambda {lam:<6g} small landmark steps 1e-6: max-norm {old:.2e} "
          f"scaled_step {new:.2e} = {new / ku:.0f} kappa_s u")
    assert old <= S.PARITY_LIMIT_STEP
    assert new >= (10 if lam >= 1e-3 else 1) * S.M_STEP * ku


@pytest.mark.parametrize("name", list(S.CASES))
def test_mutation_one_landmark_block_in_float32(name):
    """One landmark's H_ll (the one with the smallest diagonal) rounded to float32."""
    ref = S.reference(name)
    Hll = ref["Hll"].reshape(-1, 3, 3)
    act = ref["act"]
    l = act[np.argmin(Hll[act][:, (0, 1, 2), (0, 1, 2)].max(axis=1))]
    Hm = Hll.copy()
    Hm[l] = Hll[l].astype(np.float32)
    old, new = S.rel(Hm, Hll), S.scaled_sym(Hm, Hll)
    print(f"scaled_parity: mut  {name:12s} H_ll of landmark {l} in float32: max-norm {old:.2e} scaled_sym {new:.2e}")
    assert old < S.PARITY_LIMIT_H
    assert new >= 10 * S.T_LIN


# ------------------------------------------------------------------------------------------------ by hand
def test_scaled_sym_by_hand():
    Ho = np.array([[4.0, 1.0], [1.0, 9.0]])
    assert S.scaled_sym(Ho, Ho) == 0.0
    H = np.array([[4.0, 1.6], [1.6, 9.0]])
    assert S.scaled_sym(H, Ho) == pytest.approx(0.6 / 6.0, rel=1e-15)
    assert S.scaled_sym(np.array([[4.5, 1.0], [1.0, 9.0]]), Ho) == pytest.approx(0.125, rel=1e-15)
    # a zero row of the reference must be exactly zero on the other side
    Hz = np.array([[4.0, 0.0], [0.0, 0.0]])
    assert S.scaled_sym(Hz, Hz) == 0.0
    assert S.scaled_sym(np.array([[4.0, 0.0], [0.0, 1e-300]]), Hz) == np.inf
    assert S.scaled_sym(np.array([[4.0, 1e-300], [1e-300, 0.0]]), Hz) == np.inf
    # a stack of blocks: each scaled by its own diagonal
    st_o = np.stack([Ho, 1e-8 * Ho, np.zeros((2, 2))])
    st = st_o.copy()
    st[1, 0, 1] += 0.6e-8
    assert S.scaled_sym(st, st_o) == pytest.approx(0.1, rel=1e-12)
    assert S.rel(st, st_o) < 1e-9


def test_scaled_rhs_by_hand():
    bo, dg, chi = np.array([3.0, -2.0, 0.0]), np.array([4.0, 1e-4, 0.0]), 25.0
    assert S.scaled_rhs(bo, bo, dg, chi) == 0.0
    assert S.scaled_rhs(np.array([3.5, -2.0, 0.0]), bo, dg, chi) == pytest.approx(0.05, rel=1e-15)
    assert S.scaled_rhs(np.array([3.0, -2.001, 0.0]), bo, dg, chi) == pytest.approx(0.02, rel=1e-9)
    assert S.scaled_rhs(np.array([3.0, -2.0, 1e-300]), bo, dg, chi) == np.inf


def test_kappa_and_scaled_step_by_hand():
    assert S.kappa_scaled(np.diag([1e-6, 1.0, 1e9])) == pytest.approx(1.0, rel=1e-12)
    A = np.array([[4.0, 3.0], [3.0, 9.0]])    # D^-1 A D^-1 = [[1, 1/2], [1/2, 1]]: eigenvalues 1/2 and 3/2
    assert S.kappa_scaled(A) == pytest.approx(3.0, rel=1e-12)
    D, x = S.jacobi(A), np.array([1.0, -1.0])
    assert np.array_equal(D, [2.0, 3.0])
    assert S.scaled_step(x, x, D) == 0.0
    assert S.scaled_step(np.array([1.03, -1.0]), x, D) == pytest.approx(0.06 / 3.0, rel=1e-12)
    w, p, l = S.scaled_step_parts(np.array([1.03, -1.0]), x, D, 1)
    assert (w, l) == (pytest.approx(0.02, rel=1e-12), 0.0) and p == pytest.approx(0.03, rel=1e-12)


def test_refined_solve_beats_the_plain_solve():
    """A Hilbert matrix (kappa 1.5e13 at n = 10) with an exactly representable right-hand side: refined_solve's
    residual, evaluated in long double, is at the rounding of |A| |x|."""
    n = 10
    A = 1.0 / (np.arange(n)[:, None] + np.arange(n)[None, :] + 1.0)
    rhs = np.ones(n)
    x = S.refined_solve(A, rhs)
    r = np.abs(rhs.astype(np.longdouble) - A.astype(np.longdouble) @ x.astype(np.longdouble)).astype(float)
    assert np.all(r <= 2 * S.U * (np.abs(A) @ np.abs(x)))


@pytest.mark.parametrize("name,lam", S.CASE_LAMBDAS)
def test_oplus_ref_agrees_with_the_oracle_up_to_its_cancellation(name, lam):
    """scaled.oplus_ref (long double) against the oracle's apply_step of the oracle's own step: velocities and
    landmarks bitwise, quaternions within 2 u, t within 8 u plus the oracle's cancellation in Sophus' c1 =
    (1 - cos theta) / theta^2: 1 - cos theta carries u, so c1 carries u / theta^2 and t carries u |upsilon| / theta
    (2 u |upsilon| / theta allowed), in the units of state_deviation (|t| + max|t| >= max|t|)."""
    ref = S.reference(name)
    win, dx = ref["win"], ref["lam"][lam]["dx_o"]
    o = orc.Oracle(win)
    o.apply_step(dx)
    kf, lm = o.state()
    q, t, vel, lm_r = S.oplus_ref(win, dx)
    d = S.state_deviation(kf["q"], kf["t"], kf["vel"], lm, q, t, vel, lm_r)
    nf = int((win.kfs["fixed"] == 0).sum())
    xi = dx[:12 * nf].reshape(-1, 12)
    ratio = (np.linalg.norm(xi[:, :3], axis=1) / np.linalg.norm(xi[:, 3:6], axis=1)).max()
    print(f"scaled_parity: opl  {name:12s} lambda {lam:<6g} oracle vs long double in u: t {d['t']:.2f} "
          f"vel {d['vel']:.2f} lm {d['lm']:.2f} q {d['q']:.2f}   max |upsilon| / theta {ratio:.3g}")
    assert np.array_equal(kf["vel"], vel) and np.array_equal(lm, lm_r)
    assert d["q"] <= 2
    assert d["t"] <= 8 + 2 * ratio / np.abs(t).max()
