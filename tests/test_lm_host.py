"""What the tracker's four optimisers share (amc-slam_amd/csrc/lba_lm.hpp), built for the host (tests/native/lm_harness.cpp).

The controller (lm_trial, lm_stop) is driven through scripted sequences of (tempChi, scale) by the loop its callers
run, next to a Python restatement of g2o's rule (OptimizationAlgorithmLevenberg::solve and the stop rule of
SparseOptimizer::optimize), and lambda, ni, nbad, rho, currentChi, accept and stop are compared bitwise after every
trial and every iteration.  Equality is exact because both sides are IEEE double arithmetic in the same order, the cube
written t * t * t on both, and the host build (g++ -O2, x86-64 without -march) has no fused multiply-add.

chol_solve<6> and chol_solve<7>: on seeded SPD matrices A^T A + I the relative backward error
|(H + lambda I) x - b|_inf / (|H + lambda I|_inf |x|_inf + |b|_inf) is at most 64 N 2^-53 (an unpivoted Cholesky solve is
backward stable at a small multiple of N u; the bound leaves a factor of a few tens; over these seeds the worst is
0.38 N 2^-53, printed with -s), and it returns 0 for an indefinite matrix, the zero matrix at lambda = 0 and a NaN."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
DBL_MAX = sys.float_info.max


class LmCtl(ctypes.Structure):
    _fields_ = [("lam", ctypes.c_double), ("ni", ctypes.c_double), ("nbad", ctypes.c_int)]


@pytest.fixture(scope="module")
def lm_harness():
    src = os.path.join(ROOT, "tests", "native", "lm_harness.cpp")
    out = os.path.join(ROOT, "tests", "native", "_build", "liblm_harness.so")
    deps = [src] + [os.path.join(ROOT, "amc-slam_amd", "csrc", h) for h in ("lba_lm.hpp", "lba_math.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    L = ctypes.CDLL(out)
    L.lm_trial_c.argtypes = [ctypes.POINTER(LmCtl), _dp, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_int)]
    L.lm_trial_c.restype = ctypes.c_double
    L.lm_stop_c.argtypes = [ctypes.POINTER(LmCtl)] + [ctypes.c_double] * 3 + [ctypes.c_int] * 2
    L.lm_stop_c.restype = ctypes.c_int
    for f in (L.chol_solve6, L.chol_solve7):
        f.argtypes = [_dp, ctypes.c_double, _dp, _dp]
        f.restype = ctypes.c_int
    return L


def _bits(x):
    return struct.pack("<d", float(x))


class RefCtl:
    """g2o's rule restated (optimization_algorithm_levenberg.cpp:61-194, sparse_optimizer.cpp's optimize)."""

    def __init__(self, lam):
        self.lam, self.ni, self.nbad = np.float64(lam), np.float64(2.0), 0

    def trial(self, current, temp, scale):
        """-> rho, accept, the new currentChi"""
        with np.errstate(all="ignore"):
            rho = (np.float64(current) - np.float64(temp)) / np.float64(scale)
            if rho > 0 and np.isfinite(temp):
                t = 2 * rho - 1
                alpha = 1. - t * t * t
                alpha = min(alpha, np.float64(2.) / 3.)
                self.lam = self.lam * max(np.float64(1.) / 3., alpha)
                self.ni = np.float64(2.0)
                return rho, True, np.float64(temp)
            self.lam = self.lam * self.ni
            self.ni = self.ni * 2
            return rho, False, np.float64(current)

    def stop(self, ini, current, rho, qmax, max_trials):
        stop = qmax == max_trials or rho == 0
        if not stop:
            if (np.float64(ini) - np.float64(current)) * 1e3 < ini:
                self.nbad += 1
            else:
                self.nbad = 0
            stop = self.nbad >= 3
        return bool(stop)


def _drive(L, chi0, lam0, max_trials, iterations):
    """The callers' loop over scripted iterations (each a list of (tempChi, scale)); bitwise comparison throughout.
    -> per iteration (accepted trials' indices, qmax, stop)."""
    c, ref = LmCtl(lam0, 2.0, 0), RefCtl(lam0)
    cur, r_cur = ctypes.c_double(chi0), np.float64(chi0)
    log = []
    for trials in iterations:
        ini, r_ini = cur.value, r_cur
        qmax, accepted = 0, []
        while True:
            temp, scale = trials[qmax]          # (a script too short for the rule is a mistake in the test)
            acc = ctypes.c_int(-1)
            rho = L.lm_trial_c(ctypes.byref(c), ctypes.byref(cur), temp, scale, ctypes.byref(acc))
            r_rho, r_acc, r_cur = ref.trial(r_cur, temp, scale)
            assert _bits(rho) == _bits(r_rho) and acc.value == int(r_acc)
            assert _bits(c.lam) == _bits(ref.lam) and _bits(c.ni) == _bits(ref.ni) and c.nbad == ref.nbad
            assert _bits(cur.value) == _bits(r_cur)
            if acc.value:
                accepted.append(qmax)
            qmax += 1
            if not (rho < 0 and qmax < max_trials):
                break
        stop = L.lm_stop_c(ctypes.byref(c), ini, cur.value, rho, qmax, max_trials)
        assert stop == int(ref.stop(r_ini, r_cur, r_rho, qmax, max_trials)) and c.nbad == ref.nbad
        log.append((accepted, qmax, bool(stop)))
        if stop:
            break
    return log, c, cur.value


def test_acceptance_over_the_clamp(lm_harness):
    # rho = 0.05 .. 3: alpha above 2/3 (clamped), inside (1/3, 2/3), below 1/3 (clamped); each its own run of one trial
    seen = set()
    for rho_want in (0.05, 0.2, 0.25, 0.5, 0.6, 0.8, 0.9, 1.0, 3.0, 1e9):
        log, c, cur = _drive(lm_harness, 100.0, 0.7, 10, [[(100.0 - 7.0 * rho_want, 7.0)]])
        assert log == [([0], 1, False)] and cur == 100.0 - 7.0 * rho_want and c.ni == 2.0 and c.nbad == 0
        lo, hi = 0.7 * (1. / 3.), 0.7 * (2. / 3.)
        assert lo <= c.lam <= hi
        seen.add("hi" if c.lam == hi else "lo" if c.lam == lo else "mid")
    assert seen == {"hi", "mid", "lo"}


def test_rejection_until_max_trials(lm_harness):
    for max_trials in (1, 3, 10):
        log, c, cur = _drive(lm_harness, 50.0, 1e-4, max_trials, [[(60.0 + i, 2.0) for i in range(max_trials)], [(1.0, 1.0)]])
        assert log == [([], max_trials, True)] and cur == 50.0         # the trials ran out: stop, state untouched
        assert c.lam == 1e-4 * 2.0 ** (max_trials * (max_trials + 1) // 2) and c.ni == 2.0 ** (max_trials + 1)


def test_rejections_then_acceptance_resets_ni(lm_harness):
    log, c, cur = _drive(lm_harness, 50.0, 1e-4, 10, [[(60.0, 2.0), (55.0, 1.0), (40.0, 20.0)], [(39.0, 3.0)]])
    assert log == [([2], 3, False), ([0], 1, False)] and cur == 39.0 and c.ni == 2.0 and c.nbad == 0


def test_rho_exactly_zero_stops(lm_harness):
    log, c, cur = _drive(lm_harness, 8.0, 0.5, 10, [[(8.0, 3.0)], [(1.0, 1.0)]])
    assert log == [([], 1, True)] and cur == 8.0 and c.lam == 1.0 and c.ni == 4.0   # refused (rho > 0 fails), no retry


def test_failed_solve_dbl_max_and_infinities(lm_harness):
    # tempChi = DBL_MAX (a failed factorisation: scale stays 1e-3): rho = -inf, refused, the next trial decides
    log, c, cur = _drive(lm_harness, 8.0, 0.5, 10, [[(DBL_MAX, 1e-3), (DBL_MAX, 1e-3), (6.0, 4.0)]])
    assert log == [([2], 3, False)] and cur == 6.0
    # an infinite tempChi over a negative scale has rho = +inf > 0 and is still refused; rho < 0 fails, so no retry
    log, c, cur = _drive(lm_harness, 8.0, 0.5, 10, [[(float("inf"), -1.0)]])
    assert log == [([], 1, False)] and cur == 8.0 and c.lam == 1.0 and c.nbad == 1
    # a positive gain over a negative scale: rho < 0, refused and retried
    log, c, cur = _drive(lm_harness, 8.0, 0.5, 2, [[(6.0, -1.0), (6.0, -1.0)]])
    assert log == [([], 2, True)] and cur == 8.0


def test_nan_temp_chi_is_refused_without_retry(lm_harness):
    nan = float("nan")
    log, c, cur = _drive(lm_harness, 8.0, 0.5, 10, [[(nan, 1.0)], [(nan, 1.0)], [(nan, 1.0)], [(1.0, 1.0)]])
    # rho is NaN: neither > 0 nor < 0 nor == 0; each iteration is one refused trial with no gain, the third stops
    assert log == [([], 1, False), ([], 1, False), ([], 1, True)] and cur == 8.0
    assert c.nbad == 3 and c.lam == 0.5 * 2 * 4 * 8 and c.ni == 16.0


def test_three_small_gains_in_a_row_stop(lm_harness):
    small = lambda x: x * (1 - 5e-4)     # noqa: E731  (a gain of 5e-4 of iniChi, below 1e-3)
    big = lambda x: x * 0.5              # noqa: E731
    c0 = 1000.0
    c1, c2 = small(c0), small(small(c0))
    c3 = big(c2)                          # a good iteration in between resets the count
    c4, c5, c6 = small(c3), small(small(c3)), small(small(small(c3)))
    chis = [c1, c2, c3, c4, c5, c6, small(c6)]
    log, c, cur = _drive(lm_harness, c0, 1e-3, 10, [[(x, 1.0)] for x in chis])
    assert [s for _, _, s in log] == [False, False, False, False, False, True] and cur == c6 and c.nbad == 3
    # the boundary: a gain of exactly 1e-3 iniChi counts as good ((ini - cur) * 1e3 < ini is false)
    log, c, cur = _drive(lm_harness, 1000.0, 1e-3, 10, [[(999.0, 1.0)]])
    assert c.nbad == 0
    log, c, cur = _drive(lm_harness, 1000.0, 1e-3, 10, [[(999.0 + 2.0 ** -40, 1.0)]])
    assert c.nbad == 1


def _packed(M):
    n = M.shape[0]
    return np.array([M[i, j] for i in range(n) for j in range(i, n)], float)


def _solve(L, n, M, lam, b):
    x = np.full(n, np.nan)
    f = L.chol_solve6 if n == 6 else L.chol_solve7
    Hp, b = _packed(M), np.ascontiguousarray(b, float)
    ok = f(Hp.ctypes.data_as(_dp), lam, b.ctypes.data_as(_dp), x.ctypes.data_as(_dp))
    return ok, x


@pytest.mark.parametrize("n", [6, 7])
def test_chol_solve_backward_error(lm_harness, n):
    bound = 64 * n * 2.0 ** -53
    worst = 0.0
    for seed in range(40):
        rng = np.random.default_rng(1000 * n + seed)
        A = rng.standard_normal((n, n)) * 10.0 ** rng.uniform(-2, 2)
        H = A.T @ A + np.eye(n)
        H = (H + H.T) / 2
        b = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3)
        for lam in (0.0, 1e-5 * np.abs(np.diag(H)).max(), 10.0):
            ok, x = _solve(lm_harness, n, H, lam, b)
            assert ok == 1
            # the residual in extended precision, so that its own rounding does not count
            K = (H + lam * np.eye(n)).astype(np.longdouble)
            r = np.abs(K @ x.astype(np.longdouble) - b.astype(np.longdouble)).max()
            eta = float(r / (np.abs(K).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))
            worst = max(worst, eta)
    print(f"chol_solve<{n}>: worst backward error {worst:.3e} = {worst / (n * 2.0 ** -53):.2f} N u, bound {bound:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("n", [6, 7])
def test_chol_solve_refuses(lm_harness, n):
    b = np.ones(n)
    indefinite = np.eye(n)
    indefinite[n - 2, n - 2] = -1.0
    assert _solve(lm_harness, n, indefinite, 0.0, b)[0] == 0
    assert _solve(lm_harness, n, indefinite, 0.5, b)[0] == 0
    assert _solve(lm_harness, n, indefinite, 1.5, b)[0] == 1          # (the damping makes it positive)
    rank1 = np.ones((n, n))                                            # semi-definite: the second pivot is 0
    assert _solve(lm_harness, n, rank1, 0.0, b)[0] == 0
    assert _solve(lm_harness, n, np.zeros((n, n)), 0.0, b)[0] == 0
    assert _solve(lm_harness, n, np.zeros((n, n)), 1.0, b)[0] == 1
    for where in ((0, 0), (1, 3), (n - 1, n - 1)):
        M = 2.0 * np.eye(n)
        M[where] = np.nan
        assert _solve(lm_harness, n, M, 0.0, b)[0] == 0
    assert _solve(lm_harness, n, 2.0 * np.eye(n), float("nan"), b)[0] == 0
