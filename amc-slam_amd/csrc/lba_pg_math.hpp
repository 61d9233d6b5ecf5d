// lba_pg_math.hpp — the maths of the Sim3 pose graph (Optimizer::OptimizeEssentialGraph, lba_posegraph.hip): g2o's
// Sim3::log, the adjoint, and g2o::EdgeSim3 with its analytic Jacobians.  Built for the device and for the host
// (tests/native/posegraph_harness.cpp).
//
// Tangent order [omega; upsilon; sigma] (sim3.h:70-142), left update S <- Sim3(update) S.  With E = C S0 S1^-1 and
// e = log E:
//   C exp(d) S0 S1^-1 = exp(Ad(C) d) E            ->  J0 =  Jl^-1(e) Ad(C)
//   C S0 (exp(d) S1)^-1 = exp(-Ad(E) d) E         ->  J1 = -Jl^-1(e) Ad(E)
//   Ad(S) = [[R, 0, 0], [[t]x R, s R, -t], [0, 0, 1]],  ad(e) = [[[w]x, 0, 0], [[u]x, [w]x + sigma I, -u], [0, 0, 0]]
// Jl(e) = sum_n ad(e)^n / (n + 1)! is the left Jacobian.  It is summed where it converges fast: ad(e) is halved until
// its row-sum norm is <= 1/4, Jl and exp are summed there (14 terms, remainder below 1e-17), and the halvings are
// undone with Jl(2x) = 1/2 (I + exp(ad x)) Jl(x), exp(ad 2x) = exp(ad x)^2.  Jl is then inverted by a 7 x 7 LU with
// partial pivoting.
#pragma once

#include "lba_math.hpp"

namespace lba {

// x = A^-1 b for 3 x 3 A (row-major), Gaussian elimination with partial pivoting (sim3.h:217: W.lu().solve(t))
LBA_HD void solve33(const double* A, const double* b, double* x) {
    double M[3][4];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) M[i][j] = A[i * 3 + j];
        M[i][3] = b[i];
    }
    for (int k = 0; k < 3; ++k) {
        int p = k;
        double best = fabs(M[k][k]);
        for (int i = k + 1; i < 3; ++i)
            if (fabs(M[i][k]) > best) { best = fabs(M[i][k]); p = i; }
        if (p != k)
            for (int j = 0; j < 4; ++j) { const double s = M[k][j]; M[k][j] = M[p][j]; M[p][j] = s; }
        for (int i = k + 1; i < 3; ++i) {
            const double f = M[i][k] / M[k][k];
            for (int j = k; j < 4; ++j) M[i][j] -= f * M[k][j];
        }
    }
    for (int i = 2; i >= 0; --i) {
        double s = M[i][3];
        for (int j = i + 1; j < 3; ++j) s -= M[i][j] * x[j];
        x[i] = s / M[i][i];
    }
}

// Sim3::log (sim3.h:148-230): the four branches at eps = 1e-5 on |sigma| and on d = (tr R - 1) / 2; in the two
// branches with d > 1 - eps omega = deltaR(R) / 2; in the two with |sigma| < eps W ignores sigma (C = 1)
LBA_HD void sim3_log(const Sim3& S, double* e) {
    const double sigma = log(S.s);
    double R[9];
    qmat(S.q, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double eps = 0.00001;
    double A, B, C, k;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
            k = 0.5;
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = acos(d), theta2 = theta * theta;
            k = theta / (2 * sqrt(1 - d * d));
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            k = 0.5;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d), theta2 = theta * theta;
            k = theta / (2 * sqrt(1 - d * d));
            const double a = S.s * sin(theta), b = S.s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    for (int i = 0; i < 3; ++i) e[i] = k * dR[i];
    double Om[9], Om2[9], W[9];
    hat3(e, Om);
    mul33(Om, Om, Om2);
    for (int i = 0; i < 9; ++i) W[i] = A * Om[i] + B * Om2[i] + (i % 4 == 0 ? C : 0.0);
    solve33(W, S.t, e + 3);
    e[6] = sigma;
}

// Ad(S), 7 x 7 row-major
LBA_HD void sim3_Ad(const Sim3& S, double* A) {
    double R[9], T[9], TR[9];
    qmat(S.q, R);
    hat3(S.t, T);
    mul33(T, R, TR);
    for (int i = 0; i < 49; ++i) A[i] = 0.0;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            A[i * 7 + j] = R[i * 3 + j];
            A[(3 + i) * 7 + j] = TR[i * 3 + j];
            A[(3 + i) * 7 + 3 + j] = S.s * R[i * 3 + j];
        }
        A[(3 + i) * 7 + 6] = -S.t[i];
    }
    A[48] = 1.0;
}

// ad(e), 7 x 7 row-major
LBA_HD void sim3_ad(const double* e, double* A) {
    double Wx[9], Ux[9];
    hat3(e, Wx);
    hat3(e + 3, Ux);
    for (int i = 0; i < 49; ++i) A[i] = 0.0;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            A[i * 7 + j] = Wx[i * 3 + j];
            A[(3 + i) * 7 + j] = Ux[i * 3 + j];
            A[(3 + i) * 7 + 3 + j] = Wx[i * 3 + j] + (i == j ? e[6] : 0.0);
        }
        A[(3 + i) * 7 + 6] = -e[3 + i];
    }
}

LBA_HD void mul77(const double* A, const double* B, double* C) {
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) {
            double s = 0.0;
            for (int l = 0; l < 7; ++l) s += A[i * 7 + l] * B[l * 7 + j];
            C[i * 7 + j] = s;
        }
}

// the left Jacobian Jl(e) of Sim3, 7 x 7 row-major (see the head of this file)
LBA_HD void sim3_left_jac(const double* e, double* J) {
    double X[49], P[49], Ex[49], T[49];
    sim3_ad(e, X);
    double norm = 0.0;
    for (int i = 0; i < 7; ++i) {
        double r = 0.0;
        for (int j = 0; j < 7; ++j) r += fabs(X[i * 7 + j]);
        norm = fmax(norm, r);
    }
    int m = 0;
    while (norm > 0.25 && m < 60) {   // (a NaN norm ends the loop at once, an infinite one at 60)
        norm *= 0.5;
        ++m;
    }
    const double scale = ldexp(1.0, -m);
    for (int i = 0; i < 49; ++i) X[i] *= scale;
    // J = sum_n X^n / (n + 1)!,  Ex = sum_n X^n / n!
    for (int i = 0; i < 49; ++i) {
        const double id = i % 8 == 0 ? 1.0 : 0.0;
        J[i] = id; Ex[i] = id; P[i] = id;
    }
    for (int n = 1; n <= 14; ++n) {
        mul77(P, X, T);
        const double inv = 1.0 / n;
        for (int i = 0; i < 49; ++i) {
            P[i] = T[i] * inv;             // X^n / n!
            Ex[i] += P[i];
            J[i] += P[i] / (n + 1);
        }
    }
    for (int k = 0; k < m; ++k) {
        for (int i = 0; i < 49; ++i) P[i] = 0.5 * (Ex[i] + (i % 8 == 0 ? 1.0 : 0.0));
        mul77(P, J, T);
        for (int i = 0; i < 49; ++i) J[i] = T[i];
        mul77(Ex, Ex, T);
        for (int i = 0; i < 49; ++i) Ex[i] = T[i];
    }
}

// X = A^-1 B for 7 x 7 A and B (row-major; A is destroyed), LU with partial pivoting
LBA_HD void solve77(double* A, const double* B, double* X) {
    for (int i = 0; i < 49; ++i) X[i] = B[i];
    for (int k = 0; k < 7; ++k) {
        int p = k;
        double best = fabs(A[k * 7 + k]);
        for (int i = k + 1; i < 7; ++i)
            if (fabs(A[i * 7 + k]) > best) { best = fabs(A[i * 7 + k]); p = i; }
        if (p != k)
            for (int j = 0; j < 7; ++j) {
                double s = A[k * 7 + j]; A[k * 7 + j] = A[p * 7 + j]; A[p * 7 + j] = s;
                s = X[k * 7 + j]; X[k * 7 + j] = X[p * 7 + j]; X[p * 7 + j] = s;
            }
        const double piv = A[k * 7 + k];
        for (int i = k + 1; i < 7; ++i) {
            const double f = A[i * 7 + k] / piv;
            for (int j = k; j < 7; ++j) A[i * 7 + j] -= f * A[k * 7 + j];
            for (int j = 0; j < 7; ++j) X[i * 7 + j] -= f * X[k * 7 + j];
        }
    }
    for (int i = 6; i >= 0; --i)
        for (int j = 0; j < 7; ++j) {
            double s = X[i * 7 + j];
            for (int l = i + 1; l < 7; ++l) s -= A[i * 7 + l] * X[l * 7 + j];
            X[i * 7 + j] = s / A[i * 7 + i];
        }
}

// g2o::EdgeSim3 (types_seven_dof_expmap.h:99-126): e = log(C S0 S1^-1).  J0, J1 (7 x 7 row-major, d e / d update of
// either vertex) may both be NULL; under fix_scale their column 6 is zero (the vertex zeroes update[6])
LBA_HD void sim3_pg_edge(const Sim3& C, const Sim3& S0, const Sim3& S1, bool fix_scale, double* e, double* J0, double* J1) {
    const Sim3 E = sim3_mul(C, sim3_mul(S0, sim3_inv(S1)));
    sim3_log(E, e);
    if (!J0) return;
    double Jl[49], A[49];
    sim3_left_jac(e, Jl);
    sim3_Ad(C, A);
    double Jc[49];
    for (int i = 0; i < 49; ++i) Jc[i] = Jl[i];
    solve77(Jc, A, J0);
    sim3_Ad(E, A);
    solve77(Jl, A, J1);
    for (int i = 0; i < 49; ++i) J1[i] = -J1[i];
    if (fix_scale)
        for (int i = 0; i < 7; ++i) { J0[i * 7 + 6] = 0.0; J1[i * 7 + 6] = 0.0; }
}

}  // namespace lba
