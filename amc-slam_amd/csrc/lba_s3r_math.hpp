// lba_s3r_math.hpp — the hypothesis of Sim3Solver::ComputeSim3 (src/Sim3Solver.cc:343-459) in fp64: Horn's closed-form
// absolute orientation of three point pairs, and the two transfers CheckInliers scores a row with (:462-536).
//
// LBA_HD like lba_math.hpp, so tests/test_sim3_ransac_math_host.py runs the code k_s3r_hyp runs.  The 4 x 4 symmetric
// eigenproblem is a cyclic Jacobi with a FIXED number of sweeps: no data-dependent trip count (a NaN input ends like
// any other), and every index is a compile-time constant once the loops are unrolled, so the matrices live in
// registers and the kernel needs no scratch memory.
#pragma once

#include "lba_math.hpp"

namespace lba {

constexpr int S3R_SWEEPS = 6;          // cyclic Jacobi sweeps of the 4 x 4 (the residual they leave)
constexpr double S3R_DEGENERATE = 1e-5;   // |vec| < 1e-5 returns before assigning anything (Sim3Solver.cc:399-400)

// one Jacobi rotation in the (P, Q) plane: A <- G^T A G, V <- V G.  A zero pivot, or a non-finite one, leaves t = 0 or
// NaN and never loops.
template <int P, int Q>
LBA_HD void s3r_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    t = theta < 0.0 ? -t : t;
    t = apq == 0.0 ? 0.0 : t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != P && k != Q) {
            const double akp = A[k][P], akq = A[k][Q];
            A[k][P] = A[P][k] = c * akp - s * akq;
            A[k][Q] = A[Q][k] = s * akp + c * akq;
        }
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// N = [N11 N12 N13 N14 N22 N23 N24 N33 N34 N44] (upper triangle, row-major): the eigenvector of the largest eigenvalue
// (the first of equal ones, as Eigen's maxCoeff), unit length to rounding, and that eigenvalue.
LBA_HD void s3r_eig4(const double* N, double* q, double* lambda) {
    double A[4][4] = {{N[0], N[1], N[2], N[3]}, {N[1], N[4], N[5], N[6]}, {N[2], N[5], N[7], N[8]}, {N[3], N[6], N[8], N[9]}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma unroll
    for (int sweep = 0; sweep < S3R_SWEEPS; ++sweep) {
        s3r_rotate<0, 1>(A, V);
        s3r_rotate<0, 2>(A, V);
        s3r_rotate<0, 3>(A, V);
        s3r_rotate<1, 2>(A, V);
        s3r_rotate<1, 3>(A, V);
        s3r_rotate<2, 3>(A, V);
    }
    double best = A[0][0];
    q[0] = V[0][0]; q[1] = V[1][0]; q[2] = V[2][0]; q[3] = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const bool up = A[k][k] > best;
        best = up ? A[k][k] : best;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = up ? V[i][k] : q[i];
    }
    *lambda = best;
}

// What a hypothesis is scored with: T12 = [s R | t] and T21 = [(1/s) R^T | -(1/s) R^T t] (:440-458)
struct S3RHyp {
    double q[4];           // (x, y, z, w), unit, w >= 0
    double R[9], t[3], s;  // mR12i, mt12i, ms12i
    double sR[9];          // s R
    double iR[9], it[3];   // (1/s) R^T and -(1/s) R^T t
    int degenerate;
};

// X1, X2: the three sampled points of either set, [3 points][3], in the triple's order (the columns of P3Dc1i, P3Dc2i)
LBA_HD void s3r_horn(const double* X1, const double* X2, bool fix_scale, S3RHyp* H) {
    // Step 1: centroids and relative coordinates (ComputeCentroid: rowwise().sum() / cols())
    double O1[3], O2[3], P1[9], P2[9];
    for (int i = 0; i < 3; ++i) {
        O1[i] = ((X1[i] + X1[3 + i]) + X1[6 + i]) / 3.0;
        O2[i] = ((X2[i] + X2[3 + i]) + X2[6 + i]) / 3.0;
        for (int k = 0; k < 3; ++k) {   // P[k * 3 + i]: coordinate i of point k
            P1[k * 3 + i] = X1[k * 3 + i] - O1[i];
            P2[k * 3 + i] = X2[k * 3 + i] - O2[i];
        }
    }
    // Step 2: M = Pr2 Pr1^T, points in the order 0, 1, 2
    double M[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i * 3 + j] = (P2[i] * P1[j] + P2[3 + i] * P1[3 + j]) + P2[6 + i] * P1[6 + j];
    // Step 3: N (:367-381)
    const double N[10] = {M[0] + M[4] + M[8], M[5] - M[7], M[6] - M[2], M[1] - M[3], M[0] - M[4] - M[8],
                          M[1] + M[3],        M[6] + M[2], -M[0] + M[4] - M[8], M[5] + M[7], -M[0] - M[4] + M[8]};
    // Step 4: the eigenvector (w, x, y, z) of the largest eigenvalue
    double e[4], lambda;
    s3r_eig4(N, e, &lambda);
    Quat u = qnormalize(Quat{e[1], e[2], e[3], e[0]});
    if (u.w < 0.0) u = Quat{-u.x, -u.y, -u.z, -u.w};
    H->q[0] = u.x; H->q[1] = u.y; H->q[2] = u.z; H->q[3] = u.w;
    H->degenerate = sqrt(u.x * u.x + u.y * u.y + u.z * u.z) < S3R_DEGENERATE;
    // the rotation by 2 atan2(|vec|, w) about vec (:397-415) is the rotation of the unit quaternion, whatever its sign
    qmat(u, H->R);
    // Steps 5, 6: P3 = R Pr2, s = sum(Pr1 . P3) / sum(P3 . P3), summed point by point (column-major as Eigen's sum())
    double nom = 0.0, den = 0.0;
    for (int k = 0; k < 3; ++k) {
        double P3[3];
        mul33v(H->R, P2 + 3 * k, P3);
        for (int i = 0; i < 3; ++i) {
            nom += P1[3 * k + i] * P3[i];
            den += P3[i] * P3[i];
        }
    }
    H->s = fix_scale ? 1.0 : nom / den;
    // Step 7: t = O1 - s R O2
    double RO[3];
    mul33v(H->R, O2, RO);
    for (int i = 0; i < 3; ++i) H->t[i] = O1[i] - H->s * RO[i];
    // Step 8: T12 and T21
    const double is = 1.0 / H->s;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            H->sR[i * 3 + j] = H->s * H->R[i * 3 + j];
            H->iR[i * 3 + j] = is * H->R[j * 3 + i];
        }
    mul33v(H->iR, H->t, H->it);
    for (int i = 0; i < 3; ++i) H->it[i] = -H->it[i];
}

// pi(Tcb Y): pinhole, no depth test (Pinhole.cpp:43-49); z = 0 gives inf or NaN, which no gate admits
LBA_HD void s3r_project(const CamD& c, const double* Y, double* p) {
    double Xc[3];
    mul33v(c.Rcb, Y, Xc);
    Xc[0] += c.tcb[0]; Xc[1] += c.tcb[1]; Xc[2] += c.tcb[2];
    p[0] = c.fx * Xc[0] / Xc[2] + c.cx;
    p[1] = c.fy * Xc[1] / Xc[2] + c.cy;
}

// CheckInliers for one row (:470-485): err1 = |p11 - p21|^2, err2 = |p12 - p22|^2
LBA_HD void s3r_errors(const S3RHyp& H, const CamD& c1, const CamD& c2, const double* X1b, const double* X2b, double* err) {
    double p11[2], p22[2], p21[2], p12[2], Y[3];
    s3r_project(c1, X1b, p11);
    s3r_project(c2, X2b, p22);
    mul33v(H.sR, X2b, Y);
    Y[0] += H.t[0]; Y[1] += H.t[1]; Y[2] += H.t[2];
    s3r_project(c1, Y, p21);
    mul33v(H.iR, X1b, Y);
    Y[0] += H.it[0]; Y[1] += H.it[1]; Y[2] += H.it[2];
    s3r_project(c2, Y, p12);
    const double a0 = p11[0] - p21[0], a1 = p11[1] - p21[1], b0 = p12[0] - p22[0], b1 = p12[1] - p22[1];
    err[0] = a0 * a0 + a1 * a1;
    err[1] = b0 * b0 + b1 * b1;
}

}  // namespace lba
