// lba_tri_math.hpp — one match of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:408-587) in fp64: the parallax
// test, GeometricTools::Triangulate (src/GeometricTools.cc:47-66) or MultiKeyFrame::UnprojectStereo
// (src/KeyFrame.cc:829-846), and the gates behind them.
//
// LBA_HD like lba_math.hpp, so tests/test_tri_math_host.py runs the code k_triangulate runs.  The null vector of the
// 4 x 4 A is a one-sided (Hestenes) Jacobi on its columns with a FIXED number of sweeps: no data-dependent trip count
// (a NaN input ends like any other), and every index is a compile-time constant once the loops are unrolled, so A and
// V live in registers and the kernel needs no scratch memory.  Every comparison is written in the reference's sense,
// so a NaN falls where it falls there.
#pragma once

#include "../../include/amc_lba.h"
#include "lba_math.hpp"

namespace lba {

constexpr int TRI_SWEEPS = 5;   // one-sided Jacobi sweeps of the 4 x 4 (the residual they leave)

// one Hestenes rotation of the columns (P, Q): A <- A G, V <- V G with G chosen so that the two columns of A become
// orthogonal.  A zero pivot (the columns are orthogonal already), or a non-finite one, applies no rotation.
template <int P, int Q>
LBA_HD void tri_rotate(double (&A)[4][4], double (&V)[4][4]) {
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        alpha += A[k][P] * A[k][P];
        beta += A[k][Q] * A[k][Q];
        gamma += A[k][P] * A[k][Q];
    }
    const double zeta = (beta - alpha) / (2.0 * gamma);
    double t = 1.0 / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
    t = zeta < 0.0 ? -t : t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const bool rot = gamma != 0.0 && isfinite(gamma) && isfinite(c) && isfinite(s);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = rot ? c * akp - s * akq : akp;
        A[k][Q] = rot ? s * akp + c * akq : akq;
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = rot ? c * vkp - s * vkq : vkp;
        V[k][Q] = rot ? s * vkp + c * vkq : vkq;
    }
}

// A [4][4] row-major: v[4] is the right singular vector of its smallest singular value, unit length to rounding: V's
// column whose A-column has the smallest norm after the sweeps, the first on ties.  *sigma (may be null) is that norm.
template <int SWEEPS>
LBA_HD void tri_null4_sweeps(const double* A0, double* v, double* sigma) {
    double A[4][4], V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) A[i][j] = A0[4 * i + j];
#pragma unroll
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        tri_rotate<0, 1>(A, V);
        tri_rotate<0, 2>(A, V);
        tri_rotate<0, 3>(A, V);
        tri_rotate<1, 2>(A, V);
        tri_rotate<1, 3>(A, V);
        tri_rotate<2, 3>(A, V);
    }
    double best = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double n2 = ((A[0][k] * A[0][k] + A[1][k] * A[1][k]) + A[2][k] * A[2][k]) + A[3][k] * A[3][k];
        const bool take = k == 0 || n2 < best;
        best = take ? n2 : best;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = take ? V[i][k] : v[i];
    }
    if (sigma) *sigma = sqrt(best);
}

LBA_HD void tri_null4(const double* A, double* v, double* sigma) { tri_null4_sweeps<TRI_SWEEPS>(A, v, sigma); }

// the four rows of A (GeometricTools.cc:50-53): xn = (x, y, 1) of either keypoint, T = Tcw [3][4] row-major
LBA_HD void tri_build_A(const double* xn1, const double* T1, const double* xn2, const double* T2, double* A) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        A[j] = xn1[0] * T1[8 + j] - T1[j];
        A[4 + j] = xn1[1] * T1[8 + j] - T1[4 + j];
        A[8 + j] = xn2[0] * T2[8 + j] - T2[j];
        A[12 + j] = xn2[1] * T2[8 + j] - T2[4 + j];
    }
}

// Triangulate: false when w == 0 (the reference's test) or w is not finite; X = x3Dh.head(3) / w otherwise
LBA_HD bool tri_triangulate(const double* xn1, const double* T1, const double* xn2, const double* T2, double* X) {
    double A[16], v[4];
    tri_build_A(xn1, T1, xn2, T2, A);
    tri_null4(A, v, nullptr);
    const double w = v[3];
    if (w == 0.0 || !isfinite(w)) return false;
    X[0] = v[0] / w; X[1] = v[1] / w; X[2] = v[2] / w;
    return true;
}

// cos(2 atan2(b / 2, depth)) (:446-450) without a transcendental: (d^2 - h^2) / (d^2 + h^2), h = b / 2; atan2(0, 0)
// is 0 or pi, whose doubled cosine is 1
LBA_HD double tri_cos_stereo(double b, double depth) {
    const double h = b / 2.0, d2 = depth * depth, h2 = h * h, den = d2 + h2;
    return den == 0.0 ? 1.0 : (d2 - h2) / den;
}

// UnprojectStereo (KeyFrame.cc:829-846): the RAW keypoint k, the LAST camera's cx, cy, invfx, invfy, the BODY pose
LBA_HD bool tri_unproject_stereo(const double* k, double z, const lba_tri_cam& last, const lba_tri_kf& kf, double* X) {
    if (z > 0.0) {
        const double c[3] = {(k[0] - last.cx) * z * last.invfx, (k[1] - last.cy) * z * last.invfy, z};
        mul33v(kf.Rwb, c, X);
        X[0] += kf.twb[0]; X[1] += kf.twb[1]; X[2] += kf.twb[2];
        return true;
    }
    return false;
}

// the reprojection gate of one side (:497-549): true when the row is dropped.  x, y, z: the point in that camera
LBA_HD bool tri_reproj_fails(const lba_tri_cam& c, double bf, double x, double y, double z, const double* kp, double ur,
                             double sigma2) {
    if (!(ur >= 0.0)) {
        const double ex = (c.fx * x / z + c.cx) - kp[0], ey = (c.fy * y / z + c.cy) - kp[1];
        return (ex * ex + ey * ey) > 5.991 * sigma2;
    }
    const double invz = 1.0 / z;
    const double u = c.fx * x * invz + c.cx, v = c.fy * y * invz + c.cy;
    const double ex = u - kp[0], ey = v - kp[1], er = (u - bf * invz) - ur;
    return (ex * ex + ey * ey + er * er) > 7.8 * sigma2;
}

struct TriRow {   // the inputs of lba_tri_row
    double z1[2], z2[2], k1[2], k2[2], ur1, ur2, depth1, depth2, sigma2_1, sigma2_2, scale1, scale2;
};

// One match.  c1, c2: the cameras of the two keypoints; last1, last2: the last camera of either keyframe.
// Returns LBA_TRI_*; *stereo_point is bPointStereo (set whenever a back-projection was attempted); X is written only
// under LBA_TRI_OK.
LBA_HD int tri_row(const TriRow& r, const lba_tri_cam& c1, const lba_tri_cam& c2, const lba_tri_cam& last1,
                   const lba_tri_cam& last2, const lba_tri_kf& kf1, const lba_tri_kf& kf2, double ratio_factor,
                   int far_points, double th_far, int* stereo_point, double* X) {
    *stereo_point = 0;
    const bool stereo1 = r.ur1 >= 0.0, stereo2 = r.ur2 >= 0.0;
    const double xn1[3] = {(r.z1[0] - c1.cx) / c1.fx, (r.z1[1] - c1.cy) / c1.fy, 1.0};
    const double xn2[3] = {(r.z2[0] - c2.cx) / c2.fx, (r.z2[1] - c2.cy) / c2.fy, 1.0};
    // ray = Rwc xn = Rcw^T xn
    double ray1[3], ray2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ray1[i] = (c1.Tcw[i] * xn1[0] + c1.Tcw[4 + i] * xn1[1]) + c1.Tcw[8 + i] * xn1[2];
        ray2[i] = (c2.Tcw[i] * xn2[0] + c2.Tcw[4 + i] * xn2[1]) + c2.Tcw[8 + i] * xn2[2];
    }
    const double n1 = sqrt((ray1[0] * ray1[0] + ray1[1] * ray1[1]) + ray1[2] * ray1[2]);
    const double n2 = sqrt((ray2[0] * ray2[0] + ray2[1] * ray2[1]) + ray2[2] * ray2[2]);
    const double cos_rays = ((ray1[0] * ray2[0] + ray1[1] * ray2[1]) + ray1[2] * ray2[2]) / (n1 * n2);
    double cos_st1 = cos_rays + 1.0, cos_st2 = cos_rays + 1.0;
    if (stereo1) cos_st1 = tri_cos_stereo(kf1.b, r.depth1);
    else if (stereo2) cos_st2 = tri_cos_stereo(kf2.b, r.depth2);   // the `else if` of :448 is the reference's
    const double cos_st = cos_st2 < cos_st1 ? cos_st2 : cos_st1;  // std::min(cos_st1, cos_st2)
    double P[3];
    if (cos_rays < cos_st && cos_rays > 0.0 && (stereo1 || stereo2 || cos_rays < 0.9998)) {
        if (!tri_triangulate(xn1, c1.Tcw, xn2, c2.Tcw, P)) return LBA_TRI_W_ZERO;
    } else if (stereo1 && cos_st1 < cos_st2) {
        *stereo_point = 1;
        if (!tri_unproject_stereo(r.k1, r.depth1, last1, kf1, P)) return LBA_TRI_NO_DEPTH;
    } else if (stereo2 && cos_st2 < cos_st1) {
        *stereo_point = 1;
        if (!tri_unproject_stereo(r.k2, r.depth2, last2, kf2, P)) return LBA_TRI_NO_DEPTH;
    } else {
        return LBA_TRI_PARALLAX;
    }
    const double* T1 = c1.Tcw;
    const double* T2 = c2.Tcw;
    const double z1 = ((T1[8] * P[0] + T1[9] * P[1]) + T1[10] * P[2]) + T1[11];
    if (z1 <= 0.0) return LBA_TRI_BEHIND1;
    const double z2 = ((T2[8] * P[0] + T2[9] * P[1]) + T2[10] * P[2]) + T2[11];
    if (z2 <= 0.0) return LBA_TRI_BEHIND2;
    const double x1 = ((T1[0] * P[0] + T1[1] * P[1]) + T1[2] * P[2]) + T1[3];
    const double y1 = ((T1[4] * P[0] + T1[5] * P[1]) + T1[6] * P[2]) + T1[7];
    if (tri_reproj_fails(c1, kf1.bf, x1, y1, z1, r.z1, r.ur1, r.sigma2_1)) return LBA_TRI_REPROJ1;
    const double x2 = ((T2[0] * P[0] + T2[1] * P[1]) + T2[2] * P[2]) + T2[3];
    const double y2 = ((T2[4] * P[0] + T2[5] * P[1]) + T2[6] * P[2]) + T2[7];
    if (tri_reproj_fails(c2, kf2.bf, x2, y2, z2, r.z2, r.ur2, r.sigma2_2)) return LBA_TRI_REPROJ2;
    const double a0 = P[0] - c1.Ow[0], a1 = P[1] - c1.Ow[1], a2 = P[2] - c1.Ow[2];
    const double b0 = P[0] - c2.Ow[0], b1 = P[1] - c2.Ow[1], b2 = P[2] - c2.Ow[2];
    const double dist1 = sqrt((a0 * a0 + a1 * a1) + a2 * a2), dist2 = sqrt((b0 * b0 + b1 * b1) + b2 * b2);
    if (dist1 == 0.0 || dist2 == 0.0) return LBA_TRI_DIST_ZERO;
    if (far_points && (dist1 >= th_far || dist2 >= th_far)) return LBA_TRI_FAR;
    const double ratio_dist = dist2 / dist1, ratio_octave = r.scale1 / r.scale2;
    if (ratio_dist * ratio_factor < ratio_octave || ratio_dist > ratio_octave * ratio_factor) return LBA_TRI_SCALE;
    X[0] = P[0]; X[1] = P[1]; X[2] = P[2];
    return LBA_TRI_OK;
}

}  // namespace lba
