// Host build of the product's Sim3Solver maths (lba_s3r_math.hpp: s3r_eig4, s3r_horn, s3r_errors), put together as
// k_s3r_hyp does, for tests/test_sim3_ransac_math_host.py.
#include "../../amc-slam_amd/csrc/lba_s3r_math.hpp"

using namespace lba;

// N[10]: upper triangle, row-major; q[4]: the eigenvector (w, x, y, z) of the largest eigenvalue
extern "C" void s3r_eig(const double* N, double* q, double* lambda) { s3r_eig4(N, q, lambda); }

extern "C" int s3r_sweeps(void) { return S3R_SWEEPS; }

// X1, X2 [3 points][3]; out: q[4] (x, y, z, w), R[9], t[3], s; returns the degenerate flag
extern "C" int s3r_hypothesis(const double* X1, const double* X2, int fix_scale, double* q, double* R, double* t, double* s) {
    S3RHyp H;
    s3r_horn(X1, X2, fix_scale != 0, &H);
    for (int i = 0; i < 4; ++i) q[i] = H.q[i];
    for (int i = 0; i < 9; ++i) R[i] = H.R[i];
    for (int i = 0; i < 3; ++i) t[i] = H.t[i];
    *s = H.s;
    return H.degenerate;
}

// cam = {Tcb q[4], t[3], fx, fy, cx, cy}: err[2] of one row under the hypothesis of (X1, X2)
extern "C" void s3r_row_errors(const double* X1, const double* X2, int fix_scale, const double* cam1, const double* cam2,
                               const double* X1b, const double* X2b, double* err) {
    S3RHyp H;
    s3r_horn(X1, X2, fix_scale != 0, &H);
    CamD c1, c2;
    sim3_cam_derive(cam1, cam1 + 4, cam1[7], cam1[8], cam1[9], cam1[10], &c1);
    sim3_cam_derive(cam2, cam2 + 4, cam2[7], cam2[8], cam2[9], cam2[10], &c2);
    s3r_errors(H, c1, c2, X1b, X2b, err);
}
