// lba_s3p_math.hpp — the geometry in front of the Sim3 ORBmatcher::SearchByProjection (src/ORBmatcher.cc:423-548 and
// :550-685): the per-camera pose chain (Sim3 -> SE3, the GP QueryPose of an asynchronous camera, Tcw[c]) and one job's
// projection with its frustum, distance and viewing gates and MapPoint::PredictScale (src/MapPoint.cc:722-737).
//
// LBA_HD like lba_math.hpp, so tests/test_s3p_host.py runs the code k_s3p_pose and k_s3p_project run.
// The pose chain is fp64 on the float inputs widened (the tracker's convention); Tcw[c] is rounded once to 12 floats.
// Everything from Tcw on is FLOAT in the operation order written here, contraction switched off below (and by
// -ffp-contract=off where a host compiler builds this header), divide and square root correctly rounded (neither hipcc
// nor g++ relaxes them without a fast-math flag, and build.py passes none).  Only PredictScale's logarithm and quotient
// are double, on the float ratio widened, as the reference's `ceil(log(ratio) / mfLogScaleFactor)` promotes them.
// Quirks of the reference that are kept (amc_lba.h has the list): (a) PO and dist use the MAP's camera centre, the
// projection the Sim3-corrected pose; (b) a point goes on to camera c + 1 after it matched in camera c; (c) `skip` is the
// caller's isBad() || spAlreadyFound, built once; (d) z == 0 passes `z < 0` and ends OUT_OF_IMAGE; (e) Ow is never read;
// (f) 0.5 * dist; (g) floor(th_low * ratio) >= 256 is refused; (h) the level of a quotient that is not finite is
// DEFINED here as clamped: NaN -> 0, +inf -> n_levels - 1, -inf -> 0.
// The host-only part (below the device part) is the sequential loop of a whole search.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_match_math.hpp"
#include "lba_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace lba {

constexpr int S3P_PENDING = -1;   // a live job's status before k_s3p_resolve decides it

// ---- the pose chain of one (search, camera), fp64
LBA_HD SE3 s3p_se3(const float* q, const float* t) {
    SE3 T;
    T.q = qnormalize(Quat{(double)q[0], (double)q[1], (double)q[2], (double)q[3]});
    for (int i = 0; i < 3; ++i) T.t[i] = (double)t[i];
    return T;
}

// QueryPose (src/GaussianProcess.cc:5-21) in gp_sample_pose's closed form (lba_math.hpp):
// T(t) = T1 exp(p2 v1 + l1 xi12 + l2 Jr^-1(xi12) v2), xi12 = log(T1^-1 T2)
LBA_HD SE3 s3p_query_pose(const SE3& T1, const SE3& T2, const double* v1, const double* v2, double t1, double t2,
                          double t) {
    double xi12[6], Ji[36], w2[6], xi[6];
    se3_log(se3_mul(se3_inv(T1), T2), xi12);
    right_jac_inv(xi12, Ji);
    matmul(Ji, v2, w2, 6, 6, 1);
    const GPScalars g = gp_scalars(t1, t2, t);
    for (int i = 0; i < 6; ++i) xi[i] = g.p2 * v1[i] + g.l1 * xi12[i] + g.l2 * w2[i];
    return se3_mul(T1, se3_exp(xi));
}

// Tcw[c] of :445-453 as 12 doubles (R row-major, t)
LBA_HD void s3p_pose(const lba_s3p_kf& K, const lba_s3p_cam& C, const float* sq, const float* st, float ss,
                     double* tcw) {
    SE3 Tbw = s3p_se3(sq, st);
    const double s = (double)ss;
    for (int i = 0; i < 3; ++i) Tbw.t[i] = (double)st[i] / s;
    const SE3 Twb = se3_inv(Tbw);
    const SE3 Tcl = se3_mul(s3p_se3(K.q, K.t), se3_inv(s3p_se3(K.q_prev, K.t_prev)));
    const SE3 Twl = se3_mul(Twb, Tcl);
    double v1[6], v2[6];
    for (int i = 0; i < 6; ++i) {
        v1[i] = (double)K.v_prev[i];
        v2[i] = (double)K.v[i];
    }
    const SE3 Twb_c = s3p_query_pose(Twl, Twb, v1, v2, K.stamp_prev, K.stamp, C.stamp);
    const SE3 Tcw = se3_inv(se3_mul(Twb_c, s3p_se3(C.q_bc, C.t_bc)));
    qmat(Tcw.q, tcw);
    tcw[9] = Tcw.t[0]; tcw[10] = Tcw.t[1]; tcw[11] = Tcw.t[2];
}

// ---- one job, float
struct S3pJob {
    int status;          // a gate's LBA_S3P_* or S3P_PENDING
    int level;           // -1 before PredictScale
    float x, y, radius;  // 0 where not reached
};

// (h): the quotient clamped before the conversion
LBA_HD int s3p_level(float max_distance, float dist, float log_scale_factor, int n_levels) {
    const float ratio = max_distance / dist;
    const double q = ceil(log((double)ratio) / (double)log_scale_factor);
    if (!(q > 0.0)) return 0;                        // NaN, -inf, negative, zero
    if (q >= (double)n_levels) return n_levels - 1;  // +inf too
    return (int)q;
}

LBA_HD S3pJob s3p_project(const float* T, const lba_s3p_cam& C, const lba_s3p_point& P, int th, int proj_form,
                          float log_scale_factor, int n_levels, const float* scale_factors) {
    S3pJob J{LBA_S3P_SKIPPED, -1, 0.0f, 0.0f, 0.0f};
    if (P.skip != 0) return J;
    const float px = P.pos[0], py = P.pos[1], pz = P.pos[2];
    const float X = ((T[0] * px + T[1] * py) + T[2] * pz) + T[9];
    const float Y = ((T[3] * px + T[4] * py) + T[5] * pz) + T[10];
    const float Z = ((T[6] * px + T[7] * py) + T[8] * pz) + T[11];
    if (Z < 0.0f) {
        J.status = LBA_S3P_BEHIND;
        return J;
    }
    float u, v;
    if (proj_form == 0) {
        u = C.fx * X / Z + C.cx;
        v = C.fy * Y / Z + C.cy;
    } else {
        const float invz = 1.0f / Z;
        const float xn = X * invz, yn = Y * invz;
        u = C.fx * xn + C.cx;
        v = C.fy * yn + C.cy;
    }
    J.x = u;
    J.y = v;
    if (!(u >= C.min_x && u < C.max_x && v >= C.min_y && v < C.max_y)) {
        J.status = LBA_S3P_OUT_OF_IMAGE;
        return J;
    }
    const float ox = px - C.ow[0], oy = py - C.ow[1], oz = pz - C.ow[2];
    const float dist = sqrtf((ox * ox + oy * oy) + oz * oz);
    if (dist < P.min_dist || dist > P.max_dist) {
        J.status = LBA_S3P_DIST;
        return J;
    }
    const float dot = (ox * P.normal[0] + oy * P.normal[1]) + oz * P.normal[2];
    if (dot < 0.5f * dist) {
        J.status = LBA_S3P_ANGLE;
        return J;
    }
    J.level = s3p_level(P.max_distance, dist, log_scale_factor, n_levels);
    J.radius = (float)th * scale_factors[J.level];
    J.status = S3P_PENDING;
    return J;
}

// the candidate slots of a live job: the features of its cell rectangle (match_capacity's sum on one camera's cells)
LBA_HD int s3p_capacity(float x, float y, float radius, const lba_match_cam& gc, const int32_t* cam_cell_start) {
    MatchRect R;
    if (!match_rect(x, y, radius, gc, &R) || R.y0 > R.y1) return 0;
    int n = 0;
    for (int ix = R.x0; ix <= R.x1; ++ix)
        n += cam_cell_start[ix * MATCH_ROWS + R.y1 + 1] - cam_cell_start[ix * MATCH_ROWS + R.y0];
    return n;
}

// the acceptance test of :538 / :673: an int against a float product
LBA_HD bool s3p_accept(int best_dist, int th_low, float ratio_hamming) {
    const float bound = (float)th_low * ratio_hamming;
    return (float)best_dist <= bound;
}

// a decided scan's status
LBA_HD int s3p_decide(const MatchPick& p, int th_low, float ratio_hamming) {
    if (p.n == 0) return LBA_S3P_NO_CAND;
    return s3p_accept(p.best, th_low, ratio_hamming) ? LBA_S3P_OK : LBA_S3P_TOO_FAR;
}

// ---------------------------------------------------------------------------------------------------- host only

// quirk (g) and the parameters' ranges; nullptr when they are fine
inline const char* s3p_params_error(const lba_s3p_params& P) {
    if (P.th < 0 || P.th_low < 0) return "lba_match_sim3_project: th or th_low negative";
    if (!std::isfinite(P.ratio_hamming) || P.ratio_hamming < 0.0f)
        return "lba_match_sim3_project: ratio_hamming not finite or negative";
    if (s3p_accept(256, P.th_low, P.ratio_hamming))
        return "lba_match_sim3_project: floor(th_low * ratio_hamming) >= 256 (the reference indexes vpMatched[-1])";
    if (P.proj_form != 0 && P.proj_form != 1) return "lba_match_sim3_project: proj_form is neither 0 nor 1";
    return nullptr;
}

// a whole search as the reference's loops run it (no argument checks).  rows [n_points * n_cam], feat_point [n_feat],
// poses [n_cam] (rounds untouched); taken: n_feat bytes or nullptr.  Returns nmatches.
inline int s3p_search_host(const lba_s3p_kf& K, const lba_s3p_cam* kcams, const lba_match_cam* gcams,
                           const float* scale_factors, const int32_t* cell_start, const int32_t* cell_feat,
                           const lba_match_feat* feats, int n_feat, const lba_s3p_search& S,
                           const lba_s3p_point* points, const uint8_t* taken_in, const lba_s3p_params& prm,
                           lba_s3p_row* rows, int32_t* feat_point, lba_s3p_pose* poses) {
    const int n_cam = K.n_cam;
    for (int f = 0; f < n_feat; ++f) feat_point[f] = -1;
    if (!K.has_prev) {
        for (int k = 0; k < S.n_points * n_cam; ++k) rows[k] = lba_s3p_row{LBA_S3P_NO_PREV, -1, 256, -1, 0.f, 0.f, 0.f, 0};
        for (int c = 0; c < n_cam; ++c) {
            for (int i = 0; i < 12; ++i) { poses[c].tcw_d[i] = 0.0; poses[c].tcw[i] = 0.0f; }
        }
        return 0;
    }
    for (int c = 0; c < n_cam; ++c) {
        s3p_pose(K, kcams[c], S.q, S.t, S.s, poses[c].tcw_d);
        for (int i = 0; i < 12; ++i) poses[c].tcw[i] = (float)poses[c].tcw_d[i];
    }
    std::vector<char> taken(n_feat, 0);
    for (int f = 0; taken_in && f < n_feat; ++f) taken[f] = taken_in[f] != 0;
    int nmatches = 0;
    for (int p = 0; p < S.n_points; ++p) {
        const lba_s3p_point& P = points[S.point0 + p];
        for (int c = 0; c < n_cam; ++c) {
            const S3pJob J = s3p_project(poses[c].tcw, kcams[c], P, prm.th, prm.proj_form, K.log_scale_factor,
                                         K.n_levels, scale_factors);
            lba_s3p_row& R = rows[(size_t)p * n_cam + c];
            R = lba_s3p_row{J.status, -1, 256, J.level, J.x, J.y, J.radius, 0};
            if (J.status != S3P_PENDING) continue;
            MatchPick pk;
            MatchRect Q;
            const MatchJobGate G{J.x, J.y, J.radius, 0.0f, J.level - 1, J.level, false, false};
            if (match_rect(J.x, J.y, J.radius, gcams[c], &Q)) {
                const int32_t* cs = cell_start + (size_t)c * MATCH_CELLS;
                for (int ix = Q.x0; ix <= Q.x1; ++ix)
                    for (int iy = Q.y0; iy <= Q.y1; ++iy)
                        for (int k = cs[ix * MATCH_ROWS + iy]; k < cs[ix * MATCH_ROWS + iy + 1]; ++k) {
                            const int f = cell_feat[k];
                            const lba_match_feat& Ft = feats[f];
                            if (!match_gate(G, Ft.x, Ft.y, Ft.octave, Ft.u_right) || taken[f]) continue;
                            match_pick(pk, LBA_MATCH_BEST, match_dist(P.desc, Ft.desc), Ft.octave, f);
                        }
            }
            R.status = s3p_decide(pk, prm.th_low, prm.ratio_hamming);
            R.best_dist = pk.best;
            if (R.status == LBA_S3P_OK) {
                R.feat = pk.idx;
                feat_point[pk.idx] = p;
                taken[pk.idx] = 1;
                ++nmatches;
            }
        }
    }
    return nmatches;
}

}  // namespace lba
