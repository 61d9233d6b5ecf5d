// lba_fuse_math.hpp — the search of ORBmatcher::Fuse, both overloads (src/ORBmatcher.cc:1133-1316 and :1318-1437): one
// job's projection through the stored float quaternion (Sophus' SO3::operator*, so3.hpp:358-367) with its frustum,
// distance and viewing gates and PredictScale, one candidate's level, window and chi-square gates, and the decision.
//
// LBA_HD like lba_math.hpp, so tests/test_fuse_host.py runs the code k_fuse runs.  Everything is FLOAT in the
// operation order written here, contraction switched off below (and by -ffp-contract=off where a host compiler builds
// this header), divide and square root correctly rounded.  The two chi-square comparisons widen the float product and
// compare it with the double literal, as `e2 * mvInvLevelSigma2[kpLevel] > 7.8` does.  PredictScale is s3p_level.
// Quirks of the reference that are kept (amc_lba.h has the list): (a) overload 2 skips the last camera; (b) Scw is
// unused; (c) u_right >= 0, zero counts; (d) z == 0 ends OUT_OF_IMAGE; (e) bRight is unused; (f) a point fused in
// camera c goes on to camera c + 1.
// The host-only part (below the device part) is the sequential loop of a whole search.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/amc_lba.h"
#include "lba_match_math.hpp"
#include "lba_s3p_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace lba {

constexpr int FUSE_PENDING = -1;   // a live job's status before its window is walked

struct FuseJob {
    int status;              // a gate's LBA_FUSE_* or FUSE_PENDING
    int level;               // -1 before PredictScale
    float x, y, radius, ur;  // 0 where not reached
};

// the search's cameras: overload 2 stops before the last one
LBA_HD bool fuse_has_camera(int mode, int c, int n_cam) { return mode == LBA_FUSE_KF || c < n_cam - 1; }

// one job up to its window
LBA_HD FuseJob fuse_project(const lba_fuse_cam& C, const lba_s3p_point& P, int mode, int c, int n_cam, float th,
                            float bf, float log_scale_factor, int n_levels, const float* scale_factors) {
    FuseJob J{LBA_FUSE_NO_CAMERA, -1, 0.0f, 0.0f, 0.0f, 0.0f};
    if (!fuse_has_camera(mode, c, n_cam)) return J;   // whatever the point's `skip`: the loop never gets here
    if (P.skip != 0) {
        J.status = LBA_FUSE_SKIPPED;
        return J;
    }
    const float px = P.pos[0], py = P.pos[1], pz = P.pos[2];
    const float qx = C.q_cw[0], qy = C.q_cw[1], qz = C.q_cw[2], qw = C.q_cw[3];
    float ux = qy * pz - qz * py, uy = qz * px - qx * pz, uz = qx * py - qy * px;
    ux += ux; uy += uy; uz += uz;
    const float wx = qy * uz - qz * uy, wy = qz * ux - qx * uz, wz = qx * uy - qy * ux;
    const float X = ((px + qw * ux) + wx) + C.t_cw[0];
    const float Y = ((py + qw * uy) + wy) + C.t_cw[1];
    const float Z = ((pz + qw * uz) + wz) + C.t_cw[2];
    if (Z < 0.0f) {
        J.status = LBA_FUSE_BEHIND;
        return J;
    }
    const float invz = 1.0f / Z;
    const float u = C.fx * X / Z + C.cx;
    const float v = C.fy * Y / Z + C.cy;
    J.x = u;
    J.y = v;
    if (!(u >= C.min_x && u < C.max_x && v >= C.min_y && v < C.max_y)) {
        J.status = LBA_FUSE_OUT_OF_IMAGE;
        return J;
    }
    J.ur = u - bf * invz;
    const float ox = px - C.ow[0], oy = py - C.ow[1], oz = pz - C.ow[2];
    const float dist = sqrtf((ox * ox + oy * oy) + oz * oz);
    if (dist < P.min_dist || dist > P.max_dist) {
        J.status = LBA_FUSE_DIST;
        return J;
    }
    const float dot = (ox * P.normal[0] + oy * P.normal[1]) + oz * P.normal[2];
    if (dot < 0.5f * dist) {
        J.status = LBA_FUSE_ANGLE;
        return J;
    }
    J.level = s3p_level(P.max_distance, dist, log_scale_factor, n_levels);
    J.radius = th * scale_factors[J.level];
    J.status = FUSE_PENDING;
    return J;
}

// one candidate: GetFeaturesInArea's window test, the level gate and, in LBA_FUSE_KF, the chi-square gate.
// `last_cam`: the job's camera is the target's last one.  inv_level_sigma2: the target's.
LBA_HD bool fuse_gate(const FuseJob& J, int mode, bool last_cam, float fx, float fy, int octave, float u_right,
                      const float* inv_level_sigma2) {
    const MatchJobGate G{J.x, J.y, J.radius, 0.0f, J.level - 1, J.level, false, false};
    if (!match_gate(G, fx, fy, octave, u_right)) return false;
    if (mode != LBA_FUSE_KF) return true;
    const float ex = J.x - fx, ey = J.y - fy;
    if (last_cam && u_right >= 0.0f) {
        const float er = J.ur - u_right;
        const float e2 = (ex * ex + ey * ey) + er * er;
        if ((double)(e2 * inv_level_sigma2[octave]) > 7.8) return false;
    } else {
        const float e2 = ex * ex + ey * ey;
        if ((double)(e2 * inv_level_sigma2[octave]) > 5.99) return false;
    }
    return true;
}

// the row of a walked job: n_cand candidates passed the gates, `best` the smallest distance among them and `idx` the
// first feature in walk order that has it
LBA_HD lba_fuse_row fuse_decide(const FuseJob& J, int mode, int n_cand, int best, int idx, int th_low) {
    lba_fuse_row R{LBA_FUSE_NO_CAND, -1, 256, J.level, J.x, J.y, J.radius, n_cand};
    if (n_cand == 0) return R;
    if (mode == LBA_FUSE_KF && best >= 256) {   // 256 < 256 is false: bestIdx stays -1
        R.status = LBA_FUSE_TOO_FAR;
        return R;
    }
    R.feat = idx;
    R.best_dist = best;
    R.status = best <= th_low ? LBA_FUSE_OK : LBA_FUSE_TOO_FAR;
    return R;
}

// the row of a job that failed a gate
LBA_HD lba_fuse_row fuse_gated_row(const FuseJob& J) {
    return lba_fuse_row{J.status, -1, 256, J.level, J.x, J.y, J.radius, 0};
}

// ---------------------------------------------------------------------------------------------------- host only

// a whole search as the reference's loops run it (no argument checks); the arrays are the call's, `rows` the search's
// own n_points * n_cam.  Returns the number of LBA_FUSE_OK rows.
inline int fuse_search(const lba_fuse_target& T, const lba_fuse_cam* fcams, const lba_match_cam* gcams,
                       const float* scale_factors, const float* inv_level_sigma2, const int32_t* cell_start,
                       const int32_t* cell_feat, const lba_match_feat* feats, const lba_fuse_search& S,
                       const lba_s3p_point* points, int th_low, lba_fuse_row* rows) {
    const float* sf = scale_factors + T.sf0;
    const float* sg = inv_level_sigma2 + T.sigma0;
    int n_ok = 0;
    for (int p = 0; p < S.n_points; ++p) {
        const lba_s3p_point& P = points[S.point0 + p];
        for (int c = 0; c < T.n_cam; ++c) {
            const FuseJob J = fuse_project(fcams[T.cam0 + c], P, S.mode, c, T.n_cam, S.th, T.bf, T.log_scale_factor,
                                           T.n_levels, sf);
            lba_fuse_row& R = rows[(size_t)p * T.n_cam + c];
            R = fuse_gated_row(J);
            if (J.status != FUSE_PENDING) continue;
            int n_cand = 0, best = 0x7fffffff, idx = -1;
            MatchRect Q;
            if (match_rect(J.x, J.y, J.radius, gcams[T.cam0 + c], &Q)) {
                const int32_t* cs = cell_start + T.cell0 + (size_t)c * MATCH_CELLS;
                for (int ix = Q.x0; ix <= Q.x1; ++ix)
                    for (int iy = Q.y0; iy <= Q.y1; ++iy)
                        for (int k = cs[ix * MATCH_ROWS + iy]; k < cs[ix * MATCH_ROWS + iy + 1]; ++k) {
                            const int f = cell_feat[T.cf0 + k];
                            const lba_match_feat& Ft = feats[T.feat0 + f];
                            if (!fuse_gate(J, S.mode, c == T.n_cam - 1, Ft.x, Ft.y, Ft.octave, Ft.u_right, sg)) continue;
                            ++n_cand;
                            const int d = match_dist(P.desc, Ft.desc);
                            if (d < best) {
                                best = d;
                                idx = f;
                            }
                        }
            }
            R = fuse_decide(J, S.mode, n_cand, best, idx, th_low);
            n_ok += R.status == LBA_FUSE_OK;
        }
    }
    return n_ok;
}

}  // namespace lba
