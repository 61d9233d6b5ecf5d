// lba_mp_math.hpp — MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:611-700) and
// MapPoint::ComputeDistinctiveDescriptors (:498-578): one observation's step of the normal's sum and of the depth range,
// the position of the lower median, a row's median by bisection on the value (what the kernels run) and the key whose
// minimum is the first row of the least median.
//
// LBA_HD like lba_math.hpp, so tests/test_mp_host.py runs the code the kernels run.  The geometry is FLOAT in the
// operation order written here, contraction switched off below (and by -ffp-contract=off where a host compiler builds
// this header), divide and square root correctly rounded: the form host/lba_map.cpp, amc_lba.triangulate.
// new_point_geometry and lba_fuse_math.hpp's distance already use.  The descriptor's choice is integers throughout.
// Quirks of the reference that are kept (amc_lba.h has the list): (a) the normal counts observations in bad keyframes;
// (b) the lower median, ties to the first row; (c) 0 / 0 on a camera centre; (d) ref_kf == -1 stores FLT_MIN / FLT_MAX.
// The host-only part (below the device part) is the sequential refresh of one point as the reference's loops run it:
// the matrix, std::sort, the first strict minimum.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_match_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace lba {

constexpr int MP_BISECT_STEPS = 9;   // 257 values: 257 -> 129 -> 65 -> 33 -> 17 -> 9 -> 5 -> 3 -> 2 -> 1

// the running state of UpdateNormalAndDepth
struct MpGeom {
    float nx, ny, nz;   // the sum of the unit vectors
    float maxd, mind;   // maxDist, minDist
    int n;
};

LBA_HD MpGeom mp_geom_begin() { return MpGeom{0.0f, 0.0f, 0.0f, FLT_MIN, FLT_MAX, 0}; }

// one observation, in list order.  ow: its camera's centre; is_ref: its keyframe is mpRefKF (the reference's second
// loop forms the same dist from the same Pos and centre); scale: mvScaleFactors[octave] of its keypoint
LBA_HD void mp_geom_add(MpGeom& G, const float* pos, float owx, float owy, float owz, bool is_ref, float scale,
                        float scale_top) {
    const float dx = pos[0] - owx, dy = pos[1] - owy, dz = pos[2] - owz;
    const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
    G.nx = G.nx + dx / r;
    G.ny = G.ny + dy / r;
    G.nz = G.nz + dz / r;
    G.n++;
    if (is_ref) {
        const float a = r * scale;
        const float b = r * scale / scale_top;
        if (G.maxd < a) G.maxd = a;   // std::max(maxDist, a)
        if (b < G.mind) G.mind = b;   // std::min(minDist, b)
    }
}

// mNormalVector = normal / n
LBA_HD void mp_geom_end(const MpGeom& G, float* normal) {
    const float n = (float)G.n;
    normal[0] = G.nx / n;
    normal[1] = G.ny / n;
    normal[2] = G.nz / n;
}

// vDists[0.5 * (N - 1)]: the sorted position of the lower median
LBA_HD int mp_median_pos(int n) { return (int)(0.5 * (n - 1)); }

// The element at sorted position m of a row of n distances in [0, 256]: min { v : #{j : d(j) <= v} >= m + 1 }, by
// bisection on v.  `dist(j)` gives the row's j-th distance and is evaluated MP_BISECT_STEPS * n times.
template <typename Dist>
LBA_HD int mp_row_median(int n, int m, Dist dist) {
    int lo = 0, hi = 256;
    for (int s = 0; s < MP_BISECT_STEPS; ++s) {
        const int mid = (lo + hi) >> 1;
        int count = 0;
        for (int j = 0; j < n; ++j) count += dist(j) <= mid;
        if (count >= m + 1) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the minimum of this key over the rows is the FIRST row of the strictly smallest median (row < 1024, median <= 256)
LBA_HD uint32_t mp_key(int median, int row) { return ((uint32_t)median << 10) | (uint32_t)row; }
LBA_HD int mp_key_row(uint32_t key) { return (int)(key & 1023u); }
LBA_HD int mp_key_median(uint32_t key) { return (int)(key >> 10); }

// ---------------------------------------------------------------------------------------------------- host only

// One point as the reference's two functions run it, no argument checks; the arrays are the call's.  P's five fields
// are overwritten where the reference writes them, its four outputs always.  `bisect`: choose the descriptor with
// mp_row_median as the kernels do, instead of the matrix and std::sort.
inline void mp_refresh_point(lba_mp_point& P, const lba_mp_obs* obs, const lba_tri_kf* kfs, const lba_epi_kf* ekfs,
                             const lba_tri_cam* cams, const lba_epi_feat* feats, const int32_t* kf_bad, float scale_top,
                             bool bisect = false) {
    P.n = 0;
    P.best_obs = P.best_median = -1;
    P.status = P.bad ? LBA_MP_BAD : P.n_obs == 0 ? LBA_MP_EMPTY : LBA_MP_OK;
    if (P.status != LBA_MP_OK) return;
    const lba_mp_obs* L = obs + P.obs0;
    if (P.ops & LBA_MP_DESC) {
        std::vector<int> cand;   // positions in the list
        for (int k = 0; k < P.n_obs; ++k)
            if (!kf_bad || !kf_bad[L[k].kf]) cand.push_back(k);
        const int N = (int)cand.size();
        if (N > 0) {
            auto desc_of = [&](int i) { return feats[ekfs[L[cand[i]].kf].feat0 + L[cand[i]].feat].desc; };
            const int m = mp_median_pos(N);
            int best = 0x7fffffff, best_i = 0;
            if (bisect) {
                for (int i = 0; i < N; ++i) {
                    const uint32_t* di = desc_of(i);
                    const int med = mp_row_median(N, m, [&](int j) { return match_dist(di, desc_of(j)); });
                    if (med < best) {
                        best = med;
                        best_i = i;
                    }
                }
            } else {
                std::vector<int> D((size_t)N * N);
                for (int i = 0; i < N; ++i) {
                    D[(size_t)i * N + i] = 0;
                    for (int j = i + 1; j < N; ++j)
                        D[(size_t)i * N + j] = D[(size_t)j * N + i] = match_dist(desc_of(i), desc_of(j));
                }
                std::vector<int> row((size_t)N);
                for (int i = 0; i < N; ++i) {
                    std::copy(D.begin() + (size_t)i * N, D.begin() + (size_t)(i + 1) * N, row.begin());
                    std::sort(row.begin(), row.end());
                    if (row[(size_t)m] < best) {
                        best = row[(size_t)m];
                        best_i = i;
                    }
                }
            }
            const uint32_t* d = desc_of(best_i);
            for (int k = 0; k < 8; ++k) P.desc[k] = d[k];
            P.best_obs = cand[(size_t)best_i];
            P.best_median = best;
        }
    }
    if (P.ops & LBA_MP_NORMAL) {
        MpGeom G = mp_geom_begin();
        for (int k = 0; k < P.n_obs; ++k) {
            const lba_epi_feat& F = feats[ekfs[L[k].kf].feat0 + L[k].feat];
            const double* Ow = cams[kfs[L[k].kf].cam0 + F.cam].Ow;
            mp_geom_add(G, P.pos, (float)Ow[0], (float)Ow[1], (float)Ow[2], L[k].kf == P.ref_kf, F.scale, scale_top);
        }
        mp_geom_end(G, P.normal);
        P.max_distance = G.maxd;
        P.min_distance = G.mind;
        P.n = G.n;
    }
}

}  // namespace lba
