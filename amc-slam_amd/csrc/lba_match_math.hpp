// lba_match_math.hpp — one job of ORBmatcher's projection searches (src/ORBmatcher.cc:43-217 and :1439-1568):
// MultiFrame::GetFeaturesInArea's cell rectangle and gates (src/Frame.cc:608-673), the stereo gate, DescriptorDistance
// (:1743-1759), the best / second-best scan with its acceptance rule, and the rotation histogram with
// ComputeThreeMaxima (:1697-1738).
//
// LBA_HD like lba_math.hpp, so tests/test_match_host.py runs the code k_match_gather and k_match_resolve run.  Every
// floating-point expression that decides something is one to three IEEE single operations with no sum after a
// product; they are written in FLOAT in the reference's order and contraction is switched off below (and by
// -ffp-contract=off where a host compiler builds this header), so each decision is the reference's own bits.
// Everything else is integer work.  The host-only part (below the device part) is the sequential loop: the capacity
// of a job's candidate list, which lba_match_project uses, and a whole search resolved in job order, which the tests
// and scripts/bench_match.py use.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace lba {

constexpr int MATCH_COLS = LBA_MATCH_GRID_COLS, MATCH_ROWS = LBA_MATCH_GRID_ROWS;
constexpr int MATCH_CELLS = MATCH_COLS * MATCH_ROWS;
constexpr int MATCH_HISTO = 30;           // HISTO_LENGTH
constexpr int MATCH_PENDING = -1;         // a job's status before k_match_resolve decides it

LBA_HD int match_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// DescriptorDistance: the Hamming distance of two 256-bit descriptors
LBA_HD int match_dist(const uint32_t* a, const uint32_t* b) {
    int d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d += match_popc(a[i] ^ b[i]);
    return d;
}

// one bound of the cell window: v is the floor / ceil value as a float.  false: not a number or outside int's range
// (quirk (e)).  Otherwise *cell is v clamped to [-1, n] in float and converted, which max(0, .) / min(n - 1, .) and the
// reference's two early returns treat as they treat (int)v.
LBA_HD bool match_cell(float v, int n, int* cell) {
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return false;
    const float c = fminf(fmaxf(v, -1.0f), (float)n);
    *cell = (int)c;
    return true;
}

struct MatchRect {
    int x0, x1, y0, y1;   // inclusive; empty when x0 > x1 or y0 > y1
};

// GetFeaturesInArea's nMinCellX .. nMaxCellY (src/Frame.cc:617-639).  false: the reference returns no candidate (a
// window wholly outside the grid), or the job is undefined there (quirk (e)).
LBA_HD bool match_rect(float x, float y, float r, const lba_match_cam& c, MatchRect* R) {
    if (!(isfinite(x) && isfinite(y) && isfinite(r))) return false;
    int x0, x1, y0, y1;
    if (!match_cell(floorf((x - c.min_x - r) * c.grid_w_inv), MATCH_COLS, &x0)) return false;
    if (!match_cell(ceilf((x - c.min_x + r) * c.grid_w_inv), MATCH_COLS, &x1)) return false;
    if (!match_cell(floorf((y - c.min_y - r) * c.grid_h_inv), MATCH_ROWS, &y0)) return false;
    if (!match_cell(ceilf((y - c.min_y + r) * c.grid_h_inv), MATCH_ROWS, &y1)) return false;
    x0 = x0 < 0 ? 0 : x0;
    if (x0 >= MATCH_COLS) return false;
    x1 = x1 > MATCH_COLS - 1 ? MATCH_COLS - 1 : x1;
    if (x1 < 0) return false;
    y0 = y0 < 0 ? 0 : y0;
    if (y0 >= MATCH_ROWS) return false;
    y1 = y1 > MATCH_ROWS - 1 ? MATCH_ROWS - 1 : y1;
    if (y1 < 0) return false;
    R->x0 = x0; R->x1 = x1; R->y0 = y0; R->y1 = y1;
    return true;
}

// what a job needs of its record for the gates
struct MatchJobGate {
    float x, y, radius, ur;
    int min_level, max_level;
    bool stereo;        // job.cam == params.stereo_cam
    bool ur_truncate;
};

// the level test and the window test of GetFeaturesInArea (:653-667), then the stereo gate of the matcher
// (ORBmatcher.cc:95-100 or :1499-1507): true when the feature is a candidate whose distance is computed
LBA_HD bool match_gate(const MatchJobGate& j, float fx, float fy, int octave, float u_right) {
    const bool check_levels = (j.min_level > 0) || (j.max_level >= 0);
    if (check_levels) {
        if (octave < j.min_level) return false;
        if (j.max_level >= 0 && octave > j.max_level) return false;
    }
    const float distx = fx - j.x, disty = fy - j.y;
    if (!(fabsf(distx) < j.radius && fabsf(disty) < j.radius)) return false;
    if (j.stereo) {
        const float u = j.ur_truncate ? truncf(u_right) : u_right;   // `int uRight = mvuRight[..]` (:1500)
        if (u > 0.0f) {
            const float er = fabsf(j.ur - u);
            if (er > j.radius) return false;
        }
    }
    return true;
}

// a candidate in the arena: the feature's index within its camera (13 bits), the distance (9), the octave (8)
LBA_HD uint32_t match_pack(int local, int dist, int octave) {
    return (uint32_t)local | ((uint32_t)dist << 13) | ((uint32_t)octave << 22);
}
LBA_HD int match_local(uint32_t w) { return (int)(w & 8191u); }
LBA_HD int match_wdist(uint32_t w) { return (int)((w >> 13) & 511u); }
LBA_HD int match_octave(uint32_t w) { return (int)(w >> 22); }

// the scan of :80-119 (LBA_MATCH_RATIO) and :1487-1517 (LBA_MATCH_BEST)
struct MatchPick {
    int best = 256, level = -1, best2 = 256, level2 = -1, idx = -1, n = 0;
};

LBA_HD void match_pick(MatchPick& p, int mode, int dist, int octave, int idx) {
    ++p.n;
    if (dist < p.best) {
        if (mode == LBA_MATCH_RATIO) {
            p.best2 = p.best;
            p.level2 = p.level;
        }
        p.best = dist;
        p.level = octave;
        p.idx = idx;
    } else if (mode == LBA_MATCH_RATIO && dist < p.best2) {
        p.level2 = octave;
        p.best2 = dist;
    }
}

// the acceptance rule of :122-142 / :1519
LBA_HD int match_decide(const MatchPick& p, int mode, int th_high, float nn_ratio) {
    if (p.n == 0) return LBA_MATCH_NO_CAND;
    if (!(p.best <= th_high)) return LBA_MATCH_TOO_FAR;
    if (mode == LBA_MATCH_RATIO && p.level == p.level2 && (float)p.best > nn_ratio * (float)p.best2)
        return LBA_MATCH_RATIO_FAIL;
    return LBA_MATCH_OK;
}

// the bin of :1531-1536
LBA_HD int match_rot_bin(float angle_last, float angle_cur) {
    const float factor = 1.0f / MATCH_HISTO;
    float rot = angle_last - angle_cur;
    if (rot < 0.0f) rot += 360.0f;
    const float b = roundf(rot * factor);
    int bin = (b >= 0.0f && b <= (float)MATCH_HISTO) ? (int)b : 0;   // the reference asserts the range
    if (bin == MATCH_HISTO) bin = 0;
    return bin;
}

// ---------------------------------------------------------------------------------------------------- host only

// ComputeThreeMaxima on the bins' sizes (:1697-1738)
inline void match_three_maxima(const int* histo, int L, int* ind1, int* ind2, int* ind3) {
    int max1 = 0, max2 = 0, max3 = 0;
    *ind1 = *ind2 = *ind3 = -1;
    for (int i = 0; i < L; ++i) {
        const int s = histo[i];
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            *ind3 = *ind2; *ind2 = *ind1; *ind1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            *ind3 = *ind2; *ind2 = i;
        } else if (s > max3) {
            max3 = s; *ind3 = i;
        }
    }
    if ((float)max2 < 0.1f * (float)max1) {
        *ind2 = -1; *ind3 = -1;
    } else if ((float)max3 < 0.1f * (float)max1) {
        *ind3 = -1;
    }
}

inline MatchJobGate match_job_gate(const lba_match_job& j, const lba_match_params& prm) {
    return MatchJobGate{j.x, j.y, j.radius, j.ur, j.min_level, j.max_level, j.cam == prm.stereo_cam,
                        prm.ur_truncate != 0};
}

// the candidate slots k_match_gather walks for a job: the features of its cell rectangle.  cell_start: the search's.
inline int match_capacity(const lba_match_job& j, const lba_match_cam& cam, const int32_t* cell_start) {
    MatchRect R;
    if (!match_rect(j.x, j.y, j.radius, cam, &R) || R.y0 > R.y1) return 0;
    const int32_t* cs = cell_start + (size_t)j.cam * MATCH_CELLS;
    int n = 0;
    for (int ix = R.x0; ix <= R.x1; ++ix) n += cs[ix * MATCH_ROWS + R.y1 + 1] - cs[ix * MATCH_ROWS + R.y0];
    return n;
}

// one job's candidate list as k_match_gather writes it: (search-local feature, distance), in order
inline void match_gather_host(const lba_match_job& j, const lba_match_cam& cam, const int32_t* cell_start,
                              const int32_t* cell_feat, const lba_match_feat* feats, const lba_match_params& prm,
                              std::vector<int>* feat, std::vector<int>* dist) {
    feat->clear();
    dist->clear();
    MatchRect R;
    if (!match_rect(j.x, j.y, j.radius, cam, &R)) return;
    const MatchJobGate g = match_job_gate(j, prm);
    const int32_t* cs = cell_start + (size_t)j.cam * MATCH_CELLS;
    for (int ix = R.x0; ix <= R.x1; ++ix)
        for (int iy = R.y0; iy <= R.y1; ++iy)
            for (int k = cs[ix * MATCH_ROWS + iy]; k < cs[ix * MATCH_ROWS + iy + 1]; ++k) {
                const lba_match_feat& f = feats[cell_feat[k]];
                if (!match_gate(g, f.x, f.y, f.octave, f.u_right)) continue;
                feat->push_back(cell_feat[k]);
                dist->push_back(match_dist(j.desc, f.desc));
            }
}

// the rotation pass and the counts of one search on its decided jobs (status, feat) and features (job): :1546-1567
inline void match_finish(lba_match_search& S, const lba_match_params& prm, lba_match_job* jobs, lba_match_feat* feats) {
    int n = 0, mono = 0;
    for (int k = 0; k < S.n_jobs; ++k)
        if (jobs[k].status == LBA_MATCH_OK) {
            ++n;
            mono += jobs[k].cam < S.n_cam - 1;
        }
    if (prm.mode == LBA_MATCH_BEST && prm.check_orientation) {
        int histo[MATCH_HISTO] = {};
        for (int k = 0; k < S.n_jobs; ++k)
            if (jobs[k].status == LBA_MATCH_OK) ++histo[match_rot_bin(jobs[k].angle, feats[jobs[k].feat].angle)];
        int i1, i2, i3;
        match_three_maxima(histo, MATCH_HISTO, &i1, &i2, &i3);
        for (int k = 0; k < S.n_jobs; ++k) {
            if (jobs[k].status != LBA_MATCH_OK) continue;
            const int bin = match_rot_bin(jobs[k].angle, feats[jobs[k].feat].angle);
            if (bin == i1 || bin == i2 || bin == i3) continue;
            jobs[k].status = LBA_MATCH_ROT;
            feats[jobs[k].feat].job = -1;
            --n;
        }
    }
    S.n_matches = n;
    S.n_matches_mono = mono;
}

// a whole search in job order, as the reference's loops run it (no argument checks): the jobs' and features' outputs
// and the counts; the cameras' rounds are not touched.  The arrays are the search's own (index 0 is its first).
inline void match_search_host(lba_match_search& S, const lba_match_cam* cams, const int32_t* cell_start,
                              const int32_t* cell_feat, lba_match_feat* feats, lba_match_job* jobs,
                              const lba_match_params& prm) {
    std::vector<char> taken(S.n_feat);
    for (int f = 0; f < S.n_feat; ++f) {
        taken[f] = feats[f].taken != 0;
        feats[f].job = -1;
    }
    std::vector<int> cf, cd;
    for (int k = 0; k < S.n_jobs; ++k) {
        lba_match_job& j = jobs[k];
        match_gather_host(j, cams[j.cam], cell_start, cell_feat, feats, prm, &cf, &cd);
        MatchPick p;
        for (size_t i = 0; i < cf.size(); ++i)
            if (!taken[cf[i]]) match_pick(p, prm.mode, cd[i], feats[cf[i]].octave, cf[i]);
        j.status = match_decide(p, prm.mode, prm.th_high, prm.nn_ratio);
        j.best_dist = p.best;
        j.best_dist2 = p.best2;
        j.feat = j.status == LBA_MATCH_OK ? p.idx : -1;
        if (j.status == LBA_MATCH_OK) {
            feats[p.idx].job = k;
            if (j.blocks) taken[p.idx] = 1;
        }
    }
    match_finish(S, prm, jobs, feats);
}

}  // namespace lba
