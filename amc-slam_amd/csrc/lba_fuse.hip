// lba_fuse.hip — the search of ORBmatcher::Fuse, both overloads (src/ORBmatcher.cc:1133-1316 and :1318-1437), for a batch
// of searches: LocalMapping::SearchInNeighbors' 20 + 1 calls and LoopClosing::SearchAndFuse's one call per corrected
// keyframe.  Neither overload keeps a matched flag, so a job (search, point, camera) is a pure function of the point and
// the target keyframe: there is no greedy stage, no candidate list, no readback and no resolve.  The map-editing tail of
// each job (Replace / AddObservation / vpReplacePoint) is the caller's ordered walk over the rows.
//
//   k_fuse  ONE launch.  A wave takes 64 consecutive jobs.  Lane = job for the search lookup (binary search over
//           job0[]), the float projection, the gates and PredictScale (lba_fuse_math.hpp).  One ballot gives the live
//           jobs; the wave walks them one by one, wave-uniform: the owner's job, camera and point are read from its
//           lane, all 64 lanes stride the spans of the window's cell rectangle in GetFeaturesInArea's order (ix, then
//           iy, then the cell's list: a column's cells are one contiguous span of the CSR grid), each lane keeps the
//           minimum of (distance << 20 | walk position) with its feature, the position being a running ballot /
//           popcount over the candidates that passed the gates.  The wave-wide minimum is the FIRST walk position of
//           the smallest distance, which is the reference's strict <.  Every lane stores its own 32-byte row.
// No atomics, no LDS, no barrier, no wait on another workgroup.  A row depends on its job alone: not on the batch, the
// grid or its position in the wave.  One upload, one launch, one download; n_ok and the scatter on the host.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_fuse_math.hpp"
#include "lba_tracker.hpp"

using namespace lba;

namespace {

constexpr int FU_WG = 256;   // four independent waves
typedef unsigned long long u64;
static_assert(sizeof(lba_fuse_cam) == 72 && sizeof(lba_fuse_target) == 48 && sizeof(lba_fuse_search) == 32 &&
              sizeof(lba_fuse_row) == 32 && sizeof(lba_s3p_point) == 80 && sizeof(lba_match_feat) == 64 &&
              sizeof(lba_match_cam) == 20, "ABI layout");

struct FuseArgs {
    const lba_fuse_target* targets;
    const lba_fuse_cam* fcams;
    const lba_match_cam* gcams;
    const float* sf;
    const float* sigma;
    const int* cell_start;
    const int* cell_feat;
    const lba_match_feat* feats;
    const lba_fuse_search* searches;
    const lba_s3p_point* points;
    const int* job0;       // [n_searches + 1]: the search's first job
    lba_fuse_row* rows;    // out [n_jobs]
    int n_searches, n_jobs, th_low;
};

__device__ __forceinline__ int lane_int(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float lane_float(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

__global__ __launch_bounds__(FU_WG) void k_fuse(FuseArgs A) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * FU_WG + threadIdx.x;   // a wave's 64 lanes: 64 consecutive jobs
    const bool mine = g < A.n_jobs;
    FuseJob J{LBA_FUSE_SKIPPED, -1, 0.0f, 0.0f, 0.0f, 0.0f};
    int s = 0, c = 0, pt = 0;
    if (mine) {
        int lo = 0, hi = A.n_searches;   // the search with job0[s] <= g < job0[s + 1] (empty searches are stepped over)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (A.job0[mid] <= g) lo = mid;
            else hi = mid;
        }
        s = lo;
        const lba_fuse_search S = A.searches[s];
        const lba_fuse_target T = A.targets[S.target];
        const int k = g - A.job0[s];
        c = k % T.n_cam;
        pt = S.point0 + k / T.n_cam;
        J = fuse_project(A.fcams[T.cam0 + c], A.points[pt], S.mode, c, T.n_cam, S.th, T.bf, T.log_scale_factor,
                         T.n_levels, A.sf + T.sf0);
    }
    lba_fuse_row R = fuse_gated_row(J);
    u64 live = __ballot(mine && J.status == FUSE_PENDING);
    while (live) {   // wave-uniform: every lane of the wave is here
        const int o = __ffsll((long long)live) - 1;
        live &= live - 1;
        const FuseJob Jo{FUSE_PENDING, lane_int(J.level, o), lane_float(J.x, o), lane_float(J.y, o),
                         lane_float(J.radius, o), lane_float(J.ur, o)};
        const int os = lane_int(s, o), oc = lane_int(c, o), opt = lane_int(pt, o);
        const lba_fuse_search S = A.searches[os];
        const lba_fuse_target T = A.targets[S.target];
        const lba_match_cam C = A.gcams[T.cam0 + oc];
        const bool last_cam = oc == T.n_cam - 1;
        const float* sg = A.sigma + T.sigma0;
        uint32_t desc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) desc[k] = A.points[opt].desc[k];
        unsigned count = 0;
        uint32_t key = 0xffffffffu;
        int kfeat = -1;
        MatchRect Q;
        if (match_rect(Jo.x, Jo.y, Jo.radius, C, &Q) && Q.y0 <= Q.y1) {
            const int* cs = A.cell_start + T.cell0 + (size_t)oc * MATCH_CELLS;
            const int* cf = A.cell_feat + T.cf0;
            const lba_match_feat* feats = A.feats + T.feat0;
            for (int ix = Q.x0; ix <= Q.x1; ++ix) {
                const int b = cs[ix * MATCH_ROWS + Q.y0], e = cs[ix * MATCH_ROWS + Q.y1 + 1];
                for (int k = b; k < e; k += 64) {
                    const int j = k + lane;
                    bool ok = false;
                    int f = -1, d = 0;
                    if (j < e) {
                        f = cf[j];
                        const lba_match_feat* F = feats + f;
                        const int octave = F->octave;
                        ok = fuse_gate(Jo, S.mode, last_cam, F->x, F->y, octave, F->u_right, sg);
                        if (ok) d = match_dist(desc, F->desc);
                    }
                    const u64 mask = __ballot(ok);
                    if (ok) {
                        const unsigned pos = count + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
                        const uint32_t kk = ((uint32_t)d << 20) | pos;   // pos < 8192 per camera, d <= 256
                        if (kk < key) {
                            key = kk;
                            kfeat = f;
                        }
                    }
                    count += (unsigned)__popcll(mask);
                }
            }
        }
        uint32_t m = key;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)m, d, 64);
            m = other < m ? other : m;
        }
        const u64 who = __ballot(count != 0 && key == m);   // the keys differ in their positions: one lane
        const int idx = who ? lane_int(kfeat, __ffsll((long long)who) - 1) : -1;
        if (lane == o) R = fuse_decide(J, S.mode, (int)count, count ? (int)(m >> 20) : INT_MAX, idx, A.th_low);
    }
    if (mine) A.rows[g] = R;
}

#define FUSE_REFUSE(c, m) return tracker_fail(t, TrackerError{c, "lba_match_fuse: " m})

}  // namespace

extern "C" int lba_match_fuse_profile(lba_tracker* t, int32_t on, double* last_ms) {
    return t ? t->fuse_timer.profile(on, last_ms, 1) : LBA_E_ARG;
}

extern "C" int lba_match_fuse(lba_tracker* t, const lba_fuse_target* targets, int32_t n_targets,
                              const lba_fuse_cam* fcams, const lba_match_cam* gcams, int32_t n_cams,
                              const float* scale_factors, int32_t n_scale_factors, const float* inv_level_sigma2,
                              int32_t n_inv_level_sigma2, const int32_t* cell_start, int32_t n_cell_start,
                              const int32_t* cell_feat, int32_t n_cell_feat, const lba_match_feat* feats,
                              int32_t n_feats, lba_fuse_search* searches, int32_t n_searches,
                              const lba_s3p_point* points, int32_t n_points, lba_fuse_row* rows, int32_t n_rows,
                              int32_t th_low) {
    if (!t) return LBA_E_ARG;
    if (n_targets < 0 || n_cams < 0 || n_scale_factors < 0 || n_inv_level_sigma2 < 0 || n_cell_start < 0 ||
        n_cell_feat < 0 || n_feats < 0 || n_searches < 0 || n_points < 0 || n_rows < 0)
        FUSE_REFUSE(LBA_E_ARG, "a negative count");
    if ((n_targets && !targets) || (n_cams && (!fcams || !gcams)) || (n_scale_factors && !scale_factors) ||
        (n_inv_level_sigma2 && !inv_level_sigma2) || (n_cell_start && !cell_start) || (n_cell_feat && !cell_feat) ||
        (n_feats && !feats) || (n_searches && !searches) || (n_points && !points) || (n_rows && !rows))
        FUSE_REFUSE(LBA_E_ARG, "a null array");
    if (th_low < 0) FUSE_REFUSE(LBA_E_ARG, "th_low negative");
    // ---- checks first: a refused call writes nothing.  Each target's grid as lba_match_project checks one search's.
    for (int k = 0; k < n_targets; ++k) {
        const lba_fuse_target& T = targets[k];
        if (T.n_cam < 1) FUSE_REFUSE(LBA_E_ARG, "a target's n_cam < 1");
        if (T.n_levels < 1) FUSE_REFUSE(LBA_E_ARG, "a target's n_levels < 1");
        if (T.n_cam > LBA_FUSE_MAX_CAM) FUSE_REFUSE(LBA_E_LIMIT, "a target's n_cam > 64");
        if (T.cam0 < 0 || (int64_t)T.cam0 + T.n_cam > n_cams) FUSE_REFUSE(LBA_E_ARG, "a target's cameras outside the array");
        if (T.n_feat < 0 || T.feat0 < 0 || (int64_t)T.feat0 + T.n_feat > n_feats)
            FUSE_REFUSE(LBA_E_ARG, "a target's features outside the array");
        if (T.sf0 < 0 || (int64_t)T.sf0 + T.n_levels > n_scale_factors || T.sigma0 < 0 ||
            (int64_t)T.sigma0 + T.n_levels > n_inv_level_sigma2)
            FUSE_REFUSE(LBA_E_ARG, "a target's scale_factors or inv_level_sigma2 outside the array");
        const int64_t n_cells = (int64_t)T.n_cam * MATCH_CELLS;
        if (T.cell0 < 0 || (int64_t)T.cell0 + n_cells + 1 > n_cell_start)
            FUSE_REFUSE(LBA_E_ARG, "a target's cell_start outside the array");
        const int32_t* cs = cell_start + T.cell0;
        if (cs[0] != 0) FUSE_REFUSE(LBA_E_ARG, "a target's cell_start does not begin at 0");
        for (int64_t c = 0; c < n_cells; ++c)
            if (cs[c + 1] < cs[c]) FUSE_REFUSE(LBA_E_ARG, "cell_start decreases");
        if (T.cf0 < 0 || (int64_t)T.cf0 + cs[n_cells] > n_cell_feat)
            FUSE_REFUSE(LBA_E_ARG, "a target's cell_feat outside the array");
        std::vector<int> per_cam((size_t)T.n_cam, 0);
        for (int f = 0; f < T.n_feat; ++f) {
            const lba_match_feat& F = feats[T.feat0 + f];
            if (F.cam < 0 || F.cam >= T.n_cam || F.octave < 0 || F.octave > 255)
                FUSE_REFUSE(LBA_E_ARG, "a feature's camera outside [0, n_cam) or octave outside [0, 255]");
            if (++per_cam[(size_t)F.cam] > LBA_MATCH_MAX_FEAT)
                FUSE_REFUSE(LBA_E_LIMIT, "more than 8192 features in one camera");
        }
        for (int c = 0; c < T.n_cam; ++c)
            for (int i = cs[(size_t)c * MATCH_CELLS]; i < cs[(size_t)(c + 1) * MATCH_CELLS]; ++i) {
                const int f = cell_feat[T.cf0 + i];
                if (f < 0 || f >= T.n_feat || feats[T.feat0 + f].cam != c)
                    FUSE_REFUSE(LBA_E_ARG, "a cell names a feature outside the target or of another camera");
            }
    }
    std::vector<int> job0((size_t)n_searches + 1, 0);
    {
        int64_t row_end = 0;
        for (int s = 0; s < n_searches; ++s) {
            const lba_fuse_search& S = searches[s];
            if (S.target < 0 || S.target >= n_targets) FUSE_REFUSE(LBA_E_ARG, "a search's target outside the array");
            if (S.mode != LBA_FUSE_KF && S.mode != LBA_FUSE_SIM3) FUSE_REFUSE(LBA_E_ARG, "a search's mode is neither of the two");
            if (!(S.th >= 0.0f) || !std::isfinite(S.th)) FUSE_REFUSE(LBA_E_ARG, "a search's th negative or not finite");
            if (S.n_points < 0 || S.point0 < 0 || (int64_t)S.point0 + S.n_points > n_points)
                FUSE_REFUSE(LBA_E_ARG, "a search's points outside the array");
            const int64_t n = (int64_t)S.n_points * targets[S.target].n_cam;
            if (S.row0 < row_end || (int64_t)S.row0 + n > n_rows)
                FUSE_REFUSE(LBA_E_ARG, "a search's rows outside the array or overlapping the search before");
            row_end = (int64_t)S.row0 + n;
            const int64_t end = (int64_t)job0[s] + n;
            if (end > 0x7fffffff - 2 * FU_WG) FUSE_REFUSE(LBA_E_LIMIT, "the batch exceeds 2 GB");
            job0[(size_t)s + 1] = (int)end;
        }
    }
    const size_t ns = (size_t)n_searches, nj = (size_t)job0[ns];
    if (nj == 0) {
        for (int s = 0; s < n_searches; ++s) searches[s].n_ok = 0;
        return LBA_OK;
    }
    // ---- the arena: inputs (one upload), the rows (one download)
    ArenaPlan plan;
    const Sec<lba_fuse_target> o_targets = plan.in<lba_fuse_target>((size_t)n_targets);
    const Sec<lba_fuse_cam> o_fcams = plan.in<lba_fuse_cam>((size_t)n_cams);
    const Sec<lba_match_cam> o_gcams = plan.in<lba_match_cam>((size_t)n_cams);
    const Sec<float> o_sf = plan.in<float>((size_t)n_scale_factors), o_sg = plan.in<float>((size_t)n_inv_level_sigma2);
    const Sec<int32_t> o_cs = plan.in<int32_t>((size_t)n_cell_start), o_cf = plan.in<int32_t>((size_t)n_cell_feat);
    const Sec<lba_match_feat> o_feats = plan.in<lba_match_feat>((size_t)n_feats);
    const Sec<lba_fuse_search> o_searches = plan.in<lba_fuse_search>(ns);
    const Sec<lba_s3p_point> o_points = plan.in<lba_s3p_point>((size_t)n_points);
    const Sec<int> o_job0 = plan.in<int>(ns + 1);
    const Sec<lba_fuse_row> o_rows = plan.out<lba_fuse_row>(nj);
    if (plan.over_2gb()) FUSE_REFUSE(LBA_E_LIMIT, "the batch exceeds 2 GB");
    char* h = nullptr;
    try {
        ArenaCall call{t, plan, t->fuse_timer};
        h = call.pin();
        std::memcpy(o_targets.at(h), targets, (size_t)n_targets * sizeof(lba_fuse_target));
        std::memcpy(o_fcams.at(h), fcams, (size_t)n_cams * sizeof(lba_fuse_cam));
        std::memcpy(o_gcams.at(h), gcams, (size_t)n_cams * sizeof(lba_match_cam));
        std::memcpy(o_sf.at(h), scale_factors, (size_t)n_scale_factors * sizeof(float));
        std::memcpy(o_sg.at(h), inv_level_sigma2, (size_t)n_inv_level_sigma2 * sizeof(float));
        std::memcpy(o_cs.at(h), cell_start, (size_t)n_cell_start * sizeof(int32_t));
        if (n_cell_feat) std::memcpy(o_cf.at(h), cell_feat, (size_t)n_cell_feat * sizeof(int32_t));
        if (n_feats) std::memcpy(o_feats.at(h), feats, (size_t)n_feats * sizeof(lba_match_feat));
        std::memcpy(o_searches.at(h), searches, ns * sizeof(lba_fuse_search));
        std::memcpy(o_points.at(h), points, (size_t)n_points * sizeof(lba_s3p_point));
        std::memcpy(o_job0.at(h), job0.data(), (ns + 1) * sizeof(int));
        char* d = call.place();
        call.upload();
        FuseArgs a;
        a.targets = o_targets.at(d); a.fcams = o_fcams.at(d); a.gcams = o_gcams.at(d); a.sf = o_sf.at(d);
        a.sigma = o_sg.at(d); a.cell_start = o_cs.at(d); a.cell_feat = o_cf.at(d); a.feats = o_feats.at(d);
        a.searches = o_searches.at(d); a.points = o_points.at(d); a.job0 = o_job0.at(d); a.rows = o_rows.at(d);
        a.n_searches = n_searches; a.n_jobs = (int)nj; a.th_low = th_low;
        call.mark();
        hipLaunchKernelGGL(k_fuse, dim3((unsigned)((nj + FU_WG - 1) / FU_WG)), dim3(FU_WG), 0, t->stream, a);
        TR_HIP(hipGetLastError());
        call.mark();
        call.finish();
    } catch (const TrackerError& e) {
        return tracker_fail(t, e);
    }
    // ---- scatter: the rows into the searches' ranges; n_ok
    const lba_fuse_row* r_rows = o_rows.at(h);
    for (int s = 0; s < n_searches; ++s) {
        lba_fuse_search& S = searches[s];
        const size_t n = (size_t)(job0[(size_t)s + 1] - job0[s]);
        if (n) std::memcpy(rows + S.row0, r_rows + job0[s], n * sizeof(lba_fuse_row));
        int m = 0;
        for (size_t k = 0; k < n; ++k) m += r_rows[job0[s] + k].status == LBA_FUSE_OK;
        S.n_ok = m;
    }
    return LBA_OK;
}
