// lba_sim3_project.hip — the Sim3 ORBmatcher::SearchByProjection (src/ORBmatcher.cc:423-548 and :550-685) for a batch of
// hypotheses against one keyframe: the step between lba_sim3_ransac, lba_sim3_optimize and the acceptance counts of
// LoopClosing::DetectCommonRegionsFromBoW, and FindMatchesByProjection's search.
//
// The keyframe (features, grid, cameras) goes up once; a search is a hypothesis with its Sbw and its range of `points`.
// A job is one (search, point, camera), numbered search after search, point-major, cameras inner.
//   k_s3p_pose     one thread per (search, camera): the fp64 pose chain of lba_s3p_math.hpp, Tcw as doubles and floats.
//   k_s3p_project  one thread per job: the float projection and gates; a job that fails a gate has its final row here,
//                  a live one gets S3P_PENDING, its level, x, y, radius and the capacity of its candidate list.
//   k_s3p_compact  one workgroup per (search, camera): a workgroup-local scan over the camera's jobs in order gives the
//                  list of its live jobs and each one's offset into the camera's candidates, and the two totals.
//   k_s3p_base     one workgroup: the exclusive scan of the cameras' candidate totals.
//   -- ONE readback of the per-(search, camera) totals (live jobs, candidate slots): the host sizes the candidate
//      buffer and the gather's grid.  The arena cannot grow between two launches without losing what it holds, so the
//      candidate lists live in a buffer of their own on the tracker (d_cand); the 2 GB limit counts both.
//   k_s3p_gather   one wave per live job, as k_match_gather: levels [level - 1, level], no stereo gate; every store is
//                  bounded by the job's capacity.
//   k_s3p_resolve  one workgroup per (search, camera): k_match_resolve's rounds (the proof is in lba_match.hip) with
//                  this function's acceptance test; every accepted job blocks.  A second copy of that loop: lifting it
//                  into a shared header would have to leave k_match_resolve's code unchanged, which was not established.
// Cameras are independent: a feature belongs to one camera, so vpMatched never couples two of them (quirk (b)).
// No workgroup waits on another, no atomics outside LDS.  One upload, one download, n_matches and the scatter on the host.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_s3p_math.hpp"
#include "lba_tracker.hpp"

using namespace lba;

namespace {

constexpr int SP_WG = 256;
constexpr int SG_WG = 64;     // k_s3p_gather: one wave
constexpr int SR_WORDS = LBA_MATCH_MAX_FEAT / 32;
typedef unsigned long long u64;
static_assert(sizeof(lba_s3p_kf) == 136 && sizeof(lba_s3p_cam) == 88 && sizeof(lba_s3p_point) == 80 &&
              sizeof(lba_s3p_search) == 64 && sizeof(lba_s3p_row) == 32 && sizeof(lba_s3p_pose) == 152 &&
              sizeof(lba_s3p_params) == 16, "ABI layout");

struct S3pArgs {
    const lba_s3p_kf* kf;
    const lba_s3p_cam* kcams;
    const lba_match_cam* gcams;
    const float* sf;
    const int* cell_start;
    const int* cell_feat;
    const lba_match_feat* feats;
    const int* feat_local;     // [n_feats]: the feature's index within its camera
    const int* cam_feats;      // the features camera by camera, each in index order
    const int* cam_feat0;      // [n_cam + 1]
    const lba_s3p_search* searches;
    const lba_s3p_point* points;
    const uint8_t* taken;
    const int* job0;           // [n_searches + 1]: the search's first job
    lba_s3p_row* rows;         // out [n_jobs]
    int* feat_point;           // out [n_searches][n_feats]
    lba_s3p_pose* poses;       // out [n_searches][n_cam]
    int* n_live;               // out [n_searches][n_cam]
    u64* cap_total;            // out [n_searches][n_cam]
    int* cap;                  // work [n_jobs]: a live job's candidate slots
    unsigned* loff;            // work [n_jobs]: its list's offset within its camera's candidates
    int* live;                 // work [n_jobs]: camera c of search s lists its live jobs from job0[s] + c * n_points on
    int* n_cand;               // work [n_jobs]
    u64* base;                 // work [n_searches][n_cam]: the camera's first candidate slot
    uint32_t* cand;
    int n_searches, n_cam, n_feats, n_jobs;
    int th, th_low, proj_form;
    float ratio;
    int max_live;
};

__global__ __launch_bounds__(SP_WG) void k_s3p_pose(S3pArgs A) {
    const int i = blockIdx.x * SP_WG + threadIdx.x;
    if (i >= A.n_searches * A.n_cam) return;
    const int s = i / A.n_cam, c = i % A.n_cam;
    const lba_s3p_search* S = A.searches + s;
    double tcw[12];
    s3p_pose(*A.kf, A.kcams[c], S->q, S->t, S->s, tcw);
    lba_s3p_pose* P = A.poses + i;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        P->tcw_d[k] = tcw[k];
        P->tcw[k] = (float)tcw[k];
    }
    P->rounds = 0;
    P->pad = 0;
}

__global__ __launch_bounds__(SP_WG) void k_s3p_project(S3pArgs A) {
    const int g = blockIdx.x * SP_WG + threadIdx.x;
    if (g >= A.n_jobs) return;
    int lo = 0, hi = A.n_searches;   // the search with job0[s] <= g < job0[s + 1] (empty searches are stepped over)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.job0[mid] <= g) lo = mid;
        else hi = mid;
    }
    const int s = lo, k = g - A.job0[s];
    const int p = k / A.n_cam, c = k % A.n_cam;
    const lba_s3p_kf* K = A.kf;
    const S3pJob J = s3p_project(A.poses[s * A.n_cam + c].tcw, A.kcams[c], A.points[A.searches[s].point0 + p], A.th,
                                 A.proj_form, K->log_scale_factor, K->n_levels, A.sf);
    A.rows[g] = lba_s3p_row{J.status, -1, 256, J.level, J.x, J.y, J.radius, 0};
    A.cap[g] = J.status == S3P_PENDING
                   ? s3p_capacity(J.x, J.y, J.radius, A.gcams[c], A.cell_start + (size_t)c * MATCH_CELLS)
                   : 0;
}

// the workgroup's exclusive scan of one value per thread; *total: the sum.  `part`: SP_WG / 64 words of LDS.
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* part, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();   // `part` may still be read from the scan before
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SP_WG / 64; ++w) {
        const T t = part[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(SP_WG) void k_s3p_compact(S3pArgs A) {
    __shared__ unsigned part_n[SP_WG / 64];
    __shared__ u64 part_c[SP_WG / 64];
    const int s = blockIdx.x / A.n_cam, c = blockIdx.x % A.n_cam;
    const int j0 = A.job0[s], n_points = A.searches[s].n_points;
    int* list = A.live + j0 + (size_t)c * n_points;
    unsigned n_before = 0;
    u64 c_before = 0;
    for (int p0 = 0; p0 < n_points; p0 += SP_WG) {
        const int p = p0 + threadIdx.x;
        const int g = j0 + p * A.n_cam + c;
        const bool is_live = p < n_points && A.rows[g].status == S3P_PENDING;
        const u64 my_cap = is_live ? (u64)A.cap[g] : 0;
        unsigned tot_n;
        u64 tot_c;
        const unsigned pos = block_scan<unsigned>(is_live ? 1u : 0u, part_n, &tot_n);
        const u64 off = block_scan<u64>(my_cap, part_c, &tot_c);
        if (is_live) {
            list[n_before + pos] = g;                      // n_before + pos < n_points: at most one entry per point
            A.loff[g] = (unsigned)(c_before + off);        // (a camera above 2^32 slots is refused before it is used)
        }
        n_before += tot_n;
        c_before += tot_c;
    }
    if (threadIdx.x == 0) {
        A.n_live[blockIdx.x] = (int)n_before;
        A.cap_total[blockIdx.x] = c_before;
    }
}

__global__ __launch_bounds__(SP_WG) void k_s3p_base(S3pArgs A) {
    __shared__ u64 part[SP_WG / 64];
    const int n = A.n_searches * A.n_cam;
    u64 before = 0;
    for (int i0 = 0; i0 < n; i0 += SP_WG) {
        const int i = i0 + threadIdx.x;
        u64 tot;
        const u64 off = block_scan<u64>(i < n ? A.cap_total[i] : 0, part, &tot);
        if (i < n) A.base[i] = before + off;
        before += tot;
    }
}

__global__ __launch_bounds__(SG_WG) void k_s3p_gather(S3pArgs A) {
    const int sc = blockIdx.x / A.max_live, i = blockIdx.x % A.max_live, lane = threadIdx.x;
    if (i >= A.n_live[sc]) return;
    const int s = sc / A.n_cam, cam = sc % A.n_cam;
    const int g = A.live[A.job0[s] + (size_t)cam * A.searches[s].n_points + i];
    const lba_s3p_row R0 = A.rows[g];
    const int p = (g - A.job0[s]) / A.n_cam;
    const lba_s3p_point* P = A.points + A.searches[s].point0 + p;
    const lba_match_cam C = A.gcams[cam];
    const MatchJobGate G{R0.x, R0.y, R0.radius, 0.0f, R0.level - 1, R0.level, false, false};
    uint32_t desc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) desc[k] = P->desc[k];
    const u64 off = A.base[sc] + A.loff[g];
    const unsigned cap = (unsigned)A.cap[g];
    unsigned count = 0;
    MatchRect R;
    if (match_rect(G.x, G.y, G.radius, C, &R) && R.y0 <= R.y1) {
        const int* cs = A.cell_start + (size_t)cam * MATCH_CELLS;
        for (int ix = R.x0; ix <= R.x1; ++ix) {
            const int b = cs[ix * MATCH_ROWS + R.y0], e = cs[ix * MATCH_ROWS + R.y1 + 1];
            for (int k = b; k < e; k += SG_WG) {
                const int j = k + lane;
                bool ok = false;
                uint32_t w = 0;
                if (j < e) {
                    const int f = A.cell_feat[j];
                    const lba_match_feat* F = A.feats + f;
                    const int octave = F->octave;
                    ok = match_gate(G, F->x, F->y, octave, F->u_right);
                    if (ok) w = match_pack(A.feat_local[f], match_dist(desc, F->desc), octave);
                }
                const unsigned long long mask = __ballot(ok);
                if (ok) {
                    const unsigned pos = count + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
                    if (pos < cap) A.cand[off + pos] = w;   // pos < cap always: k_s3p_project summed the same spans
                }
                count += (unsigned)__popcll(mask);
            }
        }
    }
    if (lane == 0) A.n_cand[g] = (int)(count < cap ? count : cap);
}

// k_match_resolve's rounds (lba_match.hip has the proof) on the camera's live jobs: LBA_MATCH_BEST's scan, this
// function's acceptance test, every accepted job blocks.  k is the job's position in the camera's live list.
__global__ __launch_bounds__(SP_WG) void k_s3p_resolve(S3pArgs A) {
    __shared__ int minp[LBA_MATCH_MAX_FEAT];
    __shared__ int fjob[LBA_MATCH_MAX_FEAT];
    __shared__ unsigned tk[2][SR_WORDS];
    static_assert(SR_WORDS == SP_WG, "one taken word per thread");
    const int tid = threadIdx.x;
    const int sc = blockIdx.x, s = sc / A.n_cam, c = sc % A.n_cam;
    const lba_s3p_search* S = A.searches + s;
    const int n_jobs = A.n_live[sc];
    const int j0 = A.job0[s];
    const int* cam_jobs = A.live + j0 + (size_t)c * S->n_points;
    const int* cam_feats = A.cam_feats + A.cam_feat0[c];
    const int n_feat = A.cam_feat0[c + 1] - A.cam_feat0[c];
    const uint8_t* taken = S->taken0 >= 0 ? A.taken + S->taken0 : nullptr;
    const u64 base = A.base[sc];
    tk[0][tid] = 0u;
    __syncthreads();
    for (int i = tid; i < n_feat; i += SP_WG) {
        minp[i] = INT_MAX;
        fjob[i] = -1;
        if (taken && taken[cam_feats[i]] != 0) atomicOr(&tk[0][i >> 5], 1u << (i & 31));
    }
    __syncthreads();
    tk[1][tid] = tk[0][tid];
    __syncthreads();
    int rounds = 0;
    while (rounds < n_jobs) {
        int any = 0;
        for (int p = tid; p < n_jobs; p += SP_WG) {
            const int g = cam_jobs[p];
            if (A.rows[g].status != S3P_PENDING) continue;
            any = 1;
            const uint32_t* cand = A.cand + base + A.loff[g];
            const int n = A.n_cand[g];
            for (int i = 0; i < n; ++i) {
                const int l = match_local(cand[i]);
                if (!((tk[0][l >> 5] >> (l & 31)) & 1u)) atomicMin(&minp[l], p);
            }
        }
        if (!__syncthreads_or(any)) break;
        ++rounds;
        for (int p = tid; p < n_jobs; p += SP_WG) {
            const int g = cam_jobs[p];
            if (A.rows[g].status != S3P_PENDING) continue;
            const uint32_t* cand = A.cand + base + A.loff[g];
            const int n = A.n_cand[g];
            MatchPick pk;
            bool fin = true;
            for (int i = 0; i < n; ++i) {
                const uint32_t w = cand[i];
                const int l = match_local(w);
                if ((tk[0][l >> 5] >> (l & 31)) & 1u) continue;
                if (minp[l] != p) {
                    fin = false;
                    break;
                }
                match_pick(pk, LBA_MATCH_BEST, match_wdist(w), match_octave(w), l);
            }
            if (!fin) continue;
            const int st = s3p_decide(pk, A.th_low, A.ratio);
            A.rows[g].feat = st == LBA_S3P_OK ? cam_feats[pk.idx] : -1;
            A.rows[g].best_dist = pk.best;
            A.rows[g].status = st;
            if (st == LBA_S3P_OK) {
                fjob[pk.idx] = (g - j0) / A.n_cam;
                atomicOr(&tk[1][pk.idx >> 5], 1u << (pk.idx & 31));
            }
        }
        __syncthreads();
        for (int i = tid; i < n_feat; i += SP_WG) minp[i] = INT_MAX;
        tk[0][tid] = tk[1][tid];
        __syncthreads();
    }
    int* fp = A.feat_point + (size_t)s * A.n_feats;
    for (int i = tid; i < n_feat; i += SP_WG) fp[cam_feats[i]] = fjob[i];
    if (tid == 0) A.poses[sc].rounds = rounds;
}

#define S3P_REFUSE(c, m) return tracker_fail(t, TrackerError{c, "lba_match_sim3_project: " m})

}  // namespace

extern "C" int lba_match_sim3_project_profile(lba_tracker* t, int32_t on, double* last_ms) {
    return t ? t->s3p_timer.profile(on, last_ms, 6) : LBA_E_ARG;
}

extern "C" int lba_match_sim3_project(lba_tracker* t, const lba_s3p_kf* kf, const lba_s3p_cam* kcams,
                                      const lba_match_cam* gcams, const float* scale_factors, const int32_t* cell_start,
                                      int32_t n_cell_start, const int32_t* cell_feat, int32_t n_cell_feat,
                                      const lba_match_feat* feats, int32_t n_feats, lba_s3p_search* searches,
                                      int32_t n_searches, const lba_s3p_point* points, int32_t n_points,
                                      const uint8_t* taken, int32_t n_taken, lba_s3p_row* rows, int32_t n_rows,
                                      int32_t* feat_point, int32_t n_feat_point, lba_s3p_pose* poses, int32_t n_poses,
                                      const lba_s3p_params* prm) {
    if (!t) return LBA_E_ARG;
    if (n_cell_start < 0 || n_cell_feat < 0 || n_feats < 0 || n_searches < 0 || n_points < 0 || n_taken < 0 || n_rows < 0 ||
        n_feat_point < 0 || n_poses < 0)
        S3P_REFUSE(LBA_E_ARG, "a negative count");
    if (!kf || !kcams || !gcams || !scale_factors || !cell_start || !prm || (n_cell_feat && !cell_feat) ||
        (n_feats && !feats) || (n_searches && !searches) || (n_points && !points) || (n_taken && !taken) ||
        (n_rows && !rows) || (n_feat_point && !feat_point) || (n_poses && !poses))
        S3P_REFUSE(LBA_E_ARG, "a null array");
    const lba_s3p_params P = *prm;
    if (const char* m = s3p_params_error(P)) return tracker_fail(t, TrackerError{LBA_E_ARG, m});
    const lba_s3p_kf K = *kf;
    const int n_cam = K.n_cam;
    if (n_cam < 1) S3P_REFUSE(LBA_E_ARG, "n_cam < 1");
    if (K.n_levels < 1) S3P_REFUSE(LBA_E_ARG, "n_levels < 1");
    if (n_cam > LBA_S3P_MAX_CAM) S3P_REFUSE(LBA_E_LIMIT, "n_cam > 64");
    // ---- checks first: a refused call writes nothing.  The grid as lba_match_project checks one search's.
    std::vector<int> cam_feat0((size_t)n_cam + 1, 0);
    {
        const int64_t n_cells = (int64_t)n_cam * MATCH_CELLS;
        if (n_cells + 1 > n_cell_start) S3P_REFUSE(LBA_E_ARG, "cell_start shorter than n_cam * 64 * 48 + 1");
        if (cell_start[0] != 0) S3P_REFUSE(LBA_E_ARG, "cell_start does not begin at 0");
        for (int64_t c = 0; c < n_cells; ++c)
            if (cell_start[c + 1] < cell_start[c]) S3P_REFUSE(LBA_E_ARG, "cell_start decreases");
        if (cell_start[n_cells] > n_cell_feat) S3P_REFUSE(LBA_E_ARG, "cell_start past the end of cell_feat");
        for (int f = 0; f < n_feats; ++f) {
            if (feats[f].cam < 0 || feats[f].cam >= n_cam || feats[f].octave < 0 || feats[f].octave > 255)
                S3P_REFUSE(LBA_E_ARG, "a feature's camera outside [0, n_cam) or octave outside [0, 255]");
            ++cam_feat0[(size_t)feats[f].cam + 1];
        }
        for (int c = 0; c < n_cam; ++c)
            for (int k = cell_start[(size_t)c * MATCH_CELLS]; k < cell_start[(size_t)(c + 1) * MATCH_CELLS]; ++k)
                if (cell_feat[k] < 0 || cell_feat[k] >= n_feats || feats[cell_feat[k]].cam != c)
                    S3P_REFUSE(LBA_E_ARG, "a cell names a feature outside the keyframe or of another camera");
        int64_t row_end = 0, fp_end = 0, pose_end = 0;
        for (int s = 0; s < n_searches; ++s) {
            const lba_s3p_search& S = searches[s];
            if (!(S.s > 0.0f) || !std::isfinite(S.s)) S3P_REFUSE(LBA_E_ARG, "a search's scale not finite or not positive");
            if (S.n_points < 0 || S.point0 < 0 || (int64_t)S.point0 + S.n_points > n_points)
                S3P_REFUSE(LBA_E_ARG, "a search's points outside the array");
            if (S.taken0 < -1 || (S.taken0 >= 0 && (int64_t)S.taken0 + n_feats > n_taken))
                S3P_REFUSE(LBA_E_ARG, "a search's taken row outside the array");
            if (S.row0 < row_end || (int64_t)S.row0 + (int64_t)S.n_points * n_cam > n_rows)
                S3P_REFUSE(LBA_E_ARG, "a search's rows outside the array or overlapping the search before");
            if (S.featpt0 < fp_end || (int64_t)S.featpt0 + n_feats > n_feat_point)
                S3P_REFUSE(LBA_E_ARG, "a search's feat_point entries outside the array or overlapping the search before");
            if (S.pose0 < pose_end || (int64_t)S.pose0 + n_cam > n_poses)
                S3P_REFUSE(LBA_E_ARG, "a search's poses outside the array or overlapping the search before");
            row_end = (int64_t)S.row0 + (int64_t)S.n_points * n_cam;
            fp_end = (int64_t)S.featpt0 + n_feats;
            pose_end = (int64_t)S.pose0 + n_cam;
        }
        for (int c = 0; c < n_cam; ++c) {
            if (cam_feat0[(size_t)c + 1] > LBA_MATCH_MAX_FEAT) S3P_REFUSE(LBA_E_LIMIT, "more than 8192 features in one camera");
            cam_feat0[(size_t)c + 1] += cam_feat0[c];
        }
    }
    if (n_searches == 0) return LBA_OK;
    std::vector<int> job0((size_t)n_searches + 1, 0);
    for (int s = 0; s < n_searches; ++s) {
        const int64_t end = (int64_t)job0[s] + (int64_t)searches[s].n_points * n_cam;
        if (end > 0x7fffffff) S3P_REFUSE(LBA_E_LIMIT, "the batch exceeds 2 GB");
        job0[(size_t)s + 1] = (int)end;
    }
    const size_t nj = (size_t)job0[n_searches], nf = (size_t)n_feats, ns = (size_t)n_searches, n_sc = ns * (size_t)n_cam;
    if (n_sc > 0x7fffffff || ns * nf > 0x7fffffff) S3P_REFUSE(LBA_E_LIMIT, "the batch exceeds 2 GB");
    if (!K.has_prev) {   // `if (!pKF->mPrevKF) return 0;` (:441): nothing is projected
        for (int s = 0; s < n_searches; ++s) {
            lba_s3p_search& S = searches[s];
            for (int64_t k = 0; k < (int64_t)S.n_points * n_cam; ++k)
                rows[S.row0 + k] = lba_s3p_row{LBA_S3P_NO_PREV, -1, 256, -1, 0.f, 0.f, 0.f, 0};
            for (int f = 0; f < n_feats; ++f) feat_point[S.featpt0 + f] = -1;
            for (int c = 0; c < n_cam; ++c) std::memset(&poses[S.pose0 + c], 0, sizeof(lba_s3p_pose));
            S.n_matches = 0;
        }
        return LBA_OK;
    }
    // ---- the arena: inputs (one upload), outputs (one download; the totals last, they are read back early), work
    ArenaPlan plan;
    const Sec<lba_s3p_kf> o_kf = plan.in<lba_s3p_kf>(1);
    const Sec<lba_s3p_cam> o_kcams = plan.in<lba_s3p_cam>((size_t)n_cam);
    const Sec<lba_match_cam> o_gcams = plan.in<lba_match_cam>((size_t)n_cam);
    const Sec<float> o_sf = plan.in<float>((size_t)K.n_levels);
    const Sec<int32_t> o_cs = plan.in<int32_t>((size_t)n_cam * MATCH_CELLS + 1), o_cf = plan.in<int32_t>((size_t)n_cell_feat);
    const Sec<lba_match_feat> o_feats = plan.in<lba_match_feat>(nf);
    const Sec<int> o_flocal = plan.in<int>(nf), o_cfeats = plan.in<int>(nf), o_cfeat0 = plan.in<int>((size_t)n_cam + 1);
    const Sec<lba_s3p_search> o_searches = plan.in<lba_s3p_search>(ns);
    const Sec<lba_s3p_point> o_points = plan.in<lba_s3p_point>((size_t)n_points);
    const Sec<uint8_t> o_taken = plan.in<uint8_t>((size_t)n_taken);
    const Sec<int> o_job0 = plan.in<int>(ns + 1);
    const Sec<lba_s3p_row> o_rows = plan.out<lba_s3p_row>(nj);
    const Sec<int> o_fp = plan.out<int>(ns * nf);
    const Sec<lba_s3p_pose> o_poses = plan.out<lba_s3p_pose>(n_sc);
    const Sec<int> o_nlive = plan.out<int>(n_sc);
    const Sec<u64> o_ctot = plan.out<u64>(n_sc);
    const Sec<int> o_cap = plan.work<int>(nj);
    const Sec<unsigned> o_loff = plan.work<unsigned>(nj);
    const Sec<int> o_live = plan.work<int>(nj), o_ncand = plan.work<int>(nj);
    const Sec<u64> o_base = plan.work<u64>(n_sc);
    if (plan.over_2gb()) S3P_REFUSE(LBA_E_LIMIT, "the batch exceeds 2 GB");
    char* h = nullptr;
    try {
        ArenaCall call{t, plan, t->s3p_timer};
        h = call.pin();
        *o_kf.at(h) = K;
        std::memcpy(o_kcams.at(h), kcams, (size_t)n_cam * sizeof(lba_s3p_cam));
        std::memcpy(o_gcams.at(h), gcams, (size_t)n_cam * sizeof(lba_match_cam));
        std::memcpy(o_sf.at(h), scale_factors, (size_t)K.n_levels * sizeof(float));
        std::memcpy(o_cs.at(h), cell_start, ((size_t)n_cam * MATCH_CELLS + 1) * sizeof(int32_t));
        if (n_cell_feat) std::memcpy(o_cf.at(h), cell_feat, (size_t)n_cell_feat * sizeof(int32_t));
        if (nf) std::memcpy(o_feats.at(h), feats, nf * sizeof(lba_match_feat));
        std::memcpy(o_searches.at(h), searches, ns * sizeof(lba_s3p_search));
        if (n_points) std::memcpy(o_points.at(h), points, (size_t)n_points * sizeof(lba_s3p_point));
        if (n_taken) std::memcpy(o_taken.at(h), taken, (size_t)n_taken);
        std::memcpy(o_job0.at(h), job0.data(), (ns + 1) * sizeof(int));
        std::memcpy(o_cfeat0.at(h), cam_feat0.data(), ((size_t)n_cam + 1) * sizeof(int));
        {
            int *flocal = o_flocal.at(h), *cfeats = o_cfeats.at(h);
            std::vector<int> fill((size_t)n_cam, 0);
            for (size_t f = 0; f < nf; ++f) {
                const int c = feats[f].cam;
                flocal[f] = fill[c];
                cfeats[cam_feat0[c] + fill[c]++] = (int)f;
            }
        }
        char* d = call.place();
        call.upload();
        S3pArgs a;
        a.kf = o_kf.at(d); a.kcams = o_kcams.at(d); a.gcams = o_gcams.at(d); a.sf = o_sf.at(d);
        a.cell_start = o_cs.at(d); a.cell_feat = o_cf.at(d); a.feats = o_feats.at(d); a.feat_local = o_flocal.at(d);
        a.cam_feats = o_cfeats.at(d); a.cam_feat0 = o_cfeat0.at(d); a.searches = o_searches.at(d);
        a.points = o_points.at(d); a.taken = o_taken.at(d); a.job0 = o_job0.at(d);
        a.rows = o_rows.at(d); a.feat_point = o_fp.at(d); a.poses = o_poses.at(d); a.n_live = o_nlive.at(d);
        a.cap_total = o_ctot.at(d); a.cap = o_cap.at(d); a.loff = o_loff.at(d); a.live = o_live.at(d);
        a.n_cand = o_ncand.at(d); a.base = o_base.at(d); a.cand = nullptr;
        a.n_searches = n_searches; a.n_cam = n_cam; a.n_feats = n_feats; a.n_jobs = (int)nj;
        a.th = P.th; a.th_low = P.th_low; a.proj_form = P.proj_form; a.ratio = P.ratio_hamming; a.max_live = 0;
        hipStream_t st = t->stream;
        call.mark();
        hipLaunchKernelGGL(k_s3p_pose, dim3((unsigned)((n_sc + SP_WG - 1) / SP_WG)), dim3(SP_WG), 0, st, a);
        TR_HIP(hipGetLastError());
        call.mark();
        if (nj) {
            hipLaunchKernelGGL(k_s3p_project, dim3((unsigned)((nj + SP_WG - 1) / SP_WG)), dim3(SP_WG), 0, st, a);
            TR_HIP(hipGetLastError());
        }
        call.mark();
        hipLaunchKernelGGL(k_s3p_compact, dim3((unsigned)n_sc), dim3(SP_WG), 0, st, a);
        TR_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_s3p_base, dim3(1), dim3(SP_WG), 0, st, a);
        TR_HIP(hipGetLastError());
        call.mark();
        // ---- the one readback: live jobs and candidate slots per (search, camera)
        TR_HIP(hipMemcpyAsync(h + o_nlive.off, d + o_nlive.off, plan.down_end - o_nlive.off, hipMemcpyDeviceToHost, st));
        TR_HIP(hipStreamSynchronize(st));
        const int* nlive = o_nlive.at(h);
        const u64* ctot = o_ctot.at(h);
        u64 total = 0;
        int max_live = 0;
        for (size_t i = 0; i < n_sc; ++i) {
            total += ctot[i];
            if (total > (u64(1) << 29)) throw TrackerError{LBA_E_LIMIT, "lba_match_sim3_project: the batch exceeds 2 GB"};
            if (nlive[i] > max_live) max_live = nlive[i];
        }
        if (plan.total() + total * sizeof(uint32_t) > (size_t(1) << 31) || (u64)max_live * n_sc > 0x7fffffffu)
            throw TrackerError{LBA_E_LIMIT, "lba_match_sim3_project: the batch exceeds 2 GB"};
        const size_t cand_bytes = ((size_t)total + 1) * sizeof(uint32_t);
        grow_bytes(t->d_cand, t->cand_cap, cand_bytes, cand_bytes * 2);
        a.cand = reinterpret_cast<uint32_t*>(t->d_cand);
        a.max_live = max_live;
        call.mark();
        if (max_live) {
            hipLaunchKernelGGL(k_s3p_gather, dim3((unsigned)((size_t)max_live * n_sc)), dim3(SG_WG), 0, st, a);
            TR_HIP(hipGetLastError());
        }
        call.mark();
        hipLaunchKernelGGL(k_s3p_resolve, dim3((unsigned)n_sc), dim3(SP_WG), 0, st, a);
        TR_HIP(hipGetLastError());
        call.mark();
        call.finish();
    } catch (const TrackerError& e) {
        return tracker_fail(t, e);
    }
    // ---- scatter: rows, features and poses into the searches' ranges; nmatches
    const lba_s3p_row* r_rows = o_rows.at(h);
    const int* r_fp = o_fp.at(h);
    const lba_s3p_pose* r_poses = o_poses.at(h);
    for (int s = 0; s < n_searches; ++s) {
        lba_s3p_search& S = searches[s];
        const size_t n = (size_t)S.n_points * n_cam;
        if (n) std::memcpy(rows + S.row0, r_rows + job0[s], n * sizeof(lba_s3p_row));
        if (nf) std::memcpy(feat_point + S.featpt0, r_fp + (size_t)s * nf, nf * sizeof(int));
        std::memcpy(poses + S.pose0, r_poses + (size_t)s * n_cam, (size_t)n_cam * sizeof(lba_s3p_pose));
        int m = 0;
        for (size_t k = 0; k < n; ++k) m += r_rows[job0[s] + k].status == LBA_S3P_OK;
        S.n_matches = m;
    }
    return LBA_OK;
}
