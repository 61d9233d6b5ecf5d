// lba_sim3_ransac.hip — loop closing's Sim3Solver RANSAC (src/Sim3Solver.cc:250-326, :343-536; called from
// LoopClosing.cc:527-539) for a batch of candidate pairs, the step before lba_sim3_optimize.
//
// A hypothesis is Horn's closed-form alignment of three sampled point pairs (lba_s3r_math.hpp) followed by two
// reprojections of every correspondence of its pair.  Hypotheses are independent, so k_s3r_hyp gives ONE WAVE to each
// hypothesis of the whole batch, the shape of k_vel_hyp: the three sampled rows are read uniformly and every lane
// carries the same Horn solve in registers (a fixed-sweep Jacobi: nothing diverges, nothing loops on data); lane l then
// scores rows l, l + 64, ...; one ballot per 64 rows is both the stored inlier-mask word and, by popcount, the count.
// No floating-point reduction anywhere: the only sums are Horn's 3-term ones in fixed order.  k_s3r_select (one wave
// per pair, same stream) restates the sequential selection of iterate() over the counts and expands the chosen mask.
// Nothing waits on another workgroup; the two launches in stream order are the only ordering; no result depends on
// the batch, the grid or a pair's position.  Latency- and launch-bound.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/amc_lba.h"
#include "lba_math.hpp"
#include "lba_s3r_math.hpp"
#include "lba_tracker.hpp"

using namespace lba;

namespace {

constexpr int S3R_WAVE = 64;
constexpr int S3R_MAX_CAM = 64;   // per keyframe: 2 * 64 camera records of CAMD_N doubles are 16 KB of LDS

struct S3RPair {
    int row0, n;        // its rows of the packed correspondences
    int cam0;           // its 2 n_cam cameras
    int work0, n_hyp;   // its hypotheses among the work items
    int words;          // 64-bit mask words per hypothesis: ceil(n / 64)
    int fix_scale, min_inliers;
    long long mask0;    // its first mask word
};

struct S3RArgs {
    const S3RPair* pairs;
    const lba_s3r_corr* corr;   // packed: pair p's rows at [row0, row0 + n)
    const lba_sim3_cam* cams;
    const int* tri;             // per work item: its three pair-local rows, in the caller's order
    const int* work_pair;       // per work item: its pair
    double* hyp_S12;            // out, per work item [8]: q t s
    int* hyp_inl;               // out, per work item
    int* hyp_flag;              // out, per work item: LBA_S3R_DEGENERATE | LBA_S3R_NONFINITE
    double* state;              // out, per pair [8]
    int* info;                  // out, per pair [4]: best_hyp, n_inliers, converged
    int* inlier;                // out, per packed row
    unsigned long long* mask;   // per work item `words` ballots of the scoring pass
    int n_cam;
};

__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o));
    return x;
}

__global__ __launch_bounds__(S3R_WAVE) void k_s3r_hyp(S3RArgs A) {
    extern __shared__ double s3r_cam[];   // [2 n_cam][CAMD_N]
    const int w = blockIdx.x, lane = threadIdx.x;
    const S3RPair P = A.pairs[A.work_pair[w]];
    for (int c = lane; c < 2 * A.n_cam; c += S3R_WAVE) {
        const lba_sim3_cam& g = A.cams[P.cam0 + c];
        CamD d;
        sim3_cam_derive(g.q, g.t, g.fx, g.fy, g.cx, g.cy, &d);
        camd_store(d, s3r_cam + c * CAMD_N);
    }
    // ---- ComputeSim3 on the sampled triple: the same on every lane
    double X1[9], X2[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const lba_s3r_corr& r = A.corr[P.row0 + A.tri[3 * w + j]];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            X1[3 * j + i] = r.X1b[i];
            X2[3 * j + i] = r.X2b[i];
        }
    }
    S3RHyp H;
    s3r_horn(X1, X2, P.fix_scale != 0, &H);
    __syncthreads();
    // ---- CheckInliers on every row of the pair; a degenerate hypothesis is skipped and keeps an empty mask
    int count = 0;
    unsigned long long* mask = A.mask + P.mask0 + (long long)(w - P.work0) * P.words;
    for (int base = 0; base < P.n; base += S3R_WAVE) {
        const int i = base + lane;
        bool in = false;
        if (i < P.n && !H.degenerate) {
            const lba_s3r_corr& r = A.corr[P.row0 + i];
            CamD c1, c2;
            camd_load(s3r_cam + r.cam1 * CAMD_N, &c1);
            camd_load(s3r_cam + (A.n_cam + r.cam2) * CAMD_N, &c2);
            double err[2];
            s3r_errors(H, c1, c2, r.X1b, r.X2b, err);
            in = err[0] < r.max_err1 && err[1] < r.max_err2;   // strict; false for a NaN error
        }
        const unsigned long long m = __ballot(in);
        count += __popcll(m);
        if (lane == 0) mask[base / S3R_WAVE] = m;
    }
    if (lane == 0) {
        double* o = A.hyp_S12 + (size_t)w * 8;
        bool finite = isfinite(H.s);
#pragma unroll
        for (int i = 0; i < 4; ++i) { o[i] = H.q[i]; finite = finite && isfinite(H.q[i]); }
#pragma unroll
        for (int i = 0; i < 3; ++i) { o[4 + i] = H.t[i]; finite = finite && isfinite(H.t[i]); }
        o[7] = H.s;
        A.hyp_inl[w] = count;
        A.hyp_flag[w] = (H.degenerate ? LBA_S3R_DEGENERATE : 0) | (finite ? 0 : LBA_S3R_NONFINITE);
    }
}

// iterate() (:272-325) over the counts of a pair, in hypothesis order, degenerate hypotheses skipped: the first count
// > min_inliers converges and is selected; otherwise the last count that is >= every earlier one, which is the last
// hypothesis that attains the maximum.
__global__ __launch_bounds__(S3R_WAVE) void k_s3r_select(S3RArgs A) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const S3RPair P = A.pairs[p];
    int best = -1, converged = 0;
    for (int base = 0; base < P.n_hyp; base += S3R_WAVE) {
        const int h = base + lane;
        const bool hit = h < P.n_hyp && !(A.hyp_flag[P.work0 + h] & LBA_S3R_DEGENERATE) && A.hyp_inl[P.work0 + h] > P.min_inliers;
        const unsigned long long m = __ballot(hit);
        if (m) {
            best = base + __ffsll((long long)m) - 1;
            converged = 1;
            break;
        }
    }
    if (!converged) {
        int top = -1;
        for (int h = lane; h < P.n_hyp; h += S3R_WAVE)
            if (!(A.hyp_flag[P.work0 + h] & LBA_S3R_DEGENERATE)) top = max(top, A.hyp_inl[P.work0 + h]);
        top = wave_max(top);
        int last = -1;
        for (int h = lane; h < P.n_hyp; h += S3R_WAVE)
            if (!(A.hyp_flag[P.work0 + h] & LBA_S3R_DEGENERATE) && A.hyp_inl[P.work0 + h] == top) last = h;
        best = wave_max(last);
    }
    const unsigned long long* mask = A.mask + P.mask0 + (long long)(best < 0 ? 0 : best) * P.words;
    for (int i = lane; i < P.n; i += S3R_WAVE)
        A.inlier[P.row0 + i] = best < 0 ? 0 : (int)((mask[i / S3R_WAVE] >> (i % S3R_WAVE)) & 1ull);
    if (lane == 0) {
        double* o = A.state + (size_t)p * 8;
        for (int i = 0; i < 8; ++i) o[i] = best < 0 ? 0.0 : A.hyp_S12[(size_t)(P.work0 + best) * 8 + i];
        int* io = A.info + (size_t)p * 4;
        io[0] = best;
        io[1] = best < 0 ? 0 : A.hyp_inl[P.work0 + best];
        io[2] = converged;
        io[3] = 0;
    }
}

}  // namespace

extern "C" int lba_sim3_ransac_profile(lba_tracker* t, int32_t on, double* last_ms) {
    return t ? t->s3r_timer.profile(on, last_ms, 1) : LBA_E_ARG;
}

extern "C" int lba_sim3_ransac(lba_tracker* t, lba_s3r_pair* pairs, int32_t n_pairs, lba_s3r_corr* corr, int32_t n_corr,
                               const int32_t* samples, int32_t n_hyp, const lba_sim3_cam* cams, int32_t n_cam_rows,
                               int32_t n_cam, double* hyp_S12, int32_t* hyp_inliers, int32_t* hyp_flags) {
    if (!t || n_pairs < 0 || n_corr < 0 || n_hyp < 0 || n_cam_rows < 0 || (n_pairs && !pairs) || (n_corr && !corr) ||
        (n_hyp && !samples) || n_cam < 1 || !cams)
        return LBA_E_ARG;
    if (n_pairs == 0) return LBA_OK;
    if (n_cam > S3R_MAX_CAM) return tracker_fail(t, {LBA_E_LIMIT, "more than 64 cameras per keyframe"});
    // ---- checks first: a refused call writes nothing
    size_t n_rows = 0, n_work = 0;
    long long words = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const lba_s3r_pair& P = pairs[p];
        if (P.corr0 < 0 || P.n_corr < 0 || (int64_t)P.corr0 + P.n_corr > n_corr) return LBA_E_ARG;
        if (P.hyp0 < 0 || P.n_hyp < 0 || (int64_t)P.hyp0 + P.n_hyp > n_hyp) return LBA_E_ARG;
        if (P.cam0 < 0 || (int64_t)P.cam0 + 2 * (int64_t)n_cam > n_cam_rows) return LBA_E_ARG;
        if (P.min_inliers < 0) return LBA_E_ARG;
        for (int i = P.corr0; i < P.corr0 + P.n_corr; ++i) {
            const lba_s3r_corr& r = corr[i];
            if (r.cam1 < 0 || r.cam1 >= n_cam || r.cam2 < 0 || r.cam2 >= n_cam) return LBA_E_ARG;
            if (std::isnan(r.max_err1) || std::isnan(r.max_err2)) return LBA_E_ARG;
        }
        for (int h = P.hyp0; h < P.hyp0 + P.n_hyp; ++h) {
            const int32_t* s3 = samples + (size_t)3 * h;
            for (int j = 0; j < 3; ++j)
                if (s3[j] < 0 || s3[j] >= P.n_corr) return LBA_E_ARG;
            if (s3[0] == s3[1] || s3[1] == s3[2] || s3[0] == s3[2]) return LBA_E_ARG;
        }
        n_rows += (size_t)P.n_corr;
        n_work += (size_t)P.n_hyp;
        words += (long long)P.n_hyp * ((P.n_corr + S3R_WAVE - 1) / S3R_WAVE);
    }
    // ---- the arena: inputs (one upload), outputs (one download), masks (device only); its pinned host image has
    // the same offsets
    ArenaPlan plan;
    const Sec<S3RPair> o_pairs = plan.in<S3RPair>((size_t)n_pairs);
    const Sec<lba_s3r_corr> o_rows = plan.in<lba_s3r_corr>(n_rows);
    const Sec<lba_sim3_cam> o_cams = plan.in<lba_sim3_cam>((size_t)n_cam_rows);
    const Sec<int> o_tri = plan.in<int>(n_work * 3), o_work = plan.in<int>(n_work);
    const Sec<double> o_hS = plan.out<double>(n_work * 8);
    const Sec<int> o_hinl = plan.out<int>(n_work), o_hflag = plan.out<int>(n_work);
    const Sec<double> o_state = plan.out<double>((size_t)n_pairs * 8);
    const Sec<int> o_info = plan.out<int>((size_t)n_pairs * 4), o_inl = plan.out<int>(n_rows);
    const Sec<unsigned long long> o_mask = plan.work<unsigned long long>((size_t)words);
    if (n_rows > 0x7fffffff || n_work > 0x7fffffff || plan.over_2gb())
        return tracker_fail(t, {LBA_E_LIMIT, "the batch's rows, hypotheses and inlier masks exceed 2 GB"});
    char* h = nullptr;
    try {
        ArenaCall call{t, plan, t->s3r_timer};
        h = call.pin();
        // per pair: its rows packed in pair order (overlapping ranges get rows of their own), its triples as work items
        S3RPair* sp = o_pairs.at(h);
        lba_s3r_corr* rows = o_rows.at(h);
        int *tri = o_tri.at(h), *work_pair = o_work.at(h);
        size_t row0 = 0, work0 = 0;
        long long mask0 = 0;
        for (int p = 0; p < n_pairs; ++p) {
            const lba_s3r_pair& P = pairs[p];
            S3RPair& D = sp[p];
            D.row0 = (int)row0; D.n = P.n_corr;
            D.cam0 = P.cam0;
            D.work0 = (int)work0; D.n_hyp = P.n_hyp;
            D.words = (P.n_corr + S3R_WAVE - 1) / S3R_WAVE;
            D.fix_scale = P.fix_scale != 0; D.min_inliers = P.min_inliers;
            D.mask0 = mask0;
            if (P.n_corr) std::memcpy(rows + row0, corr + P.corr0, (size_t)P.n_corr * sizeof(lba_s3r_corr));
            if (P.n_hyp) std::memcpy(tri + 3 * work0, samples + (size_t)3 * P.hyp0, (size_t)P.n_hyp * 3 * sizeof(int));
            for (int k = 0; k < P.n_hyp; ++k) work_pair[work0 + k] = p;
            row0 += (size_t)P.n_corr;
            work0 += (size_t)P.n_hyp;
            mask0 += (long long)P.n_hyp * D.words;
        }
        std::memcpy(o_cams.at(h), cams, (size_t)n_cam_rows * sizeof(lba_sim3_cam));
        char* d = call.place();
        call.upload();
        S3RArgs a;
        a.pairs = o_pairs.at(d); a.corr = o_rows.at(d); a.cams = o_cams.at(d);
        a.tri = o_tri.at(d); a.work_pair = o_work.at(d);
        a.hyp_S12 = o_hS.at(d); a.hyp_inl = o_hinl.at(d); a.hyp_flag = o_hflag.at(d);
        a.state = o_state.at(d); a.info = o_info.at(d); a.inlier = o_inl.at(d);
        a.mask = o_mask.at(d);
        a.n_cam = n_cam;
        const size_t lds = sizeof(double) * 2 * (size_t)n_cam * CAMD_N;
        hipStream_t s = t->stream;
        call.mark();
        if (n_work) hipLaunchKernelGGL(k_s3r_hyp, dim3((unsigned)n_work), dim3(S3R_WAVE), lds, s, a);
        hipLaunchKernelGGL(k_s3r_select, dim3((unsigned)n_pairs), dim3(S3R_WAVE), 0, s, a);
        TR_HIP(hipGetLastError());
        call.mark();
        call.finish();
    } catch (const TrackerError& e) {
        return tracker_fail(t, e);
    }
    const S3RPair* sp = o_pairs.at(h);
    const double *r_hS = o_hS.at(h), *r_state = o_state.at(h);
    const int *r_hinl = o_hinl.at(h), *r_hflag = o_hflag.at(h), *r_info = o_info.at(h), *r_inl = o_inl.at(h);
    for (int p = 0; p < n_pairs; ++p) {
        lba_s3r_pair& P = pairs[p];
        const S3RPair& D = sp[p];
        const int* io = r_info + (size_t)p * 4;
        P.best_hyp = io[0]; P.n_inliers = io[1]; P.converged = io[2];
        if (P.best_hyp >= 0) {
            const double* st = r_state + (size_t)p * 8;
            std::memcpy(P.q, st, 4 * sizeof(double));
            std::memcpy(P.t, st + 4, 3 * sizeof(double));
            P.s = st[7];
        }
        for (int i = 0; i < P.n_corr; ++i) corr[P.corr0 + i].inlier = r_inl[D.row0 + i];
        for (int k = 0; k < P.n_hyp; ++k) {
            const size_t g = (size_t)P.hyp0 + k, w = (size_t)D.work0 + k;
            if (hyp_S12) std::memcpy(hyp_S12 + g * 8, r_hS + w * 8, 8 * sizeof(double));
            if (hyp_inliers) hyp_inliers[g] = r_hinl[w];
            if (hyp_flags) hyp_flags[g] = r_hflag[w];
        }
    }
    return LBA_OK;
}
