// lba_sim3.hip — loop closing's Optimizer::OptimizeSim3 (src/Optimizer.cc:2049-2362) for a batch of candidate pairs.
//
// Per pair: one 7-dof VertexSim3Expmap, fixed points, two 2-d edges per correspondence, optimize(5), the stale-chi2
// outlier pass, optimize(5 or 10) without the robust kernel, the final pass.  The whole flow of a pair runs in ONE
// workgroup of ONE launch (k_sim3), with no host round trip; pairs are independent, so a batch is one workgroup each.
//
// Workgroup size: 64 threads, one wave.  What a trial costs is (a) the edge loop, rows / 64 passes of two edge
// evaluations, (b) the reduction of 28 + 7 + 1 sums and (c) the dependent chain every lane carries alike: a 7 x 7
// damped Cholesky, Sim3(update), the product and g2o's LM controller.  (c) is the same for any workgroup size.
// LoopClosing hands over the BoW matches of one candidate, some tens to about a hundred (it needs 20 to try at
// all): at most two passes of (a) for one wave.  Four waves would quarter (a) only from 256 rows up, where one wave
// makes 4 .. 5 passes, and pay for it in (b) on every trial at every size: partials through LDS and two barriers
// instead of a shuffle tree that needs neither.  With one wave nothing in the LM loop waits on another wave, every
// decision is taken on values that are the same bits on all lanes, and a batch of candidates occupies four times as
// many CUs per thread.  The crossover at 300 rows is not measured (profiles/sim3_bench.txt has one wave's times).
//
// Data: a pair's cameras (Tcb as matrix, intrinsics) and rows (the two body points Y1 = Tc1b^-1 X1c, Y2 = Tc2b^-1 X2c,
// z1, z2, w1, w2, cameras, dropped flag) are read once from global memory into LDS, field-major so that the lanes'
// reads do not collide; lane l owns rows l, l + 64, ...: it alone reads and writes them, in row order, e12 before e21
// as g2o inserts them.  Sums: per lane in row order, then an xor shuffle tree, then lane 0's value broadcast.
// A failed factorisation (non-positive pivot) is a trial with chi2 = max whose state is the untouched one, k_track's
// rule.  No atomics, no inter-workgroup traffic, no spin waits.  Latency-bound like k_track and k_vel_hyp.
// The LM controller's state and rule and the 7 x 7 solve are lba_lm.hpp's (the rule is restated in lm_round, for the
// reason given there), the arena and the error path lba_tracker.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "../../include/amc_lba.h"
#include "lba_lm.hpp"
#include "lba_math.hpp"
#include "lba_tracker.hpp"

using namespace lba;

namespace {

constexpr int S3_WAVE = 64;
constexpr int S3_FIELDS = 12;      // Y1(3) Y2(3) z1(2) z2(2) w1 w2, then two int fields: cameras, dropped
constexpr size_t S3_LDS_MAX = 64 * 1024;
constexpr int S3_MIN_INLIERS = 10; // nCorrespondences - nBad < 10 returns 0 (src/Optimizer.cc:2328)

struct S3Pair {
    double q[4], t[3], s, th2, delta;
    int fix_scale, row0, n, cam0;
};

struct S3Args {
    const S3Pair* pairs;
    const lba_sim3_corr* corr;   // packed: pair p's rows at [row0, row0 + n)
    const lba_sim3_cam* cams;
    double* state;               // out, per pair [8]: q t s
    int* info;                   // out, per pair [4]: n_in, n_bad, iterations, 1 if S12 is written back
    int* flag;                   // out, per packed row
    double tau;
    int max_trials, early_stop, n_cam, stride;   // stride: rows of the largest pair (LDS field pitch)
};

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return __shfl(x, 0);
}
__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

struct S3Ctx {
    const double* cam;   // LDS [2 n_cam][CAMD_N]
    const double* row;   // LDS [S3_FIELDS][stride]
    int* cams12;         // LDS [stride]: cam1 | cam2 << 16
    int* dropped;        // LDS [stride]
    int n, n_cam, stride, lane, fix_scale;
    double th2, delta;
};

// both edges of row i at the state S: errors, e^T Omega e and, if JAC, the Jacobians (2 x 7 each)
template <bool JAC>
__device__ __forceinline__ void row_edges(const S3Ctx& C, const Sim3M& S, int i, double* e12, double* e21, double* c12,
                                          double* c21, double* w, double* J12, double* J21) {
    double f[S3_FIELDS];
#pragma unroll
    for (int k = 0; k < S3_FIELDS; ++k) f[k] = C.row[k * C.stride + i];
    const int cc = C.cams12[i];
    CamD c1, c2;
    camd_load(C.cam + (cc & 0xffff) * CAMD_N, &c1);
    camd_load(C.cam + (C.n_cam + (cc >> 16)) * CAMD_N, &c2);
    sim3_edge12(S, c1, f + 3, f + 6, C.fix_scale != 0, e12, JAC ? J12 : nullptr);
    sim3_edge21(S, c2, f, f + 8, C.fix_scale != 0, e21, JAC ? J21 : nullptr);
    w[0] = f[10]; w[1] = f[11];
    *c12 = e12[0] * (w[0] * e12[0]) + e12[1] * (w[0] * e12[1]);
    *c21 = e21[0] * (w[1] * e21[0]) + e21[1] * (w[1] * e21[1]);
}

// activeRobustChi2 at S over the rows that are not dropped
__device__ double chi_at(const S3Ctx& C, const Sim3& S, bool robust) {
    const Sim3M M = sim3_matrix(S);
    double chi = 0.0;
    for (int i = C.lane; i < C.n; i += S3_WAVE) {
        if (C.dropped[i]) continue;
        double e12[2], e21[2], c12, c21, w[2], r0, r1;
        row_edges<false>(C, M, i, e12, e21, &c12, &c21, w, nullptr, nullptr);
        if (robust) { huber(c12, C.delta, &r0, &r1); chi += r0; huber(c21, C.delta, &r0, &r1); chi += r0; }
        else { chi += c12; chi += c21; }
    }
    return wave_sum(chi);
}

__device__ __forceinline__ void accumulate(const double* J, const double* e, double sw, double* H, double* b) {
#pragma unroll
    for (int a = 0, q = 0; a < 7; ++a)
#pragma unroll
        for (int c = a; c < 7; ++c, ++q) H[q] += sw * (J[a] * J[c] + J[7 + a] * J[7 + c]);
#pragma unroll
    for (int a = 0; a < 7; ++a) b[a] += sw * (J[a] * e[0] + J[7 + a] * e[1]);
}

// optimize(iterations): g2o Levenberg, lambda from computeLambdaInit.
// S: the vertex; last: the state of the last computeActiveErrors (the last trial's, accepted or not).
__device__ int lm_round(const S3Ctx& C, const S3Args& A, Sim3& S, Sim3& last, int iterations, bool robust) {
    LmCtl lm{0.0, 2.0, 0};
    int iters = 0;
    for (int k = 0; k < iterations; ++k) {
        double H[28], b[7], chi = 0.0;
#pragma unroll
        for (int i = 0; i < 28; ++i) H[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 7; ++i) b[i] = 0.0;
        {
            const Sim3M M = sim3_matrix(S);
            for (int i = C.lane; i < C.n; i += S3_WAVE) {
                if (C.dropped[i]) continue;
                double e12[2], e21[2], c12, c21, w[2], J12[14], J21[14], r0, r1;
                row_edges<true>(C, M, i, e12, e21, &c12, &c21, w, J12, J21);
                if (robust) huber(c12, C.delta, &r0, &r1); else { r0 = c12; r1 = 1.0; }
                chi += r0;
                accumulate(J12, e12, r1 * w[0], H, b);   // robustInformation (base_edge.h:96-102)
                if (robust) huber(c21, C.delta, &r0, &r1); else { r0 = c21; r1 = 1.0; }
                chi += r0;
                accumulate(J21, e21, r1 * w[1], H, b);
            }
        }
#pragma unroll
        for (int i = 0; i < 28; ++i) H[i] = wave_sum(H[i]);
#pragma unroll
        for (int i = 0; i < 7; ++i) b[i] = -wave_sum(b[i]);
        double currentChi = wave_sum(chi);
        const double iniChi = currentChi;
        if (k == 0) {
            double m = 0.0;
            for (int a = 0, q = 0; a < 7; q += 7 - a, ++a) m = fmax(m, fabs(H[q]));
            lm = LmCtl{A.tau * m, 2.0, 0};
        }
        double rho = 0.0;
        int qmax = 0;
        do {
            double x[7];
            const int ok = chol_solve<7>(H, lm.lambda, b, x);
            Sim3 St = S;
            if (ok) {
                if (C.fix_scale) x[6] = 0.0;   // oplusImpl (include/OptimizableTypes.h:162-163)
                St = sim3_mul(sim3_exp(x), S);
            }
            last = St;
            double tempChi = chi_at(C, St, robust);
            if (!ok) tempChi = DBL_MAX;
            double scale = 1e-3;
            if (ok)
                for (int i = 0; i < 7; ++i) scale += x[i] * (lm.lambda * x[i] + b[i]);
            // lm_trial and lm_stop (lba_lm.hpp), written out: called as functions they leave this arithmetic as it is
            // but make the compiler round the other product of 2xy - 2wz in chi_at's rotation matrix, and S12 moves
            // by 1e-11.  Keep the two in step with the header.
            rho = (currentChi - tempChi) / scale;
            if (rho > 0 && isfinite(tempChi)) {
                const double t = 2 * rho - 1;
                double alpha = 1. - t * t * t;
                alpha = fmin(alpha, 2. / 3.);
                lm.lambda *= fmax(1. / 3., alpha);
                lm.ni = 2;
                currentChi = tempChi;
                S = St;
            } else {
                lm.lambda *= lm.ni;
                lm.ni *= 2;
            }
            qmax++;
        } while (rho < 0 && qmax < A.max_trials);
        ++iters;
        bool stop = qmax == A.max_trials || rho == 0;
        if (!stop) {
            if ((iniChi - currentChi) * 1e3 < iniChi) lm.nbad++;
            else lm.nbad = 0;
            stop = lm.nbad >= 3;
        }
        if (stop && A.early_stop) break;
    }
    return iters;
}

// e->chi2() of both edges at S: flags the rows with either > th2 (a NaN is not), returns how many of the live rows
__device__ int classify(const S3Ctx& C, const Sim3& S, int* mark) {
    const Sim3M M = sim3_matrix(S);
    int cnt = 0;
    for (int i = C.lane; i < C.n; i += S3_WAVE) {
        if (C.dropped[i]) continue;
        double e12[2], e21[2], c12, c21, w[2];
        row_edges<false>(C, M, i, e12, e21, &c12, &c21, w, nullptr, nullptr);
        const int bad = (c12 > C.th2 || c21 > C.th2) ? 1 : 0;
        mark[i] = bad;
        cnt += bad;
    }
    return wave_sum(cnt);
}

__global__ __launch_bounds__(S3_WAVE) void k_sim3(S3Args A) {
    extern __shared__ double s3_lds[];
    const int p = blockIdx.x, lane = threadIdx.x;
    const S3Pair P = A.pairs[p];
    double* sCam = s3_lds;
    double* sRow = sCam + 2 * A.n_cam * CAMD_N;
    int* sInt = reinterpret_cast<int*>(sRow + (size_t)S3_FIELDS * A.stride);
    S3Ctx C;
    C.cam = sCam; C.row = sRow; C.cams12 = sInt; C.dropped = sInt + A.stride;
    C.n = P.n; C.n_cam = A.n_cam; C.stride = A.stride; C.lane = lane; C.fix_scale = P.fix_scale;
    C.th2 = P.th2; C.delta = P.delta;
    int* final_bad = sInt + 2 * A.stride;

    for (int c = lane; c < 2 * A.n_cam; c += S3_WAVE) {
        const lba_sim3_cam& g = A.cams[P.cam0 + c];
        CamD d;
        sim3_cam_derive(g.q, g.t, g.fx, g.fy, g.cx, g.cy, &d);
        camd_store(d, sCam + c * CAMD_N);
    }
    __syncthreads();
    for (int i = lane; i < P.n; i += S3_WAVE) {
        const lba_sim3_corr& r = A.corr[P.row0 + i];
        CamD c1, c2;
        camd_load(sCam + r.cam1 * CAMD_N, &c1);
        camd_load(sCam + (A.n_cam + r.cam2) * CAMD_N, &c2);
        double f[S3_FIELDS];
        sim3_body_point(c1, r.X1c, f);
        sim3_body_point(c2, r.X2c, f + 3);
        f[6] = r.z1[0]; f[7] = r.z1[1]; f[8] = r.z2[0]; f[9] = r.z2[1]; f[10] = r.w1; f[11] = r.w2;
        for (int k = 0; k < S3_FIELDS; ++k) sRow[k * A.stride + i] = f[k];
        C.cams12[i] = r.cam1 | (r.cam2 << 16);
        C.dropped[i] = 0;
        final_bad[i] = 0;
    }
    __syncthreads();   // (each lane reads back only rows it wrote; the barrier is for the cameras' readers above)

    Sim3 S, last;
    S.q = qnormalize(Quat{P.q[0], P.q[1], P.q[2], P.q[3]});
    S.t[0] = P.t[0]; S.t[1] = P.t[1]; S.t[2] = P.t[2];
    S.s = P.s;
    last = S;
    int n_in = 0, n_bad = 0, iters = 0, wrote = 0;
    if (P.n > 0) {
        iters = lm_round(C, A, S, last, 5, true);
        // first pass: the edges' stale chi2() (:2291-2320); the rows dropped here stay out of every later sum
        n_bad = classify(C, last, C.dropped);
        if (P.n - n_bad >= S3_MIN_INLIERS) {
            iters += lm_round(C, A, S, last, n_bad > 0 ? 10 : 5, false);
            // final pass: computeError() at the estimate (:2336-2355)
            const int late = classify(C, S, final_bad);
            n_in = P.n - n_bad - late;
            wrote = 1;
        }
        for (int i = lane; i < P.n; i += S3_WAVE) A.flag[P.row0 + i] = (C.dropped[i] | final_bad[i]) ? 1 : 0;
    }
    if (lane == 0) {
        double* o = A.state + (size_t)p * 8;
        o[0] = S.q.x; o[1] = S.q.y; o[2] = S.q.z; o[3] = S.q.w;
        o[4] = S.t[0]; o[5] = S.t[1]; o[6] = S.t[2]; o[7] = S.s;
        int* io = A.info + (size_t)p * 4;
        io[0] = n_in; io[1] = n_bad; io[2] = iters; io[3] = wrote;
    }
}

}  // namespace

extern "C" int lba_sim3_profile(lba_tracker* t, int32_t on, double* last_ms) {
    return t ? t->sim3_timer.profile(on, last_ms, 1) : LBA_E_ARG;
}

extern "C" int lba_sim3_optimize(lba_tracker* t, lba_sim3_pair* pairs, int32_t n_pairs, lba_sim3_corr* corr, int32_t n_corr,
                                 const lba_sim3_cam* cams, int32_t n_cam_rows, int32_t n_cam) {
    if (!t || n_pairs < 0 || n_corr < 0 || n_cam_rows < 0 || (n_pairs && !pairs) || (n_corr && !corr) || n_cam < 1 || !cams)
        return LBA_E_ARG;
    if (n_pairs == 0) return LBA_OK;
    if (n_cam > 0x7fff) return LBA_E_ARG;
    // ---- checks first: a refused call writes nothing
    size_t n_rows = 0;
    int stride = 1;
    for (int p = 0; p < n_pairs; ++p) {
        const lba_sim3_pair& P = pairs[p];
        if (P.corr0 < 0 || P.n_corr < 0 || (int64_t)P.corr0 + P.n_corr > n_corr) return LBA_E_ARG;
        if (P.cam0 < 0 || (int64_t)P.cam0 + 2 * (int64_t)n_cam > n_cam_rows) return LBA_E_ARG;
        if (!std::isfinite(P.th2) || !(P.th2 > 0) || !std::isfinite(P.s) || !(P.s > 0)) return LBA_E_ARG;
        for (int i = P.corr0; i < P.corr0 + P.n_corr; ++i)
            if (corr[i].cam1 < 0 || corr[i].cam1 >= n_cam || corr[i].cam2 < 0 || corr[i].cam2 >= n_cam) return LBA_E_ARG;
        n_rows += (size_t)P.n_corr;
        stride = std::max(stride, (int)P.n_corr);
    }
    if (n_rows > 0x7fffffff) return LBA_E_ARG;
    const size_t lds = sizeof(double) * (2 * (size_t)n_cam * CAMD_N + (size_t)S3_FIELDS * stride) + sizeof(int) * 3 * (size_t)stride;
    if (lds > S3_LDS_MAX) return tracker_fail(t, {LBA_E_LIMIT, "a pair's correspondences and cameras exceed 64 KB of LDS"});
    // ---- the arena: inputs (one upload), outputs (one download); its pinned host image has the same offsets
    ArenaPlan plan;
    const Sec<S3Pair> o_pairs = plan.in<S3Pair>((size_t)n_pairs);
    const Sec<lba_sim3_corr> o_rows = plan.in<lba_sim3_corr>(n_rows);
    const Sec<lba_sim3_cam> o_cams = plan.in<lba_sim3_cam>((size_t)n_cam_rows);
    const Sec<double> o_state = plan.out<double>((size_t)n_pairs * 8);
    const Sec<int> o_info = plan.out<int>((size_t)n_pairs * 4), o_flag = plan.out<int>(n_rows);
    char* h = nullptr;
    try {
        ArenaCall call{t, plan, t->sim3_timer};
        h = call.pin();
        // per pair: its rows packed in pair order (overlapping ranges get rows of their own)
        S3Pair* sp = o_pairs.at(h);
        lba_sim3_corr* rows = o_rows.at(h);
        size_t row0 = 0;
        for (int p = 0; p < n_pairs; ++p) {
            const lba_sim3_pair& P = pairs[p];
            S3Pair& D = sp[p];
            std::memcpy(D.q, P.q, sizeof(D.q));
            std::memcpy(D.t, P.t, sizeof(D.t));
            D.s = P.s;
            D.th2 = P.th2;
            D.delta = (double)(float)std::sqrt(P.th2);   // const float deltaHuber = sqrt(th2) (:2115)
            D.fix_scale = P.fix_scale != 0;
            D.row0 = (int)row0;
            D.n = P.n_corr;
            D.cam0 = P.cam0;
            if (P.n_corr) std::memcpy(rows + row0, corr + P.corr0, (size_t)P.n_corr * sizeof(lba_sim3_corr));
            row0 += (size_t)P.n_corr;
        }
        std::memcpy(o_cams.at(h), cams, (size_t)n_cam_rows * sizeof(lba_sim3_cam));
        char* d = call.place();
        call.upload();
        S3Args a;
        a.pairs = o_pairs.at(d); a.corr = o_rows.at(d); a.cams = o_cams.at(d);
        a.state = o_state.at(d); a.info = o_info.at(d); a.flag = o_flag.at(d);
        a.tau = t->cfg.tau; a.max_trials = t->cfg.max_trials; a.early_stop = t->cfg.early_stop;
        a.n_cam = n_cam; a.stride = stride;
        call.mark();
        hipLaunchKernelGGL(k_sim3, dim3((unsigned)n_pairs), dim3(S3_WAVE), lds, t->stream, a);
        TR_HIP(hipGetLastError());
        call.mark();
        call.finish();
    } catch (const TrackerError& e) {
        return tracker_fail(t, e);
    }
    const S3Pair* sp = o_pairs.at(h);
    const double* r_state = o_state.at(h);
    const int *r_info = o_info.at(h), *r_flag = o_flag.at(h);
    for (int p = 0; p < n_pairs; ++p) {
        lba_sim3_pair& P = pairs[p];
        const int* io = r_info + (size_t)p * 4;
        P.n_in = io[0]; P.n_bad = io[1]; P.iterations = io[2];
        if (io[3]) {
            const double* st = r_state + (size_t)p * 8;
            std::memcpy(P.q, st, 4 * sizeof(double));
            std::memcpy(P.t, st + 4, 3 * sizeof(double));
            P.s = st[7];
        }
        for (int i = 0; i < P.n_corr; ++i) corr[P.corr0 + i].outlier = r_flag[sp[p].row0 + i];
    }
    return LBA_OK;
}
