// lba_track_vel.hip — the hypotheses of Tracking::MCRansac (src/Tracking.cc:1939-2002) on the GPU: one
// Optimizer::OptimizeVel (src/Optimizer.cc:2364-2447) per sampled triple, the step before lba_track.
//
// A hypothesis is a 6-dof velocity fitted to three EdgeVelReproj edges by optimize(40) of g2o's Levenberg (the
// controller and the 6 x 6 solve of lba_lm.hpp, the arena of lba_tracker.hpp: DESIGN.md §7 item 8) and then
// scored on every matched feature of the frame.  Hypotheses are independent and each is a short dependent chain on
// a 6 x 6 system, so k_vel_hyp gives ONE WAVE to each hypothesis of the batch: lanes 0..2 hold the three edges
// (error, Jacobian, Huber weight), H and b are their sums broadcast in the edges' order, and every lane carries the
// same 6 x 6 damped Cholesky solve and LM controller in registers, so the wave never diverges on a decision and
// needs no hand-off.  exp(v dt) is evaluated once per distinct (cam, dt) of the frame and per trial state, by one
// lane each, into LDS.  The scoring pass runs all 64 lanes over the frame's observations; a ballot per 64
// observations is both the inlier mask (kept for the selection) and, by popcount, the count: no floating-point
// reduction, one fixed order.  k_vel_select (one wave per frame, same stream) picks the first hypothesis with
// strictly more inliers than every earlier one and writes its velocity and flags.  Nothing waits on another
// workgroup, and no result depends on the batch or the grid.  Latency-bound like k_track.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_lm.hpp"
#include "lba_math.hpp"
#include "lba_tracker.hpp"

using namespace lba;

namespace {

constexpr int VEL_WAVE = 64;

struct VelFrame {
    double q[4], t[3], vel[6];
    int obs0, n_obs;      // its observations in `obs`
    int smp0, n_smp;      // its distinct (cam, dt) in smp_dt
    int work0, n_hyp;     // its hypotheses among the work items
    int row0;             // its first row of the packed inlier flags
    int words;            // 64-bit mask words per hypothesis: ceil(n_obs / 64)
    long long mask0;      // its first mask word
};

struct VelArgs {
    const VelFrame* frames;
    const lba_vel_obs* obs;
    const int* obs_smp;        // per observation: the frame-local (cam, dt) index
    const double* smp_dt;      // per (cam, dt)
    const int* tri;            // per work item: its three frame-local observation indices, ascending
    const int* work_frame;     // per work item: its frame
    const double* camd;        // [n_cam][CAMD_N]
    double* hyp_vel;           // out, per work item [6]
    int* hyp_inl;              // out, per work item
    int* hyp_it;               // out, per work item
    double* frame_vel;         // out, per frame [6]
    int* frame_best;           // out, per frame [2]: best hypothesis (frame-local) or -1, its inliers
    int* inlier;               // out, per packed row
    unsigned long long* mask;  // per work item `words` ballots of the scoring pass
    double threshold, huber_delta, tau;
    int iterations, max_trials, early_stop;
};

// T^-1 of the last frame's pose (Sophus cast<double>(): normalised quaternion)
__device__ __forceinline__ SE3 frame_inverse(const VelFrame& F) {
    SE3 T;
    T.q = qnormalize(Quat{F.q[0], F.q[1], F.q[2], F.q[3]});
    T.t[0] = F.t[0]; T.t[1] = F.t[1]; T.t[2] = F.t[2];
    return se3_inv(T);
}

__device__ __forceinline__ void body_point(const SE3& Ti, const double* Xw, double* Xb) {
    qrot(Ti.q, Xw, Xb);
    Xb[0] += Ti.t[0]; Xb[1] += Ti.t[1]; Xb[2] += Ti.t[2];
}

// exp(v dt) of every (cam, dt) of the frame at the state v: one lane each
__device__ __forceinline__ void motions(const VelArgs& A, const VelFrame& F, const double* v, double (*sM)[12]) {
    __syncthreads();   // the readers of the last state are done
    const int si = threadIdx.x;
    if (si < F.n_smp) vel_motion(v, A.smp_dt[F.smp0 + si], sM[si], sM[si] + 9);
    __syncthreads();
}

// the three edges' sum, in their order, on every lane
__device__ __forceinline__ double sum3(double x) {
    return (__shfl(x, 0) + __shfl(x, 1)) + __shfl(x, 2);
}

__global__ __launch_bounds__(VEL_WAVE) void k_vel_hyp(VelArgs A) {
    __shared__ double sM[TR_MAXS][12];   // exp(v dt) per (cam, dt): Rp(9) tp(3)
    const int w = blockIdx.x, lane = threadIdx.x;
    const VelFrame& F = A.frames[A.work_frame[w]];
    const SE3 Ti = frame_inverse(F);
    // this lane's edge of the triple (lanes 3.. repeat edge 0; sum3 never reads them)
    const int eo = F.obs0 + A.tri[LBA_VEL_SET * w + (lane < LBA_VEL_SET ? lane : 0)];
    const lba_vel_obs eob = A.obs[eo];
    const int es = A.obs_smp[eo];
    CamD ecd;
    camd_load(A.camd + (size_t)eob.cam * CAMD_N, &ecd);
    double eXb[3];
    body_point(Ti, eob.Xw, eXb);

    double v[6];
    for (int i = 0; i < 6; ++i) v[i] = F.vel[i];
    // ---- optimize(iterations): g2o Levenberg, lambda from computeLambdaInit, on the three level-0 edges
    LmCtl lm{0.0, 2.0, 0};
    int iters = 0;
    for (int k = 0; k < A.iterations; ++k) {
        motions(A, F, v, sM);
        double e[2], Xc[3], J[12], H[21], b[6], r0, r1;
        vel_reproj_error(sM[es], sM[es] + 9, ecd, eXb, eob.z, Xc, e);
        vel_reproj_jac(v, eob.dt, sM[es], ecd, eXb, Xc, J);
        huber(e[0] * (eob.w * e[0]) + e[1] * (eob.w * e[1]), A.huber_delta, &r0, &r1);
        const double sw = r1 * eob.w;   // robustInformation (base_edge.h:96-102)
#pragma unroll
        for (int a = 0, q = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c, ++q) H[q] = sum3(sw * (J[a] * J[c] + J[6 + a] * J[6 + c]));
#pragma unroll
        for (int a = 0; a < 6; ++a) b[a] = -sum3(sw * (J[a] * e[0] + J[6 + a] * e[1]));
        double currentChi = sum3(r0);
        const double iniChi = currentChi;
        if (k == 0) {
            double m = 0.0;
            for (int a = 0, q = 0; a < 6; q += 6 - a, ++a) m = fmax(m, fabs(H[q]));
            lm = LmCtl{A.tau * m, 2.0, 0};
        }
        double rho = 0.0;
        int qmax = 0;
        do {
            double x[6], vt[6];
            const int ok = chol_solve<6>(H, lm.lambda, b, x);
            for (int i = 0; i < 6; ++i) vt[i] = ok ? v[i] + x[i] : v[i];
            motions(A, F, vt, sM);
            vel_reproj_error(sM[es], sM[es] + 9, ecd, eXb, eob.z, Xc, e);
            huber(e[0] * (eob.w * e[0]) + e[1] * (eob.w * e[1]), A.huber_delta, &r0, &r1);
            double tempChi = sum3(r0);
            if (!ok) tempChi = DBL_MAX;
            double scale = 1e-3;
            if (ok)
                for (int i = 0; i < 6; ++i) scale += x[i] * (lm.lambda * x[i] + b[i]);
            bool accept;
            rho = lm_trial(lm, currentChi, tempChi, scale, accept);
            if (accept)
                for (int i = 0; i < 6; ++i) v[i] = vt[i];
            qmax++;
        } while (rho < 0 && qmax < A.max_trials);
        ++iters;
        if (lm_stop(lm, iniChi, currentChi, rho, qmax, A.max_trials) && A.early_stop) break;
    }
    // ---- computeError() on every edge of the frame: inlier iff ||e|| <= threshold (Optimizer.cc:2425-2440)
    motions(A, F, v, sM);
    int count = 0;
    unsigned long long* mask = A.mask + F.mask0 + (long long)(w - F.work0) * F.words;
    for (int base = 0; base < F.n_obs; base += VEL_WAVE) {
        const int i = base + lane;
        bool in = false;
        if (i < F.n_obs) {
            const lba_vel_obs& ob = A.obs[F.obs0 + i];
            const int s = A.obs_smp[F.obs0 + i];
            CamD cd;
            camd_load(A.camd + (size_t)ob.cam * CAMD_N, &cd);
            double Xb[3], Xc[3], e[2];
            body_point(Ti, ob.Xw, Xb);
            vel_reproj_error(sM[s], sM[s] + 9, cd, Xb, ob.z, Xc, e);
            in = sqrt(e[0] * e[0] + e[1] * e[1]) <= A.threshold;   // (false for a NaN error)
        }
        const unsigned long long m = __ballot(in);
        count += __popcll(m);
        if (lane == 0) mask[base / VEL_WAVE] = m;
    }
    if (lane == 0) {
        for (int i = 0; i < 6; ++i) A.hyp_vel[(size_t)w * 6 + i] = v[i];
        A.hyp_inl[w] = count;
        A.hyp_it[w] = iters;
    }
}

// Tracking.cc:1978-1984 per frame: the first hypothesis with strictly more inliers than every earlier one
__global__ __launch_bounds__(VEL_WAVE) void k_vel_select(VelArgs A) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const VelFrame& F = A.frames[f];
    int best = -1, best_n = 0;
    for (int h = 0; h < F.n_hyp; ++h) {
        const int n = A.hyp_inl[F.work0 + h];
        if (n > best_n) { best_n = n; best = h; }
    }
    const unsigned long long* mask = A.mask + F.mask0 + (long long)(best < 0 ? 0 : best) * F.words;
    for (int i = lane; i < F.n_obs; i += VEL_WAVE)
        A.inlier[F.row0 + i] = best < 0 ? 0 : (int)((mask[i / VEL_WAVE] >> (i % VEL_WAVE)) & 1ull);
    if (lane == 0) {
        for (int i = 0; i < 6; ++i) A.frame_vel[(size_t)f * 6 + i] = best < 0 ? F.vel[i] : A.hyp_vel[(size_t)(F.work0 + best) * 6 + i];
        A.frame_best[2 * f] = best;
        A.frame_best[2 * f + 1] = best_n;
    }
}

}  // namespace

extern "C" int lba_track_vel_ransac(lba_tracker* t, lba_vel_frame* frames, int32_t n_frames, lba_vel_obs* obs, int32_t n_obs,
                                    const int32_t* samples, int32_t n_hyp, const lba_vel_params* prm, const lba_cam* cams,
                                    int32_t n_cam, double* hyp_vel, int32_t* hyp_inliers, int32_t* hyp_iterations) {
    if (!t || n_frames < 0 || n_obs < 0 || n_hyp < 0 || (n_frames && !frames) || (n_obs && !obs) || (n_hyp && !samples) ||
        n_cam < 1 || !cams)
        return LBA_E_ARG;
    lba_vel_params P{2.0, 5.991, 40, 0};   // OptimizeVel's threshold, rk->setDelta(5.991), optimize(40)
    if (prm) P = *prm;
    if (P.iterations < 0) return LBA_E_ARG;
    if (n_frames == 0) return LBA_OK;
    // ---- per frame: its distinct (cam, dt), the observations' index into them, its triples in ascending order
    std::vector<VelFrame> vf(n_frames);
    std::vector<int> obs_smp((size_t)n_obs, 0), tri, work_frame;
    std::vector<double> smp_dt;
    int rows = 0;
    long long words = 0;
    for (int f = 0; f < n_frames; ++f) {
        const lba_vel_frame& F = frames[f];
        if (F.obs0 < 0 || F.n_obs < 0 || (int64_t)F.obs0 + F.n_obs > n_obs) return LBA_E_ARG;
        if (F.hyp0 < 0 || F.n_hyp < 0 || (int64_t)F.hyp0 + F.n_hyp > n_hyp) return LBA_E_ARG;
        // (at most TR_MAXS distinct pairs: a linear search per observation instead of a sort of them all)
        std::pair<int, double> cd[TR_MAXS];
        int ncd = 0;
        bool over = false;
        for (int i = F.obs0; i < F.obs0 + F.n_obs; ++i) {
            if (obs[i].cam < 0 || obs[i].cam >= n_cam || !std::isfinite(obs[i].dt)) return LBA_E_ARG;
            const std::pair<int, double> key((int)obs[i].cam, obs[i].dt);
            if (std::find(cd, cd + ncd, key) != cd + ncd) continue;
            if (ncd == TR_MAXS) over = true;
            else cd[ncd++] = key;
        }
        if (over) return tracker_fail(t, {LBA_E_LIMIT, "more than 16 distinct (camera, dt) pairs in a frame"});
        std::sort(cd, cd + ncd);
        for (int i = F.obs0; i < F.obs0 + F.n_obs; ++i)
            obs_smp[i] = (int)(std::find(cd, cd + ncd, std::make_pair((int)obs[i].cam, obs[i].dt)) - cd);
        VelFrame& V = vf[f];
        std::memcpy(V.q, F.q, sizeof(V.q));
        std::memcpy(V.t, F.t, sizeof(V.t));
        std::memcpy(V.vel, F.vel, sizeof(V.vel));
        V.obs0 = F.obs0; V.n_obs = F.n_obs;
        V.smp0 = (int)smp_dt.size(); V.n_smp = ncd;
        V.work0 = (int)work_frame.size(); V.n_hyp = F.n_hyp;
        V.row0 = rows;
        V.words = (F.n_obs + VEL_WAVE - 1) / VEL_WAVE;
        V.mask0 = words;
        for (int j = 0; j < ncd; ++j) smp_dt.push_back(cd[j].second);
        for (int h = F.hyp0; h < F.hyp0 + F.n_hyp; ++h) {
            int s3[LBA_VEL_SET];
            for (int j = 0; j < LBA_VEL_SET; ++j) {
                s3[j] = samples[(size_t)LBA_VEL_SET * h + j];
                if (s3[j] < 0 || s3[j] >= F.n_obs) return LBA_E_ARG;
            }
            std::sort(s3, s3 + LBA_VEL_SET);
            if (s3[0] == s3[1] || s3[1] == s3[2]) return LBA_E_ARG;
            tri.insert(tri.end(), s3, s3 + LBA_VEL_SET);
            work_frame.push_back(f);
        }
        rows += F.n_obs;
        words += (long long)F.n_hyp * V.words;
    }
    const size_t n_work = work_frame.size();
    // ---- the arena: inputs (one upload), outputs (one download), masks (device only)
    ArenaImage in;
    const Sec<VelFrame> o_frames = in.put(vf);
    const Sec<lba_vel_obs> o_obs = in.put(obs, (size_t)n_obs);
    const Sec<int> o_obs_smp = in.put(obs_smp);
    const Sec<double> o_smp_dt = in.put(smp_dt);
    const Sec<int> o_tri = in.put(tri), o_work = in.put(work_frame);
    const Sec<double> o_camd = in.put(camd_pack(cams, n_cam));
    ArenaLayout& lay = in.lay;
    const size_t out0 = lay.total;
    const Sec<double> o_hvel = lay.take<double>(n_work * 6), o_fvel = lay.take<double>((size_t)n_frames * 6);
    const Sec<int> o_hinl = lay.take<int>(n_work), o_hit = lay.take<int>(n_work);
    const Sec<int> o_best = lay.take<int>((size_t)n_frames * 2), o_inl = lay.take<int>((size_t)rows);
    const size_t out1 = lay.total;
    const Sec<unsigned long long> o_mask = lay.take<unsigned long long>((size_t)words);
    std::vector<char> out(out1 - out0);
    try {
        TR_HIP(hipSetDevice(t->cfg.device));
        grow_bytes(t->d_arena, t->arena_cap, lay.total, lay.total * 2);
        char* d = t->d_arena;
        hipStream_t s = t->stream;
        TR_HIP(hipMemcpyAsync(d, in.bytes.data(), in.bytes.size(), hipMemcpyHostToDevice, s));
        VelArgs a;
        a.frames = o_frames.at(d); a.obs = o_obs.at(d); a.obs_smp = o_obs_smp.at(d); a.smp_dt = o_smp_dt.at(d);
        a.tri = o_tri.at(d); a.work_frame = o_work.at(d); a.camd = o_camd.at(d);
        a.hyp_vel = o_hvel.at(d); a.frame_vel = o_fvel.at(d); a.hyp_inl = o_hinl.at(d); a.hyp_it = o_hit.at(d);
        a.frame_best = o_best.at(d); a.inlier = o_inl.at(d); a.mask = o_mask.at(d);
        a.threshold = P.threshold; a.huber_delta = P.huber_delta; a.tau = t->cfg.tau;
        a.iterations = P.iterations; a.max_trials = t->cfg.max_trials; a.early_stop = t->cfg.early_stop;
        if (n_work) hipLaunchKernelGGL(k_vel_hyp, dim3((unsigned)n_work), dim3(VEL_WAVE), 0, s, a);
        hipLaunchKernelGGL(k_vel_select, dim3(n_frames), dim3(VEL_WAVE), 0, s, a);
        TR_HIP(hipGetLastError());
        TR_HIP(hipMemcpyAsync(out.data(), d + out0, out.size(), hipMemcpyDeviceToHost, s));
        TR_HIP(hipStreamSynchronize(s));
    } catch (const TrackerError& e) {
        return tracker_fail(t, e);
    }
    const char* r = out.data();   // the arena from out0 on
    const double *r_hvel = o_hvel.at(r, out0), *r_fvel = o_fvel.at(r, out0);
    const int *r_hinl = o_hinl.at(r, out0), *r_hit = o_hit.at(r, out0), *r_best = o_best.at(r, out0), *r_inl = o_inl.at(r, out0);
    for (int f = 0; f < n_frames; ++f) {
        lba_vel_frame& F = frames[f];
        const VelFrame& V = vf[f];
        F.best_hyp = r_best[2 * f];
        F.n_inliers = r_best[2 * f + 1];
        if (F.best_hyp >= 0) std::memcpy(F.vel, r_fvel + (size_t)f * 6, sizeof(F.vel));
        for (int i = 0; i < F.n_obs; ++i) obs[F.obs0 + i].inlier = r_inl[V.row0 + i];
        for (int h = 0; h < F.n_hyp; ++h) {
            const size_t g = (size_t)F.hyp0 + h, w = (size_t)V.work0 + h;
            if (hyp_vel) std::memcpy(hyp_vel + g * 6, r_hvel + w * 6, 6 * sizeof(double));
            if (hyp_inliers) hyp_inliers[g] = r_hinl[w];
            if (hyp_iterations) hyp_iterations[g] = r_hit[w];
        }
    }
    return LBA_OK;
}
