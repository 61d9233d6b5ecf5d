// lba_triangulate.hip — local mapping's CreateNewMapPoints triangulation (src/LocalMapping.cc:408-587, with
// GeometricTools::Triangulate and MultiKeyFrame::UnprojectStereo) for a batch of (keyframe, neighbour) pairs, the step
// that makes the landmarks the next lba_set_problem receives.
//
// Every match is independent (lba_tri_math.hpp: tri_row), so k_triangulate gives ONE THREAD to each row and one
// 64-thread workgroup to each chunk of at most 64 rows of one pair; the host builds the chunk list.  The pair's 2 n_cam
// camera records and its two keyframe records go to LDS once per workgroup, as k_s3r_hyp does.  The rows lie in the
// arena field-major, so a wave's loads and its status / X stores are contiguous.  The null vector of the 4 x 4 is a
// fixed-sweep one-sided Jacobi in registers: nothing loops on data.  No floating-point reduction, no atomics, nothing
// waits on another workgroup; a row's result does not depend on the batch, the grid or its position.  One upload, one
// launch, one download.  Latency- and launch-bound.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/amc_lba.h"
#include "lba_math.hpp"
#include "lba_tracker.hpp"
#include "lba_tri_math.hpp"

using namespace lba;

namespace {

constexpr int TRI_WG = 64;
constexpr int TRI_MAX_CAM = 64;   // per keyframe: 2 * 64 camera records of 21 doubles are 21 KB of LDS
constexpr int TRI_CAM_W = sizeof(lba_tri_cam) / 8, TRI_KF_W = sizeof(lba_tri_kf) / 8;   // in 8-byte words
static_assert(sizeof(lba_tri_cam) == 168 && sizeof(lba_tri_kf) == 120 && sizeof(lba_tri_row) == 168, "ABI layout");
constexpr int TRI_NF = 16;        // double fields of a row: z1 z2 k1 k2 (2 each) ur depth sigma2 scale (1 each per side)

struct TriChunk {
    int row0, n;    // its packed rows, n <= TRI_WG
    int kf1, kf2;
};

struct TriArgs {
    const TriChunk* chunks;
    const lba_tri_kf* kfs;
    const lba_tri_cam* cams;
    const int* cam12;       // [2][n]: cam1, cam2
    const double* field;    // [TRI_NF][n], in TriRow's order
    int* status;            // out [n]
    int* stereo;            // out [n]
    double* X;              // out [3][n], written under LBA_TRI_OK only
    int n, n_cam, far_points;
    double ratio_factor, th_far;
};

__global__ __launch_bounds__(TRI_WG) void k_triangulate(TriArgs A) {
    extern __shared__ unsigned long long tri_lds[];   // [2 n_cam] lba_tri_cam, [2] lba_tri_kf
    const int lane = threadIdx.x;
    const TriChunk C = A.chunks[blockIdx.x];
    const int cam_words = A.n_cam * TRI_CAM_W;
    const unsigned long long* g1 = reinterpret_cast<const unsigned long long*>(A.cams + A.kfs[C.kf1].cam0);
    const unsigned long long* g2 = reinterpret_cast<const unsigned long long*>(A.cams + A.kfs[C.kf2].cam0);
    for (int i = lane; i < cam_words; i += TRI_WG) {
        tri_lds[i] = g1[i];
        tri_lds[cam_words + i] = g2[i];
    }
    const unsigned long long* k1 = reinterpret_cast<const unsigned long long*>(A.kfs + C.kf1);
    const unsigned long long* k2 = reinterpret_cast<const unsigned long long*>(A.kfs + C.kf2);
    if (lane < TRI_KF_W) {
        tri_lds[2 * cam_words + lane] = k1[lane];
        tri_lds[2 * cam_words + TRI_KF_W + lane] = k2[lane];
    }
    __syncthreads();
    if (lane >= C.n) return;
    const lba_tri_cam* cam = reinterpret_cast<const lba_tri_cam*>(tri_lds);
    const lba_tri_kf* kf = reinterpret_cast<const lba_tri_kf*>(tri_lds + 2 * cam_words);
    const size_t i = (size_t)C.row0 + lane, n = (size_t)A.n;
    const int cam1 = A.cam12[i], cam2 = A.cam12[n + i];
    const double* f = A.field + i;
    TriRow r;
    r.z1[0] = f[0 * n]; r.z1[1] = f[1 * n]; r.z2[0] = f[2 * n]; r.z2[1] = f[3 * n];
    r.k1[0] = f[4 * n]; r.k1[1] = f[5 * n]; r.k2[0] = f[6 * n]; r.k2[1] = f[7 * n];
    r.ur1 = f[8 * n]; r.ur2 = f[9 * n]; r.depth1 = f[10 * n]; r.depth2 = f[11 * n];
    r.sigma2_1 = f[12 * n]; r.sigma2_2 = f[13 * n]; r.scale1 = f[14 * n]; r.scale2 = f[15 * n];
    int stereo_point;
    double X[3];
    const int status = tri_row(r, cam[cam1], cam[A.n_cam + cam2], cam[A.n_cam - 1], cam[2 * A.n_cam - 1], kf[0], kf[1],
                               A.ratio_factor, A.far_points, A.th_far, &stereo_point, X);
    A.status[i] = status;
    A.stereo[i] = stereo_point;
    if (status == LBA_TRI_OK) {
        A.X[i] = X[0];
        A.X[n + i] = X[1];
        A.X[2 * n + i] = X[2];
    }
}

}  // namespace

extern "C" int lba_triangulate_profile(lba_tracker* t, int32_t on, double* last_ms) {
    return t ? t->tri_timer.profile(on, last_ms, 1) : LBA_E_ARG;
}

extern "C" int lba_triangulate(lba_tracker* t, lba_tri_pair* pairs, int32_t n_pairs, lba_tri_row* rows, int32_t n_rows,
                               const lba_tri_kf* kfs, int32_t n_kf, const lba_tri_cam* cams, int32_t n_cam_rows,
                               int32_t n_cam, const lba_tri_params* prm) {
    if (!t || n_pairs < 0 || n_rows < 0 || n_kf < 0 || n_cam_rows < 0 || (n_pairs && !pairs) || (n_rows && !rows) ||
        !kfs || !cams || n_cam < 1)
        return LBA_E_ARG;
    const double ratio_factor = prm ? prm->ratio_factor : 1.5 * 1.2;
    const double th_far = prm ? prm->th_far : 0.0;
    const int far_points = prm ? prm->far_points != 0 : 0;
    if (!std::isfinite(ratio_factor) || !(ratio_factor > 0.0)) return LBA_E_ARG;
    if (n_cam > TRI_MAX_CAM) return tracker_fail(t, {LBA_E_LIMIT, "more than 64 cameras per keyframe"});
    // ---- checks first: a refused call writes nothing
    for (int k = 0; k < n_kf; ++k)
        if (kfs[k].cam0 < 0 || (int64_t)kfs[k].cam0 + n_cam > n_cam_rows) return LBA_E_ARG;
    size_t n = 0, n_chunks = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const lba_tri_pair& P = pairs[p];
        if (P.kf1 < 0 || P.kf1 >= n_kf || P.kf2 < 0 || P.kf2 >= n_kf) return LBA_E_ARG;
        if (P.row0 < 0 || P.n_rows < 0 || (int64_t)P.row0 + P.n_rows > n_rows) return LBA_E_ARG;
        for (int i = P.row0; i < P.row0 + P.n_rows; ++i)
            if (rows[i].cam1 < 0 || rows[i].cam1 >= n_cam || rows[i].cam2 < 0 || rows[i].cam2 >= n_cam) return LBA_E_ARG;
        n += (size_t)P.n_rows;
        n_chunks += ((size_t)P.n_rows + TRI_WG - 1) / TRI_WG;
    }
    if (n == 0) {   // no pair, or only pairs without rows: nothing to launch
        for (int p = 0; p < n_pairs; ++p) pairs[p].n_new = pairs[p].n_stereo = 0;
        return LBA_OK;
    }
    // ---- the arena: inputs (one upload), outputs (one download); its pinned host image has the same offsets
    ArenaPlan plan;
    const Sec<TriChunk> o_chunks = plan.in<TriChunk>(n_chunks);
    const Sec<lba_tri_kf> o_kfs = plan.in<lba_tri_kf>((size_t)n_kf);
    const Sec<lba_tri_cam> o_cams = plan.in<lba_tri_cam>((size_t)n_cam_rows);
    const Sec<int> o_cam12 = plan.in<int>(2 * n);
    const Sec<double> o_field = plan.in<double>(TRI_NF * n);
    const Sec<int> o_status = plan.out<int>(n), o_stereo = plan.out<int>(n);
    const Sec<double> o_X = plan.out<double>(3 * n);
    if (n > 0x7fffffff || n_chunks > 0x7fffffff || plan.over_2gb())
        return tracker_fail(t, {LBA_E_LIMIT, "the batch's rows, keyframes and cameras exceed 2 GB"});
    char* h = nullptr;
    try {
        ArenaCall call{t, plan, t->tri_timer};
        h = call.pin();
        // per pair: its rows packed in pair order (overlapping ranges get rows of their own), cut into chunks
        TriChunk* ch = o_chunks.at(h);
        int* cam12 = o_cam12.at(h);
        double* fd = o_field.at(h);
        size_t at = 0, c = 0;
        for (int p = 0; p < n_pairs; ++p) {
            const lba_tri_pair& P = pairs[p];
            for (int k = 0; k < P.n_rows; k += TRI_WG)
                ch[c++] = TriChunk{(int)(at + k), P.n_rows - k < TRI_WG ? P.n_rows - k : TRI_WG, P.kf1, P.kf2};
            for (int k = 0; k < P.n_rows; ++k, ++at) {
                const lba_tri_row& r = rows[P.row0 + k];
                cam12[at] = r.cam1; cam12[n + at] = r.cam2;
                const double v[TRI_NF] = {r.z1[0], r.z1[1], r.z2[0], r.z2[1], r.k1[0], r.k1[1], r.k2[0], r.k2[1],
                                          r.ur1, r.ur2, r.depth1, r.depth2, r.sigma2_1, r.sigma2_2, r.scale1, r.scale2};
                for (int j = 0; j < TRI_NF; ++j) fd[(size_t)j * n + at] = v[j];
            }
        }
        std::memcpy(o_kfs.at(h), kfs, (size_t)n_kf * sizeof(lba_tri_kf));
        std::memcpy(o_cams.at(h), cams, (size_t)n_cam_rows * sizeof(lba_tri_cam));
        char* d = call.place();
        call.upload();
        TriArgs a;
        a.chunks = o_chunks.at(d); a.kfs = o_kfs.at(d); a.cams = o_cams.at(d);
        a.cam12 = o_cam12.at(d); a.field = o_field.at(d);
        a.status = o_status.at(d); a.stereo = o_stereo.at(d); a.X = o_X.at(d);
        a.n = (int)n; a.n_cam = n_cam; a.far_points = far_points;
        a.ratio_factor = ratio_factor; a.th_far = th_far;
        const size_t lds = 8 * (2 * (size_t)n_cam * TRI_CAM_W + 2 * (size_t)TRI_KF_W);
        call.mark();
        hipLaunchKernelGGL(k_triangulate, dim3((unsigned)n_chunks), dim3(TRI_WG), lds, t->stream, a);
        TR_HIP(hipGetLastError());
        call.mark();
        call.finish();
    } catch (const TrackerError& e) {
        return tracker_fail(t, e);
    }
    // ---- scatter: status, stereo_point and X (under LBA_TRI_OK) into the rows; the counts from the statuses
    const int *r_status = o_status.at(h), *r_stereo = o_stereo.at(h);
    const double* r_X = o_X.at(h);
    // A row shared by two pairs carries the later pair's result alone (its X stays untouched unless THAT is
    // LBA_TRI_OK): the first pass leaves in `status` the packed index of the row's last visit, the second writes there.
    size_t at = 0;
    for (int p = 0; p < n_pairs; ++p)
        for (int k = 0; k < pairs[p].n_rows; ++k, ++at) rows[pairs[p].row0 + k].status = -1 - (int)at;
    at = 0;
    for (int p = 0; p < n_pairs; ++p) {
        lba_tri_pair& P = pairs[p];
        int n_new = 0, n_stereo = 0;
        for (int k = 0; k < P.n_rows; ++k, ++at) {
            const bool ok = r_status[at] == LBA_TRI_OK;
            n_new += ok;
            n_stereo += ok && r_stereo[at] != 0;
            lba_tri_row& r = rows[P.row0 + k];
            if (r.status != -1 - (int)at) continue;
            r.status = r_status[at];
            r.stereo_point = r_stereo[at];
            if (ok) { r.X[0] = r_X[at]; r.X[1] = r_X[n + at]; r.X[2] = r_X[2 * n + at]; }
        }
        P.n_new = n_new;
        P.n_stereo = n_stereo;
    }
    return LBA_OK;
}
