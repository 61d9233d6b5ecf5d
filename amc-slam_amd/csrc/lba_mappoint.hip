// lba_mappoint.hip — MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:611-700) and
// MapPoint::ComputeDistinctiveDescriptors (:498-578) for a batch of map points: what local mapping runs point by point
// after ProcessNewKeyFrame, after SearchInNeighbors' fuses and at the end of the two bundle adjustments.  A point reads
// its own position, list and reference keyframe and the keyframes' immutable features and current centres, so a batch
// is the sequence exactly.  The arithmetic is lba_mp_math.hpp's, the same functions the host builds.
//
//   k_mp_geom        one LANE per point: it walks the point's list in order (the float sum is one chain in list order),
//                    with the depth range of the reference keyframe's observations in the same pass.
//   k_mp_desc_wave   N <= 64 candidates: one WAVE per point.  Lane i finds its candidate (the i-th observation whose
//                    keyframe is not bad: ballots over the list and a select of the i-th set bit), holds its descriptor
//                    in 8 VGPRs (two 16-byte loads), and takes its row's median by bisection on the value; candidate
//                    j's words reach every lane by readlane.  No LDS.
//   k_mp_desc_block  65 <= N <= 1024: one 256-thread workgroup per point.  The candidates are compacted into LDS (ballot
//                    per 64 observations, the 16 counts through LDS), 32 bytes each, at most 32 KB; rows are strided
//                    over the threads, the same bisection, candidate j read from LDS by every lane at once.
//   Both: the minimum of (median << 10 | row) over the rows is the first row of the least median.
// No atomics, no wait on another workgroup, no scratch.  The host sorts the points into the two classes (it knows
// kf_bad), narrows the camera centres to float, and copies the winner's descriptor from the caller's own features.
// One upload, up to three launches, one download.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_mp_math.hpp"
#include "lba_tracker.hpp"

using namespace lba;

namespace {

constexpr int MP_WG = 256;
typedef unsigned long long u64;
static_assert(sizeof(lba_mp_point) == 112 && sizeof(lba_mp_obs) == 8 && sizeof(lba_epi_feat) == 64 &&
              offsetof(lba_epi_feat, desc) == 32, "ABI layout");

struct MpIn {          // what the device reads of a point
    float pos[3];
    int ref_kf, obs0, n_obs;
    int geom;          // k_mp_geom computes it
    int pad;
};
struct MpGeomOut {
    float normal[3], mind, maxd;
    int n, pad[2];
};
struct MpDescOut { int best_obs, best_median; };
struct MpFs { float scale; int cam; };   // what the geometry reads of a feature
static_assert(sizeof(MpIn) == 32 && sizeof(MpGeomOut) == 32, "device records");

struct MpArgs {
    const MpIn* pts;
    const lba_mp_obs* obs;
    const float4* ow;           // [n_kf][n_cam]: the centres, narrowed
    const int* feat0;           // [n_kf]
    const int* kf_bad;          // [n_kf]
    const MpFs* fs;             // [n_feats]
    const lba_epi_feat* feats;  // [n_feats], uploaded when a point asks for its descriptor
    const int* wave_list;       // points with N <= 64
    const int* block_list;      // points with N > 64
    MpGeomOut* geom;            // out [n_points]
    MpDescOut* dw;              // out [n_wave]
    MpDescOut* db;              // out [n_block]
    int n_points, n_wave, n_block, n_cam;
    float scale_top;
};

__global__ __launch_bounds__(MP_WG) void k_mp_geom(MpArgs A) {
    const int p = blockIdx.x * MP_WG + threadIdx.x;
    if (p >= A.n_points) return;
    const MpIn P = A.pts[p];
    if (!P.geom) return;
    const lba_mp_obs* __restrict__ L = A.obs + P.obs0;
    MpGeom G = mp_geom_begin();
#pragma unroll 4
    for (int k = 0; k < P.n_obs; ++k) {
        const lba_mp_obs o = L[k];
        const MpFs f = A.fs[A.feat0[o.kf] + o.feat];
        const float4 w = A.ow[o.kf * A.n_cam + f.cam];
        mp_geom_add(G, P.pos, w.x, w.y, w.z, o.kf == P.ref_kf, f.scale, A.scale_top);
    }
    MpGeomOut R;
    mp_geom_end(G, R.normal);
    R.mind = G.mind;
    R.maxd = G.maxd;
    R.n = G.n;
    R.pad[0] = R.pad[1] = 0;
    A.geom[p] = R;
}

// the index of the r-th set bit of m (r counted from 0; m has more than r bits set)
__device__ __forceinline__ int mp_select(u64 m, int r) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const int c = __popcll((m >> pos) & ((1ull << w) - 1ull));
        if (r >= c) {
            r -= c;
            pos += w;
        }
    }
    return pos;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t m) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)m, d, 64);
        m = other < m ? other : m;
    }
    return m;
}

__device__ __forceinline__ const uint4* desc_words(const MpArgs& A, lba_mp_obs o) {
    return reinterpret_cast<const uint4*>(A.feats[A.feat0[o.kf] + o.feat].desc);
}

__global__ __launch_bounds__(MP_WG) void k_mp_desc_wave(MpArgs A) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (MP_WG / 64) + (threadIdx.x >> 6);
    if (w >= A.n_wave) return;   // wave-uniform
    const MpIn P = A.pts[A.wave_list[w]];
    const lba_mp_obs* L = A.obs + P.obs0;
    int pos = -1, count = 0;     // the lane's candidate: its position in the list
    for (int k0 = 0; k0 < P.n_obs; k0 += 64) {
        const int k = k0 + lane;
        const bool good = k < P.n_obs && A.kf_bad[L[k].kf] == 0;
        const u64 mask = __ballot(good);
        const int c = __popcll(mask);
        if (lane >= count && lane < count + c) pos = k0 + mp_select(mask, lane - count);
        count += c;
    }
    const int N = __builtin_amdgcn_readfirstlane(count);   // 1 .. 64: the host's class
    uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (lane < N) {
        const uint4* q = desc_words(A, L[pos]);
        const uint4 a = q[0], b = q[1];
        d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
        d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
    }
    // every lane runs the row (the loops are wave-uniform); lanes >= N carry a row nobody reads
    const int med = mp_row_median(N, mp_median_pos(N), [&](int j) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += __popc(d[k] ^ (uint32_t)__builtin_amdgcn_readlane((int)d[k], j));
        return s;
    });
    const uint32_t key = wave_min(lane < N ? mp_key(med, lane) : 0xffffffffu);
    const int best = __builtin_amdgcn_readlane(pos, mp_key_row(key));
    if (lane == 0) A.dw[w] = MpDescOut{best, mp_key_median(key)};
}

__global__ __launch_bounds__(MP_WG) void k_mp_desc_block(MpArgs A) {
    __shared__ uint4 s_desc[2 * LBA_MP_MAX_OBS];   // candidate q: s_desc[2 q], s_desc[2 q + 1]
    __shared__ int s_pos[LBA_MP_MAX_OBS];          // its position in the list
    __shared__ int s_cnt[16];                      // candidates per 64 observations
    __shared__ uint32_t s_key[MP_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MpIn P = A.pts[A.block_list[blockIdx.x]];
    const lba_mp_obs* L = A.obs + P.obs0;
    bool good[4];
    int before[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // chunk r * 4 + wave holds observations [64 chunk, 64 chunk + 64)
        const int k = r * MP_WG + tid;
        good[r] = k < P.n_obs && A.kf_bad[L[k].kf] == 0;
        const u64 mask = __ballot(good[r]);
        before[r] = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[r * 4 + wave] = __popcll(mask);
    }
    __syncthreads();
    int N = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int base = 0;
        for (int c = 0; c < r * 4 + wave; ++c) base += s_cnt[c];
        if (good[r]) {
            const int k = r * MP_WG + tid, q = base + before[r];   // q < N <= n_obs <= 1024
            const uint4* g = desc_words(A, L[k]);
            s_desc[2 * q] = g[0];
            s_desc[2 * q + 1] = g[1];
            s_pos[q] = k;
        }
    }
    for (int c = 0; c < 16; ++c) N += s_cnt[c];
    __syncthreads();
    const int m = mp_median_pos(N);
    uint32_t key = 0xffffffffu;
    for (int i = tid; i < N; i += MP_WG) {
        const uint4 a = s_desc[2 * i], b = s_desc[2 * i + 1];
        const int med = mp_row_median(N, m, [&](int j) {
            const uint4 x = s_desc[2 * j], y = s_desc[2 * j + 1];   // one address for the whole wave: a broadcast
            return (__popc(a.x ^ x.x) + __popc(a.y ^ x.y)) + (__popc(a.z ^ x.z) + __popc(a.w ^ x.w)) +
                   (__popc(b.x ^ y.x) + __popc(b.y ^ y.y)) + (__popc(b.z ^ y.z) + __popc(b.w ^ y.w));
        });
        const uint32_t kk = mp_key(med, i);
        key = kk < key ? kk : key;
    }
    key = wave_min(key);
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < MP_WG / 64; ++v) key = s_key[v] < key ? s_key[v] : key;
        A.db[blockIdx.x] = MpDescOut{s_pos[mp_key_row(key)], mp_key_median(key)};
    }
}

#define MP_REFUSE(c, m) return tracker_fail(t, TrackerError{c, "lba_mappoint_refresh: " m})

}  // namespace

extern "C" int lba_mappoint_refresh_profile(lba_tracker* t, int32_t on, double* last_ms) {
    return t ? t->mp_timer.profile(on, last_ms, 3) : LBA_E_ARG;
}

extern "C" int lba_mappoint_refresh(lba_tracker* t, lba_mp_point* points, int32_t n_points, const lba_mp_obs* obs,
                                    int32_t n_obs, const lba_tri_kf* kfs, const lba_epi_kf* ekfs, int32_t n_kf,
                                    const lba_tri_cam* cams, int32_t n_cam_rows, int32_t n_cam,
                                    const lba_epi_feat* feats, int32_t n_feats, const int32_t* kf_bad,
                                    const lba_mp_params* prm) {
    if (!t) return LBA_E_ARG;
    if (n_points < 0 || n_obs < 0 || n_kf < 0 || n_cam_rows < 0 || n_feats < 0) MP_REFUSE(LBA_E_ARG, "a negative count");
    if ((n_points && !points) || (n_obs && !obs) || (n_kf && (!kfs || !ekfs)) || (n_cam_rows && !cams) ||
        (n_feats && !feats))
        MP_REFUSE(LBA_E_ARG, "a null array");
    if (!prm) MP_REFUSE(LBA_E_ARG, "null params");
    if (std::isnan(prm->scale_top)) MP_REFUSE(LBA_E_ARG, "scale_top is not a number");
    if (n_cam < 1) MP_REFUSE(LBA_E_ARG, "n_cam < 1");
    if (n_cam > 64) MP_REFUSE(LBA_E_LIMIT, "n_cam > 64");
    // ---- checks first: a refused call writes nothing
    std::vector<MpFs> fs((size_t)n_feats, MpFs{0.0f, 0});
    std::vector<int> per_cam((size_t)n_cam);
    for (int k = 0; k < n_kf; ++k) {
        if (kfs[k].cam0 < 0 || (int64_t)kfs[k].cam0 + n_cam > n_cam_rows)
            MP_REFUSE(LBA_E_ARG, "a keyframe's cameras outside the array");
        const lba_epi_kf& E = ekfs[k];
        if (E.n_feat < 0 || E.feat0 < 0 || (int64_t)E.feat0 + E.n_feat > n_feats)
            MP_REFUSE(LBA_E_ARG, "a keyframe's features outside the array");
        std::fill(per_cam.begin(), per_cam.end(), 0);
        for (int f = E.feat0; f < E.feat0 + E.n_feat; ++f) {
            const int c = feats[f].cam;
            if (c < 0 || c >= n_cam) MP_REFUSE(LBA_E_ARG, "a feature's camera outside [0, n_cam)");
            if (++per_cam[(size_t)c] > LBA_MATCH_MAX_FEAT) MP_REFUSE(LBA_E_LIMIT, "more than 8192 features in one camera");
            fs[(size_t)f] = MpFs{feats[f].scale, c};
        }
    }
    for (int i = 0; i < n_obs; ++i)
        if (obs[i].kf < 0 || obs[i].kf >= n_kf || obs[i].feat < 0 || obs[i].feat >= ekfs[obs[i].kf].n_feat)
            MP_REFUSE(LBA_E_ARG, "an observation's kf or feat out of range");
    bool any_bad = false;
    for (int k = 0; kf_bad && k < n_kf; ++k) any_bad |= kf_bad[k] != 0;
    // the size classes: cand[p] = N of a point whose descriptor is asked for, -1 otherwise
    std::vector<int> wave_list, block_list, cand((size_t)n_points, -1);
    bool any_geom = false;
    for (int p = 0; p < n_points; ++p) {
        const lba_mp_point& P = points[p];
        if (P.ops < 1 || P.ops > 3) MP_REFUSE(LBA_E_ARG, "a point's ops outside 1..3");
        if (P.ref_kf < -1 || P.ref_kf >= n_kf) MP_REFUSE(LBA_E_ARG, "a point's ref_kf out of range");
        if (P.n_obs < 0 || P.obs0 < 0 || (int64_t)P.obs0 + P.n_obs > n_obs)
            MP_REFUSE(LBA_E_ARG, "a point's observations outside the array");
        if (P.n_obs > LBA_MP_MAX_OBS) MP_REFUSE(LBA_E_LIMIT, "a point with more than 1024 observations");
        if (P.bad || P.n_obs == 0) continue;
        any_geom |= (P.ops & LBA_MP_NORMAL) != 0;
        if (!(P.ops & LBA_MP_DESC)) continue;
        int N = P.n_obs;
        if (any_bad) {
            N = 0;
            for (int k = 0; k < P.n_obs; ++k) N += kf_bad[obs[P.obs0 + k].kf] == 0;
        }
        cand[(size_t)p] = N;
        if (N > 64) block_list.push_back(p);
        else if (N > 0) wave_list.push_back(p);
    }
    const size_t np = (size_t)n_points, nw = wave_list.size(), nb = block_list.size();
    const bool any_desc = nw + nb > 0;
    // ---- the arena: inputs (one upload), the results (one download)
    ArenaPlan plan;
    const Sec<MpIn> o_pts = plan.in<MpIn>(np);
    const Sec<lba_mp_obs> o_obs = plan.in<lba_mp_obs>((size_t)n_obs);
    const Sec<float4> o_ow = plan.in<float4>((size_t)n_kf * n_cam);
    const Sec<int> o_feat0 = plan.in<int>((size_t)n_kf), o_bad = plan.in<int>((size_t)n_kf);
    const Sec<MpFs> o_fs = plan.in<MpFs>(any_geom ? (size_t)n_feats : 0);
    const Sec<lba_epi_feat> o_feats = plan.in<lba_epi_feat>(any_desc ? (size_t)n_feats : 0);
    const Sec<int> o_wl = plan.in<int>(nw), o_bl = plan.in<int>(nb);
    const Sec<MpGeomOut> o_geom = plan.out<MpGeomOut>(any_geom ? np : 0);
    const Sec<MpDescOut> o_dw = plan.out<MpDescOut>(nw), o_db = plan.out<MpDescOut>(nb);
    if (plan.over_2gb()) MP_REFUSE(LBA_E_LIMIT, "the batch exceeds 2 GB");
    char* h = nullptr;
    if (any_geom || any_desc) {
        try {
            ArenaCall call{t, plan, t->mp_timer};
            h = call.pin();
            MpIn* in = o_pts.at(h);
            for (size_t p = 0; p < np; ++p) {
                const lba_mp_point& P = points[p];
                in[p] = MpIn{{P.pos[0], P.pos[1], P.pos[2]}, P.ref_kf, P.obs0, P.n_obs,
                             !P.bad && P.n_obs > 0 && (P.ops & LBA_MP_NORMAL), 0};
            }
            std::memcpy(o_obs.at(h), obs, (size_t)n_obs * sizeof(lba_mp_obs));
            float4* ow = o_ow.at(h);
            for (int k = 0; k < n_kf; ++k) {
                for (int c = 0; c < n_cam; ++c) {
                    const double* O = cams[kfs[k].cam0 + c].Ow;
                    ow[(size_t)k * n_cam + c] = make_float4((float)O[0], (float)O[1], (float)O[2], 0.0f);
                }
                o_feat0.at(h)[k] = ekfs[k].feat0;
                o_bad.at(h)[k] = kf_bad && kf_bad[k] != 0;
            }
            if (any_geom && n_feats) std::memcpy(o_fs.at(h), fs.data(), (size_t)n_feats * sizeof(MpFs));
            if (any_desc) std::memcpy(o_feats.at(h), feats, (size_t)n_feats * sizeof(lba_epi_feat));
            if (nw) std::memcpy(o_wl.at(h), wave_list.data(), nw * sizeof(int));
            if (nb) std::memcpy(o_bl.at(h), block_list.data(), nb * sizeof(int));
            char* d = call.place();
            call.upload();
            MpArgs a;
            a.pts = o_pts.at(d); a.obs = o_obs.at(d); a.ow = o_ow.at(d); a.feat0 = o_feat0.at(d); a.kf_bad = o_bad.at(d);
            a.fs = o_fs.at(d); a.feats = o_feats.at(d); a.wave_list = o_wl.at(d); a.block_list = o_bl.at(d);
            a.geom = o_geom.at(d); a.dw = o_dw.at(d); a.db = o_db.at(d);
            a.n_points = n_points; a.n_wave = (int)nw; a.n_block = (int)nb; a.n_cam = n_cam; a.scale_top = prm->scale_top;
            call.mark();
            if (any_geom) {
                hipLaunchKernelGGL(k_mp_geom, dim3((unsigned)((np + MP_WG - 1) / MP_WG)), dim3(MP_WG), 0, t->stream, a);
                TR_HIP(hipGetLastError());
            }
            call.mark();
            if (nw) {
                hipLaunchKernelGGL(k_mp_desc_wave, dim3((unsigned)((nw + 3) / 4)), dim3(MP_WG), 0, t->stream, a);
                TR_HIP(hipGetLastError());
            }
            call.mark();
            if (nb) {
                hipLaunchKernelGGL(k_mp_desc_block, dim3((unsigned)nb), dim3(MP_WG), 0, t->stream, a);
                TR_HIP(hipGetLastError());
            }
            call.mark();
            call.finish();
        } catch (const TrackerError& e) {
            return tracker_fail(t, e);
        }
    }
    // ---- the results into the points: only what the reference writes
    std::vector<MpDescOut> chosen(np, MpDescOut{-1, -1});
    for (size_t i = 0; i < nw; ++i) chosen[(size_t)wave_list[i]] = o_dw.at(h)[i];
    for (size_t i = 0; i < nb; ++i) chosen[(size_t)block_list[i]] = o_db.at(h)[i];
    for (size_t p = 0; p < np; ++p)
        if (cand[p] > 0 && (chosen[p].best_obs < 0 || chosen[p].best_obs >= points[p].n_obs))
            MP_REFUSE(LBA_E_HIP, "the device chose an observation outside the point's list");
    for (size_t p = 0; p < np; ++p) {
        lba_mp_point& P = points[p];
        P.n = 0;
        P.best_obs = P.best_median = -1;
        P.status = P.bad ? LBA_MP_BAD : P.n_obs == 0 ? LBA_MP_EMPTY : LBA_MP_OK;
        if (P.status != LBA_MP_OK) continue;
        if (P.ops & LBA_MP_NORMAL) {
            const MpGeomOut& G = o_geom.at(h)[p];
            std::memcpy(P.normal, G.normal, sizeof P.normal);
            P.min_distance = G.mind;
            P.max_distance = G.maxd;
            P.n = G.n;
        }
        if (cand[p] > 0) {
            const MpDescOut& D = chosen[p];
            const lba_mp_obs& o = obs[P.obs0 + D.best_obs];
            std::memcpy(P.desc, feats[ekfs[o.kf].feat0 + o.feat].desc, sizeof P.desc);
            P.best_obs = D.best_obs;
            P.best_median = D.best_median;
        }
    }
    return LBA_OK;
}
