// lba_epipolar.hip — ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:947-1131) for a batch of (keyframe,
// neighbour) pairs: the matcher in front of lba_triangulate in LocalMapping::CreateNewMapPoints.
//
// In this reference the function decides every keypoint of KF1 on its own (vbMatched2 is never set, the map is only
// read; lba_epi_math.hpp), so k_epi_match gives ONE LANE to each keypoint of KF1 and one 64-lane wave to each task: a
// chunk of at most 64 entries of KF1's list of a node that both keyframes hold.  The host does the merge walk of the
// two node lists while packing and emits the tasks.  The wave walks KF2's list of the node sequentially in list order;
// the candidate's index and its 64-byte record have wave-uniform addresses (scalar loads, one cache line), each lane
// keeps its own descriptor in registers, does the 8 popcounts and, only when dist <= bestDist, the two fp64 gates
// against the table of (its camera, the candidate's camera).  The lane's loop is the reference's inner loop statement
// for statement (epi_candidate), so the tie rule holds by construction.  No reduction, no atomics, no flag, nothing
// waits on another workgroup, no LDS.  k_epi_tables makes the 11 doubles per (pair, c1, c2) into a work section first.
// Keypoints of KF1 in no common node keep LBA_EPI_NO_NODE from the host's pre-fill of the arena image (the out section
// is uploaded with the inputs, 16 bytes per row; no third pass: DESIGN.md §7 item 12 has what that costs).
// One upload, two launches, one download.  Integer- and latency-bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_epi_math.hpp"
#include "lba_tracker.hpp"

using namespace lba;

namespace {

constexpr int EPI_WAVE = 64;
constexpr int EPI_WG = 256;        // four tasks per workgroup
constexpr int EPI_MAX_CAM = 64;    // as lba_triangulate
static_assert(sizeof(lba_epi_feat) == 64 && sizeof(lba_epi_kf) == 24 && sizeof(lba_epi_pair) == 16 &&
              sizeof(lba_epi_row) == 16 && sizeof(lba_epi_params) == 16, "ABI layout");

struct EpiTask {
    int a, na;      // the chunk of KF1's node list: node_feat[a, a + na), na <= 64
    int b, nb;      // KF2's list of the node: node_feat[b, b + nb)
    int f1, f2;     // feat0 of either keyframe
    int row0;       // the pair's packed rows
    int pair;
};

struct EpiTabArgs {
    const lba_epi_pair* pairs;
    const lba_tri_kf* kfs;
    const lba_tri_cam* cams;
    double* tabs;   // [n_pairs][n_cam][n_cam][EPI_TAB]
    int n_pairs, n_cam;
};

__global__ __launch_bounds__(EPI_WG) void k_epi_tables(EpiTabArgs A) {
    const int cc = A.n_cam * A.n_cam;
    const long long i = (long long)blockIdx.x * EPI_WG + threadIdx.x;
    if (i >= (long long)A.n_pairs * cc) return;
    const int p = (int)(i / cc), c = (int)(i % cc), c1 = c / A.n_cam, c2 = c % A.n_cam;
    const lba_epi_pair P = A.pairs[p];
    double tab[EPI_TAB];
    epi_table(A.cams[A.kfs[P.kf1].cam0 + c1], A.cams[A.kfs[P.kf2].cam0 + c2], tab);
#pragma unroll
    for (int k = 0; k < EPI_TAB; ++k) A.tabs[(size_t)i * EPI_TAB + k] = tab[k];
}

struct EpiArgs {
    const EpiTask* tasks;
    const lba_epi_feat* feats;
    const int* node_feat;
    const double* tabs;
    lba_epi_row* rows;      // packed: pair after pair, n_feat(kf1) each
    int n_tasks, n_cam, th_low, only_stereo, coarse;
};

__global__ __launch_bounds__(EPI_WG) void k_epi_match(EpiArgs A) {
    const int lane = threadIdx.x % EPI_WAVE;
    // the wave's task: the same value in all its lanes
    const int task = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (EPI_WG / EPI_WAVE) + threadIdx.x / EPI_WAVE));
    if (task >= A.n_tasks) return;
    const EpiTask T = A.tasks[task];
    if (lane >= T.na) return;
    const int idx1 = A.node_feat[T.a + lane];
    const lba_epi_feat f1 = A.feats[T.f1 + idx1];
    const bool stereo1 = epi_stereo(f1.cam, A.n_cam, f1.u_right);
    EpiBest best{A.th_low, -1};
    int status = epi_entry_status(f1, stereo1, A.only_stereo);
    if (status == LBA_EPI_OK) {
        const double* tabs = A.tabs + (size_t)T.pair * A.n_cam * A.n_cam * EPI_TAB;
        const lba_epi_feat* f2 = A.feats + T.f2;
        for (int i2 = 0; i2 < T.nb; ++i2) {
            const int idx2 = A.node_feat[T.b + i2];
            epi_candidate(f1, stereo1, f2[idx2], idx2, A.n_cam, A.only_stereo, A.coarse, A.th_low, tabs, best);
        }
        status = best.idx2 >= 0 ? LBA_EPI_OK : LBA_EPI_NO_MATCH;
    }
    A.rows[(size_t)T.row0 + idx1] = lba_epi_row{best.idx2, best.dist, status, 0};
}

int refuse(lba_tracker* t, const char* msg) { return tracker_fail(t, {LBA_E_ARG, msg}); }

}  // namespace

extern "C" int lba_match_epipolar_profile(lba_tracker* t, int32_t on, double* last_ms) {
    return t ? t->epi_timer.profile(on, last_ms, 2) : LBA_E_ARG;
}

extern "C" int lba_match_epipolar(lba_tracker* t, lba_epi_pair* pairs, int32_t n_pairs, lba_epi_row* out, int32_t n_out,
                                  const lba_tri_kf* kfs, const lba_epi_kf* ekfs, int32_t n_kf, const lba_tri_cam* cams,
                                  int32_t n_cam_rows, int32_t n_cam, const lba_epi_feat* feats, int32_t n_feats,
                                  const int32_t* node_id, const int32_t* node_start, int32_t n_node_rows,
                                  const int32_t* node_feat, int32_t n_node_feat, const lba_epi_params* prm_in) {
    if (!t) return LBA_E_ARG;
    if (n_pairs < 0 || n_out < 0 || n_kf < 0 || n_cam_rows < 0 || n_feats < 0 || n_node_rows < 0 || n_node_feat < 0)
        return refuse(t, "a negative count");
    if ((n_pairs && !pairs) || (n_out && !out) || !kfs || !ekfs || !cams || (n_feats && !feats) ||
        (n_node_rows && (!node_id || !node_start)) || (n_node_feat && !node_feat))
        return refuse(t, "a null array");
    if (n_cam < 1) return refuse(t, "n_cam < 1");
    const lba_epi_params prm = epi_params_or_default(prm_in);
    if (prm.th_low < 0 || prm.th_low > 255) return refuse(t, "th_low outside [0, 255]");
    if (n_cam > EPI_MAX_CAM) return tracker_fail(t, {LBA_E_LIMIT, "more than 64 cameras per keyframe"});
    // ---- checks first: a refused call writes nothing
    {
        std::vector<char> seen;
        for (int k = 0; k < n_kf; ++k) {
            const lba_epi_kf& E = ekfs[k];
            if (kfs[k].cam0 < 0 || (int64_t)kfs[k].cam0 + n_cam > n_cam_rows) return refuse(t, "a keyframe's cameras outside cams");
            if (E.feat0 < 0 || E.n_feat < 0 || (int64_t)E.feat0 + E.n_feat > n_feats) return refuse(t, "a keyframe's features outside feats");
            for (int i = 0; i < E.n_feat; ++i)
                if (feats[E.feat0 + i].cam < 0 || feats[E.feat0 + i].cam >= n_cam) return refuse(t, "a feature's cam outside [0, n_cam)");
            if (E.node0 < 0 || E.n_node < 0 || E.nf0 < 0 || E.nf0 > n_node_feat) return refuse(t, "a keyframe's nodes outside their arrays");
            if (E.n_node == 0) continue;
            if ((int64_t)E.node0 + E.n_node + 1 > n_node_rows) return refuse(t, "a keyframe's nodes outside node_id / node_start");
            const int32_t *id = node_id + E.node0, *st = node_start + E.node0;
            if (st[0] != 0) return refuse(t, "node_start does not start at 0");
            for (int j = 0; j < E.n_node; ++j) {
                if (j && id[j] <= id[j - 1]) return refuse(t, "node_id not strictly ascending");
                if (st[j + 1] < st[j]) return refuse(t, "node_start decreases");
            }
            if ((int64_t)E.nf0 + st[E.n_node] > n_node_feat) return refuse(t, "node_start past the end of node_feat");
            seen.assign((size_t)E.n_feat, 0);
            for (int j = 0; j < st[E.n_node]; ++j) {
                const int f = node_feat[E.nf0 + j];
                if (f < 0 || f >= E.n_feat) return refuse(t, "a node_feat entry outside [0, n_feat)");
                if (seen[f]) return refuse(t, "a node_feat entry listed twice in one keyframe");
                seen[f] = 1;
            }
        }
    }
    size_t n_rows = 0;
    {
        std::vector<std::pair<int64_t, int64_t>> spans;
        for (int p = 0; p < n_pairs; ++p) {
            const lba_epi_pair& P = pairs[p];
            if (P.kf1 < 0 || P.kf1 >= n_kf || P.kf2 < 0 || P.kf2 >= n_kf) return refuse(t, "a pair's keyframe outside [0, n_kf)");
            const int n1 = ekfs[P.kf1].n_feat;
            if (P.out0 < 0 || (int64_t)P.out0 + n1 > n_out) return refuse(t, "a pair's out range does not fit in out");
            if (n1) spans.push_back({P.out0, (int64_t)P.out0 + n1});
            n_rows += (size_t)n1;
        }
        std::sort(spans.begin(), spans.end());
        for (size_t i = 1; i < spans.size(); ++i)
            if (spans[i].first < spans[i - 1].second) return refuse(t, "two pairs' out ranges overlap");
    }
    if (n_rows == 0) {   // no pair, or only pairs whose KF1 has no feature
        for (int p = 0; p < n_pairs; ++p) pairs[p].n_matches = 0;
        return LBA_OK;
    }
    // ---- the tasks: per pair the merge walk of the two node lists (both strictly ascending, so stepping the smaller
    // side visits the nodes FeatureVector::lower_bound would), per common node the chunks of KF1's list
    std::vector<EpiTask> tasks;
    {
        size_t row0 = 0;
        for (int p = 0; p < n_pairs; ++p) {
            const lba_epi_kf &E1 = ekfs[pairs[p].kf1], &E2 = ekfs[pairs[p].kf2];
            const int32_t *id1 = node_id + E1.node0, *id2 = node_id + E2.node0;
            const int32_t *s1 = node_start + E1.node0, *s2 = node_start + E2.node0;
            for (int a = 0, b = 0; a < E1.n_node && b < E2.n_node;) {
                if (id1[a] < id2[b]) { ++a; continue; }
                if (id1[a] > id2[b]) { ++b; continue; }
                for (int k = s1[a]; k < s1[a + 1]; k += EPI_WAVE)
                    tasks.push_back(EpiTask{E1.nf0 + k, std::min(EPI_WAVE, s1[a + 1] - k), E2.nf0 + s2[b], s2[b + 1] - s2[b],
                                            E1.feat0, E2.feat0, (int)row0, p});
                ++a;
                ++b;
            }
            row0 += (size_t)E1.n_feat;
        }
    }
    const size_t n_tasks = tasks.size(), n_tab = (size_t)n_pairs * n_cam * n_cam;
    // ---- the arena: the rows are an input too (their pre-fill goes up), then come back
    ArenaPlan plan;
    const Sec<EpiTask> o_tasks = plan.in<EpiTask>(n_tasks);
    const Sec<lba_epi_pair> o_pairs = plan.in<lba_epi_pair>((size_t)n_pairs);
    const Sec<lba_tri_kf> o_kfs = plan.in<lba_tri_kf>((size_t)n_kf);
    const Sec<lba_tri_cam> o_cams = plan.in<lba_tri_cam>((size_t)n_cam_rows);
    const Sec<lba_epi_feat> o_feats = plan.in<lba_epi_feat>((size_t)n_feats);
    const Sec<int> o_nf = plan.in<int>((size_t)n_node_feat);
    const Sec<lba_epi_row> o_rows = plan.out<lba_epi_row>(n_rows);
    const Sec<double> o_tabs = plan.work<double>(n_tab * EPI_TAB);
    if (n_rows > 0x7fffffff || n_tasks > 0x7fffffff || n_tab > 0x7fffffff || plan.over_2gb())
        return tracker_fail(t, {LBA_E_LIMIT, "the batch's keyframes, tables and rows exceed 2 GB"});
    char* h = nullptr;
    try {
        ArenaCall call{t, plan, t->epi_timer};
        h = call.pin();
        if (n_tasks) std::memcpy(o_tasks.at(h), tasks.data(), n_tasks * sizeof(EpiTask));
        std::memcpy(o_pairs.at(h), pairs, (size_t)n_pairs * sizeof(lba_epi_pair));
        std::memcpy(o_kfs.at(h), kfs, (size_t)n_kf * sizeof(lba_tri_kf));
        std::memcpy(o_cams.at(h), cams, (size_t)n_cam_rows * sizeof(lba_tri_cam));
        if (n_feats) std::memcpy(o_feats.at(h), feats, (size_t)n_feats * sizeof(lba_epi_feat));
        if (n_node_feat) std::memcpy(o_nf.at(h), node_feat, (size_t)n_node_feat * sizeof(int));
        lba_epi_row* pre = o_rows.at(h);
        for (size_t i = 0; i < n_rows; ++i) pre[i] = lba_epi_row{-1, prm.th_low, LBA_EPI_NO_NODE, 0};
        if (n_tasks) {   // (no common node anywhere: the pre-fill is the result)
            char* d = call.place();
            // the upload of ArenaCall::upload, extended over the pre-filled rows
            TR_HIP(hipMemcpyAsync(d, h, plan.down_end, hipMemcpyHostToDevice, t->stream));
            EpiTabArgs ta{o_pairs.at(d), o_kfs.at(d), o_cams.at(d), o_tabs.at(d), n_pairs, n_cam};
            EpiArgs a{o_tasks.at(d), o_feats.at(d), o_nf.at(d), o_tabs.at(d), o_rows.at(d),
                      (int)n_tasks, n_cam, prm.th_low, prm.only_stereo != 0, prm.coarse != 0};
            call.mark();
            hipLaunchKernelGGL(k_epi_tables, dim3((unsigned)((n_tab + EPI_WG - 1) / EPI_WG)), dim3(EPI_WG), 0, t->stream, ta);
            TR_HIP(hipGetLastError());
            call.mark();
            constexpr int per_wg = EPI_WG / EPI_WAVE;
            hipLaunchKernelGGL(k_epi_match, dim3((unsigned)((n_tasks + per_wg - 1) / per_wg)), dim3(EPI_WG), 0, t->stream, a);
            TR_HIP(hipGetLastError());
            call.mark();
            call.finish();
        }
    } catch (const TrackerError& e) {
        return tracker_fail(t, e);
    }
    // ---- per pair: the rotation pass and nmatches on the host, the rows into `out`
    lba_epi_row* r = o_rows.at(h);
    for (int p = 0; p < n_pairs; ++p) {
        const lba_epi_kf &E1 = ekfs[pairs[p].kf1], &E2 = ekfs[pairs[p].kf2];
        pairs[p].n_matches = epi_finish(feats + E1.feat0, E1.n_feat, feats + E2.feat0, prm.check_orientation != 0, r);
        if (E1.n_feat) std::memcpy(out + pairs[p].out0, r, (size_t)E1.n_feat * sizeof(lba_epi_row));
        r += E1.n_feat;
    }
    return LBA_OK;
}
