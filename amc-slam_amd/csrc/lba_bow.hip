// lba_bow.hip — ORBmatcher::SearchByBoW for a batch of pairs, both overloads (src/ORBmatcher.cc:805-945 for loop
// closing, :227-421 for TrackReferenceKeyFrame): the matcher in front of lba_sim3_ransac / lba_sim3_optimize in
// LoopClosing::DetectCommonRegionsFromBoW.
//
// The function is greedy: an accepted idx2 is skipped by every later idx1 (vbMatched2).  The flag is indexed by idx2
// and a feature is in exactly one node, so the state never leaves a node: k_bow_match gives ONE 64-LANE WAVE to each
// task, a (pair, node both sides hold).  The host does the merge walk of the two node lists while packing and emits
// the tasks.  Lane l owns the candidates l, l + 64, ... of side 2's list; their matched flags (and, in LBA_BOW_KF, "has
// no point") are the bits of one register, so a list holds at most 32 * 64 = LBA_BOW_MAX_NODE entries and there is no
// flag array and no atomic.  The first BOW_LDS_CAP candidates' descriptors are staged once per task in LDS as two
// 16-byte planes (lane stride 16 bytes; each lane reads back only what it wrote, so no barrier); the candidates behind
// them are read from global memory at every step.  The LDS of a launch is sized to the longest list of the batch, so
// that ordinary nodes (tens of entries) do not pay the occupancy of the cap.  The wave walks side 1's list serially,
// in blocks of 64: lane e holds entry e of the block (vector loads, the next block's ahead of the walk) and a step
// broadcasts its entry with readlane, so that no load is on the chain from step to step (scalar loads would be: they
// share the counter the LDS reads and the cross-lane moves wait on); each lane folds its candidates (bow_fold), one
// 6-stage butterfly of bow_merge on (key, second) gives every lane the best key (distance, position) and the second
// best (lba_bow_math.hpp has why that is exact), the accept test is the same in all lanes, the owner lane sets its
// bit, lane e keeps the result of entry e and writes the block's rows after the walk.
// Rows of side 1 that run no inner loop (no point, no common node, an empty list) keep the host's pre-fill of the
// arena image, as in lba_epipolar.hip.
// One upload, one launch, one download.  Integer- and latency-bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_bow_math.hpp"
#include "lba_tracker.hpp"

using namespace lba;

namespace {

constexpr int BOW_WAVE = 64;
constexpr int BOW_WG = 256;          // four tasks per workgroup
constexpr int BOW_LDS_CAP = 512;     // candidates of a task staged in LDS at the most: 16 KB per wave, 64 KB per workgroup
static_assert(LBA_BOW_MAX_NODE == 32 * BOW_WAVE, "one matched bit per candidate in a 32-bit register per lane");
static_assert(LBA_BOW_MAX_NODE <= BOW_NO_POS, "a list position fits the key");
static_assert(sizeof(lba_epi_feat) == 64 && sizeof(lba_epi_kf) == 24 && sizeof(lba_bow_pair) == 16 &&
              sizeof(lba_bow_row) == 16 && sizeof(lba_bow_params) == 16, "ABI layout");

struct BowTask {
    int a, na;      // side 1's list of the node: node_feat[a, a + na), na >= 1
    int b, nb;      // side 2's list of the node: node_feat[b, b + nb), 1 <= nb <= LBA_BOW_MAX_NODE
    int f1, f2;     // feat0 of either side
    int row0;       // the pair's packed rows
    int pad;
};

struct BowArgs {
    const BowTask* tasks;
    const lba_epi_feat* feats;
    const int* node_feat;
    lba_bow_row* rows;      // packed: pair after pair, n_feat(kf1) each
    int n_tasks, mode, th_low;
    float nn_ratio;
    int lds_chunks;         // 64-candidate chunks of a list staged in LDS: 1 .. BOW_LDS_CAP / 64
};

// bow_merge over the wave on (key, second): a butterfly, so the two sides of a stage hold disjoint lanes and every
// lane ends with the whole wave's.  The loser's best is the larger key's distance.
__device__ __forceinline__ void wave_merge(int& key, int& b2) {
#pragma unroll
    for (int m = 1; m < BOW_WAVE; m <<= 1) {
        const int okey = __shfl_xor(key, m, BOW_WAVE), ob2 = __shfl_xor(b2, m, BOW_WAVE);
        b2 = min(min(b2, ob2), max(key, okey) >> 16);
        key = min(key, okey);
    }
}

__device__ __forceinline__ int bow_dist(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// the two 16-byte halves of a record's descriptor (offset 32 of a 64-byte record in a 256-byte aligned section)
__device__ __forceinline__ const uint4* desc_of(const lba_epi_feat* f) { return reinterpret_cast<const uint4*>(f->desc); }

// entry e of side 1's list (na entries) as its lane holds it; has == 0 past the end
struct BowEntry {
    int idx, has;
    uint4 d0, d1;
};
__device__ __forceinline__ BowEntry bow_entry(const int* l1, const lba_epi_feat* f1, int e, int na) {
    BowEntry E{0, 0, uint4{0, 0, 0, 0}, uint4{0, 0, 0, 0}};
    if (e < na) {
        E.idx = l1[e];
        const lba_epi_feat* r = f1 + E.idx;
        E.has = r->has_point != 0;
        E.d0 = desc_of(r)[0];
        E.d1 = desc_of(r)[1];
    }
    return E;
}

__global__ __launch_bounds__(BOW_WG) void k_bow_match(BowArgs A) {
    extern __shared__ uint4 s_desc[];   // [wave][plane][lds_chunks * 64]
    const int lane = threadIdx.x % BOW_WAVE, wave = threadIdx.x / BOW_WAVE;
    // the wave's task: the same value in all its lanes
    const int task = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (BOW_WG / BOW_WAVE)) + wave);
    if (task >= A.n_tasks) return;
    const BowTask T = A.tasks[task];
    const int* l1 = A.node_feat + T.a;
    const int* l2 = A.node_feat + T.b;
    const lba_epi_feat* f1 = A.feats + T.f1;
    const lba_epi_feat* f2 = A.feats + T.f2;
    const int lds_n = A.lds_chunks * BOW_WAVE;
    uint4* sd0 = s_desc + (size_t)wave * 2 * lds_n;
    uint4* sd1 = sd0 + lds_n;
    const int nk = (T.nb + BOW_WAVE - 1) / BOW_WAVE;                 // chunks of side 2's list, <= 32
    const int nk_lds = nk < A.lds_chunks ? nk : A.lds_chunks;

    // ---- side 2 once per task: bit k of `skip` = candidate lane + 64 k is not to be looked at (past the end of the
    // list, without a point in LBA_BOW_KF, or, later, matched)
    uint32_t skip = nk < 32 ? ~0u << nk : 0u;
    for (int k = 0; k < nk; ++k) {
        const int c = lane + BOW_WAVE * k;
        if (c >= T.nb) {
            skip |= 1u << k;
            continue;
        }
        const lba_epi_feat* r = f2 + l2[c];
        if (A.mode == LBA_BOW_KF && !r->has_point) skip |= 1u << k;
        if (k < nk_lds) {
            sd0[c] = desc_of(r)[0];
            sd1[c] = desc_of(r)[1];
        }
    }

    // ---- side 1 serially, in blocks of 64 entries.  Lane e holds entry blk + e of the list (index, has_point, the
    // descriptor in 8 registers; vector loads, the next block's asked for before this block's walk) and, after the
    // walk, its result, which it writes itself.  A step broadcasts its entry with readlane, so no memory access
    // except the LDS reads of the candidates is on the chain from step to step.
    BowEntry cur = bow_entry(l1, f1, lane, T.na);
    for (int blk = 0; blk < T.na; blk += BOW_WAVE) {
        const BowEntry nxt = bow_entry(l1, f1, blk + BOW_WAVE + lane, T.na);
        int r_key = 0, r_b2 = 0, r_status = 0;
        // the entries of the block with a point, in list order (the others keep the host's LBA_BOW_NO_POINT)
        for (unsigned long long todo = __ballot(cur.has); todo; todo &= todo - 1) {
            const int s = __builtin_ctzll(todo);
            uint4 d0, d1;
            d0.x = __builtin_amdgcn_readlane(cur.d0.x, s); d0.y = __builtin_amdgcn_readlane(cur.d0.y, s);
            d0.z = __builtin_amdgcn_readlane(cur.d0.z, s); d0.w = __builtin_amdgcn_readlane(cur.d0.w, s);
            d1.x = __builtin_amdgcn_readlane(cur.d1.x, s); d1.y = __builtin_amdgcn_readlane(cur.d1.y, s);
            d1.z = __builtin_amdgcn_readlane(cur.d1.z, s); d1.w = __builtin_amdgcn_readlane(cur.d1.w, s);
            BowBest best;
            for (int k = 0; k < nk_lds; ++k) {
                const int c = lane + BOW_WAVE * k;
                const int dist = bow_dist(d0, d1, sd0[c], sd1[c]);
                bow_fold(best, (skip >> k) & 1u ? BOW_NONE : dist, c);
            }
            for (int k = nk_lds; k < nk; ++k) {   // behind the LDS cap: from global memory
                const int c = lane + BOW_WAVE * k;
                if ((skip >> k) & 1u) continue;
                const uint4* d = desc_of(f2 + l2[c]);
                bow_fold(best, bow_dist(d0, d1, d[0], d[1]), c);
            }
            // the best: the smallest (distance, position); the second best: the smallest of the winner's second and
            // every loser's best (with no candidate anywhere all keys are equal and everything is 256)
            int key = bow_key(best.b1, best.pos1), second = best.b2;
            wave_merge(key, second);
            const int kmin = __builtin_amdgcn_readfirstlane(key), b2 = __builtin_amdgcn_readfirstlane(second);
            const int pos = kmin & 0xffff;
            const int status = bow_accept(kmin >> 16, b2, A.mode, A.th_low, A.nn_ratio);
            if (status == LBA_BOW_OK && lane == (pos & (BOW_WAVE - 1))) skip |= 1u << (pos / BOW_WAVE);
            if (lane == s) {
                r_key = kmin;
                r_b2 = b2;
                r_status = status;
            }
        }
        if (cur.has) {
            const int pos = r_key & 0xffff;
            const int idx2 = pos == BOW_NO_POS ? -1 : l2[pos];
            A.rows[(size_t)T.row0 + cur.idx] = lba_bow_row{idx2, r_key >> 16, r_b2, r_status};
        }
        cur = nxt;
    }
}

int refuse(lba_tracker* t, const char* msg) { return tracker_fail(t, {LBA_E_ARG, msg}); }

}  // namespace

extern "C" int lba_match_bow_profile(lba_tracker* t, int32_t on, double* last_ms) {
    return t ? t->bow_timer.profile(on, last_ms, 1) : LBA_E_ARG;
}

extern "C" int lba_match_bow(lba_tracker* t, lba_bow_pair* pairs, int32_t n_pairs, lba_bow_row* out, int32_t n_out,
                             const lba_epi_kf* ekfs, int32_t n_kf, const lba_epi_feat* feats, int32_t n_feats,
                             const int32_t* node_id, const int32_t* node_start, int32_t n_node_rows,
                             const int32_t* node_feat, int32_t n_node_feat, const lba_bow_params* prm_in) {
    if (!t) return LBA_E_ARG;
    if (n_pairs < 0 || n_out < 0 || n_kf < 0 || n_feats < 0 || n_node_rows < 0 || n_node_feat < 0)
        return refuse(t, "a negative count");
    if ((n_pairs && !pairs) || (n_out && !out) || !ekfs || (n_feats && !feats) ||
        (n_node_rows && (!node_id || !node_start)) || (n_node_feat && !node_feat))
        return refuse(t, "a null array");
    const lba_bow_params prm = bow_params_or_default(prm_in);
    if (prm.mode != LBA_BOW_KF && prm.mode != LBA_BOW_FRAME) return refuse(t, "an unknown mode");
    if (prm.th_low < 0 || prm.th_low > 255) return refuse(t, "th_low outside [0, 255]");
    if (!std::isfinite(prm.nn_ratio)) return refuse(t, "nn_ratio is not finite");
    // ---- checks first: a refused call writes nothing.  The keyframes' arrays as lba_match_epipolar checks them.
    {
        std::vector<char> seen;
        for (int k = 0; k < n_kf; ++k) {
            const lba_epi_kf& E = ekfs[k];
            if (E.feat0 < 0 || E.n_feat < 0 || (int64_t)E.feat0 + E.n_feat > n_feats) return refuse(t, "a keyframe's features outside feats");
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
            const lba_bow_pair& P = pairs[p];
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
    if (n_rows > 0x7fffffff) return tracker_fail(t, {LBA_E_LIMIT, "the batch's rows exceed 2 GB"});
    // ---- per pair the merge walk of the two node lists (both strictly ascending, so stepping the smaller side visits
    // the nodes FeatureVector::lower_bound would): the rows that run no inner loop, and one task per common node with
    // a point on side 1 and a candidate on side 2.  Nothing of the caller's is written before the walk is through.
    std::vector<BowTask> tasks;
    int max_nb = 1;
    std::vector<lba_bow_row> pre(n_rows, bow_blank_row(LBA_BOW_NO_NODE));
    {
        size_t row0 = 0;
        for (int p = 0; p < n_pairs; ++p) {
            const lba_epi_kf &E1 = ekfs[pairs[p].kf1], &E2 = ekfs[pairs[p].kf2];
            const int32_t *id1 = node_id + E1.node0, *id2 = node_id + E2.node0;
            const int32_t *s1 = node_start + E1.node0, *s2 = node_start + E2.node0;
            for (int a = 0, b = 0; a < E1.n_node && b < E2.n_node;) {
                if (id1[a] < id2[b]) { ++a; continue; }
                if (id1[a] > id2[b]) { ++b; continue; }
                const int nb = s2[b + 1] - s2[b];
                if (nb > LBA_BOW_MAX_NODE)
                    return tracker_fail(t, {LBA_E_LIMIT, "a side-2 node list longer than LBA_BOW_MAX_NODE"});
                int with_point = 0;
                for (int k = s1[a]; k < s1[a + 1]; ++k) {
                    const int idx1 = node_feat[E1.nf0 + k];
                    const bool has = feats[E1.feat0 + idx1].has_point != 0;
                    pre[row0 + idx1] = bow_blank_row(has ? LBA_BOW_NO_CAND : LBA_BOW_NO_POINT);   // (NO_CAND: an empty list)
                    with_point += has;
                }
                if (with_point && nb) max_nb = std::max(max_nb, nb);
                if (with_point && nb)
                    tasks.push_back(BowTask{E1.nf0 + s1[a], s1[a + 1] - s1[a], E2.nf0 + s2[b], nb, E1.feat0, E2.feat0, (int)row0, 0});
                ++a;
                ++b;
            }
            row0 += (size_t)E1.n_feat;
        }
    }
    if (n_rows == 0) {   // no pair, or only pairs whose side 1 has no feature
        for (int p = 0; p < n_pairs; ++p) pairs[p].n_matches = 0;
        return LBA_OK;
    }
    const size_t n_tasks = tasks.size();
    // ---- the arena: the rows are an input too (their pre-fill goes up), then come back
    ArenaPlan plan;
    const Sec<BowTask> o_tasks = plan.in<BowTask>(n_tasks);
    const Sec<lba_epi_feat> o_feats = plan.in<lba_epi_feat>((size_t)n_feats);
    const Sec<int> o_nf = plan.in<int>((size_t)n_node_feat);
    const Sec<lba_bow_row> o_rows = plan.out<lba_bow_row>(n_rows);
    if (n_tasks > 0x7fffffff || plan.over_2gb())
        return tracker_fail(t, {LBA_E_LIMIT, "the batch's keyframes, tasks and rows exceed 2 GB"});
    char* h = nullptr;
    try {
        ArenaCall call{t, plan, t->bow_timer};
        h = call.pin();
        if (n_tasks) std::memcpy(o_tasks.at(h), tasks.data(), n_tasks * sizeof(BowTask));
        if (n_feats) std::memcpy(o_feats.at(h), feats, (size_t)n_feats * sizeof(lba_epi_feat));
        if (n_node_feat) std::memcpy(o_nf.at(h), node_feat, (size_t)n_node_feat * sizeof(int));
        std::memcpy(o_rows.at(h), pre.data(), n_rows * sizeof(lba_bow_row));
        if (n_tasks) {   // (no task anywhere: the pre-fill is the result)
            char* d = call.place();
            // the upload of ArenaCall::upload, extended over the pre-filled rows
            TR_HIP(hipMemcpyAsync(d, h, plan.down_end, hipMemcpyHostToDevice, t->stream));
            constexpr int per_wg = BOW_WG / BOW_WAVE;
            const int lds_chunks = (std::min(max_nb, BOW_LDS_CAP) + BOW_WAVE - 1) / BOW_WAVE;
            const size_t lds_bytes = (size_t)per_wg * 2 * lds_chunks * BOW_WAVE * sizeof(uint4);   // <= 64 KB
            BowArgs a{o_tasks.at(d), o_feats.at(d), o_nf.at(d), o_rows.at(d), (int)n_tasks, prm.mode, prm.th_low, prm.nn_ratio,
                      lds_chunks};
            call.mark();
            hipLaunchKernelGGL(k_bow_match, dim3((unsigned)((n_tasks + per_wg - 1) / per_wg)), dim3(BOW_WG), lds_bytes, t->stream, a);
            TR_HIP(hipGetLastError());
            call.mark();
            call.finish();
        }
    } catch (const TrackerError& e) {
        return tracker_fail(t, e);
    }
    // ---- per pair: the rotation pass and nmatches on the host, the rows into `out`
    lba_bow_row* r = o_rows.at(h);
    for (int p = 0; p < n_pairs; ++p) {
        const lba_epi_kf &E1 = ekfs[pairs[p].kf1], &E2 = ekfs[pairs[p].kf2];
        pairs[p].n_matches = bow_finish(feats + E1.feat0, E1.n_feat, feats + E2.feat0, prm.check_orientation != 0, r);
        if (E1.n_feat) std::memcpy(out + pairs[p].out0, r, (size_t)E1.n_feat * sizeof(lba_bow_row));
        r += E1.n_feat;
    }
    return LBA_OK;
}
