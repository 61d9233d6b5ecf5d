// lba_match.hip — ORBmatcher's two projection searches (src/ORBmatcher.cc:43-217 and :1439-1568) for a batch of frames:
// the descriptor matching that makes the inputs of lba_track and lba_track_vel_ransac.
//
// Two launches.  k_match_gather gives ONE WAVE to each job: the job's record is wave-uniform, the wave walks the
// columns of its cell rectangle (in the CSR a column's cells [ix][y0 .. y1] are one contiguous span of cell_feat), 64
// candidate slots at a time; lane l gates slot l, computes the Hamming distance as eight popcounts, and one ballot per
// chunk compacts the survivors IN ORDER into the job's list in the arena.  The host has summed the same spans with
// the same four float expressions (lba_match_math.hpp), so no list can overflow.  No scratch, no atomics.
// k_match_resolve gives one workgroup to each (search, camera): a job depends on earlier jobs only through the taken
// features of its own camera, and the sequential loop is reproduced exactly in rounds (see the kernel).  The rotation
// pass and the counts run on the host after the download (match_finish).  Nothing waits on another workgroup; the two
// launches in stream order are the only ordering.  One upload, one download.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_match_math.hpp"
#include "lba_tracker.hpp"

using namespace lba;

namespace {

constexpr int MG_WG = 64;     // k_match_gather: one wave
constexpr int MR_WG = 256;    // k_match_resolve
constexpr int MR_WORDS = LBA_MATCH_MAX_FEAT / 32;
static_assert(sizeof(lba_match_feat) == 64 && sizeof(lba_match_job) == 96 && sizeof(lba_match_cam) == 20 &&
              sizeof(lba_match_search) == 40 && sizeof(lba_match_params) == 24, "ABI layout");
static_assert(LBA_MATCH_MAX_FEAT == 8192, "match_pack keeps the camera-local feature index in 13 bits");

struct MatchCamRec {   // one (search, camera)
    int jobs0, n_jobs;     // its jobs in cam_jobs, in job order
    int feats0, n_feat;    // its features in cam_feats, by camera-local index
    int job0, feat0;       // the search's first job and feature
};

struct MatchArgs {
    const lba_match_search* searches;
    const lba_match_cam* cams;
    const int* cell_start;
    const int* cell_feat;
    const lba_match_feat* feats;
    const lba_match_job* jobs;
    const int* job_search;     // [n_jobs]: the job's search, -1 for a job no search covers
    const int* feat_local;     // [n_feats]: the feature's index within its camera
    const unsigned* list_off;  // [n_jobs + 1]: the job's candidate list in `cand`
    const MatchCamRec* camrec;
    const int* cam_jobs;
    const int* cam_feats;
    uint32_t* cand;            // work
    int* n_cand;               // work [n_jobs]
    int* status;               // out [4][n_jobs]: status, feat, best_dist, best_dist2
    int* feat_job;             // out [n_feats]
    int* rounds;               // out [n_camrec]
    int n_jobs;
    int mode, th_high, stereo_cam, ur_truncate;
    float nn_ratio;
};

__global__ __launch_bounds__(MG_WG) void k_match_gather(MatchArgs A) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int s = A.job_search[g];
    if (s < 0) return;
    const lba_match_search S = A.searches[s];
    const lba_match_job* J = A.jobs + g;
    const int cam = J->cam;
    const lba_match_cam C = A.cams[S.cam0 + cam];
    const MatchJobGate G{J->x, J->y, J->radius, J->ur, J->min_level, J->max_level, cam == A.stereo_cam,
                         A.ur_truncate != 0};
    uint32_t desc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) desc[i] = J->desc[i];
    const unsigned off = A.list_off[g], cap = A.list_off[g + 1] - off;
    unsigned count = 0;
    MatchRect R;
    if (match_rect(G.x, G.y, G.radius, C, &R) && R.y0 <= R.y1) {
        const int* cs = A.cell_start + S.cell0 + cam * MATCH_CELLS;
        const int* cf = A.cell_feat + S.cf0;
        for (int ix = R.x0; ix <= R.x1; ++ix) {
            const int b = cs[ix * MATCH_ROWS + R.y0], e = cs[ix * MATCH_ROWS + R.y1 + 1];
            for (int k = b; k < e; k += MG_WG) {
                const int i = k + lane;
                bool ok = false;
                uint32_t w = 0;
                if (i < e) {
                    const int f = S.feat0 + cf[i];
                    const lba_match_feat* F = A.feats + f;
                    const int octave = F->octave;
                    ok = match_gate(G, F->x, F->y, octave, F->u_right);
                    if (ok) w = match_pack(A.feat_local[f], match_dist(desc, F->desc), octave);
                }
                const unsigned long long mask = __ballot(ok);
                if (ok) {
                    const unsigned pos = count + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
                    if (pos < cap) A.cand[off + pos] = w;   // pos < cap always: the host counted the same spans
                }
                count += (unsigned)__popcll(mask);
            }
        }
    }
    if (lane == 0) {
        A.n_cand[g] = (int)(count < cap ? count : cap);
        A.status[g] = MATCH_PENDING;
    }
}

// The sequential loop of one camera, exactly, in rounds.  LDS: a taken bit per feature and a word min_pending[f].
// Per round, (A) every pending job k does atomicMin(min_pending[f], k) on each of its candidates that is not taken;
// (B) a pending job whose untaken candidates all read back k is FINAL: it scans its list in order, skipping taken
// features, applies its mode's rule, and on LBA_MATCH_OK writes fjob[f] = k and, if it blocks, the taken bit.
//  1. Two jobs final in the same round have disjoint untaken candidates (a shared one reads back the smaller of the
//     two), so their writes cannot meet, and neither sees the other's taken bit: the bits are double-buffered and a
//     round reads those of its start.
//  2. A job is final only when no earlier pending job shares an untaken candidate with it, so every earlier job that
//     could take one of its candidates, or be overwritten by it, has been decided: fjob[f] is written in job order and
//     the job sees exactly the taken set the sequential loop shows it.
//  3. The smallest pending job is always final, so every round decides at least one job: at most n_jobs rounds.
// k here is the job's position among its camera's jobs.  The loop is bounded by that count and waits on nothing.
__global__ __launch_bounds__(MR_WG) void k_match_resolve(MatchArgs A) {
    __shared__ int minp[LBA_MATCH_MAX_FEAT];
    __shared__ int fjob[LBA_MATCH_MAX_FEAT];
    __shared__ unsigned tk[2][MR_WORDS];
    const int tid = threadIdx.x;
    const MatchCamRec C = A.camrec[blockIdx.x];
    const int* cam_jobs = A.cam_jobs + C.jobs0;
    const int* cam_feats = A.cam_feats + C.feats0;
    tk[0][tid] = 0u;
    __syncthreads();
    for (int i = tid; i < C.n_feat; i += MR_WG) {
        minp[i] = INT_MAX;
        fjob[i] = -1;
        if (A.feats[cam_feats[i]].taken != 0) atomicOr(&tk[0][i >> 5], 1u << (i & 31));
    }
    __syncthreads();
    tk[1][tid] = tk[0][tid];
    __syncthreads();
    int rounds = 0;
    while (rounds < C.n_jobs) {
        int any = 0;
        for (int p = tid; p < C.n_jobs; p += MR_WG) {
            const int g = cam_jobs[p];
            if (A.status[g] != MATCH_PENDING) continue;
            any = 1;
            const uint32_t* cand = A.cand + A.list_off[g];
            const int n = A.n_cand[g];
            for (int i = 0; i < n; ++i) {
                const int l = match_local(cand[i]);
                if (!((tk[0][l >> 5] >> (l & 31)) & 1u)) atomicMin(&minp[l], p);
            }
        }
        if (!__syncthreads_or(any)) break;
        ++rounds;
        for (int p = tid; p < C.n_jobs; p += MR_WG) {
            const int g = cam_jobs[p];
            if (A.status[g] != MATCH_PENDING) continue;
            const uint32_t* cand = A.cand + A.list_off[g];
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
                match_pick(pk, A.mode, match_wdist(w), match_octave(w), l);
            }
            if (!fin) continue;
            const int st = match_decide(pk, A.mode, A.th_high, A.nn_ratio);
            const size_t nj = (size_t)A.n_jobs;
            A.status[g] = st;
            A.status[nj + g] = st == LBA_MATCH_OK ? cam_feats[pk.idx] - C.feat0 : -1;
            A.status[2 * nj + g] = pk.best;
            A.status[3 * nj + g] = pk.best2;
            if (st == LBA_MATCH_OK) {
                fjob[pk.idx] = g - C.job0;
                if (A.jobs[g].blocks != 0) atomicOr(&tk[1][pk.idx >> 5], 1u << (pk.idx & 31));
            }
        }
        __syncthreads();
        for (int i = tid; i < C.n_feat; i += MR_WG) minp[i] = INT_MAX;
        tk[0][tid] = tk[1][tid];
        __syncthreads();
    }
    for (int i = tid; i < C.n_feat; i += MR_WG) A.feat_job[cam_feats[i]] = fjob[i];
    if (tid == 0) A.rounds[blockIdx.x] = rounds;
}

#define MATCH_REFUSE(c, m) return tracker_fail(t, TrackerError{c, m})

}  // namespace

extern "C" int lba_match_profile(lba_tracker* t, int32_t on, double* last_ms) {
    return t ? t->match_timer.profile(on, last_ms, 2) : LBA_E_ARG;
}

extern "C" int lba_match_project(lba_tracker* t, lba_match_search* searches, int32_t n_searches, lba_match_cam* cams,
                                 int32_t n_cams, const int32_t* cell_start, int32_t n_cell_start,
                                 const int32_t* cell_feat, int32_t n_cell_feat, lba_match_feat* feats, int32_t n_feats,
                                 lba_match_job* jobs, int32_t n_jobs, const lba_match_params* prm) {
    if (!t) return LBA_E_ARG;
    if (n_searches < 0 || n_cams < 0 || n_cell_start < 0 || n_cell_feat < 0 || n_feats < 0 || n_jobs < 0)
        MATCH_REFUSE(LBA_E_ARG, "lba_match_project: a negative count");
    if (!prm || (n_searches && !searches) || (n_cams && !cams) || (n_cell_start && !cell_start) ||
        (n_cell_feat && !cell_feat) || (n_feats && !feats) || (n_jobs && !jobs))
        MATCH_REFUSE(LBA_E_ARG, "lba_match_project: a null array");
    const lba_match_params P = *prm;
    if (P.mode != LBA_MATCH_RATIO && P.mode != LBA_MATCH_BEST) MATCH_REFUSE(LBA_E_ARG, "lba_match_project: unknown mode");
    if (P.th_high < 0 || P.th_high > 255) MATCH_REFUSE(LBA_E_ARG, "lba_match_project: th_high outside [0, 255]");
    if (P.nn_ratio != P.nn_ratio) MATCH_REFUSE(LBA_E_ARG, "lba_match_project: nn_ratio is not a number");
    if (P.check_orientation && P.mode != LBA_MATCH_BEST)
        MATCH_REFUSE(LBA_E_ARG, "lba_match_project: check_orientation needs LBA_MATCH_BEST");
    // ---- checks first: a refused call writes nothing
    size_t n_camrec = 0;
    {
        int cam_end = 0, feat_end = 0, job_end = 0;
        for (int s = 0; s < n_searches; ++s) {
            const lba_match_search& S = searches[s];
            if (S.n_cam < 1 || S.cam0 < cam_end || (int64_t)S.cam0 + S.n_cam > n_cams)
                MATCH_REFUSE(LBA_E_ARG, "lba_match_project: a search's cameras outside the array or overlapping the search before");
            if (S.n_feat < 0 || S.feat0 < feat_end || (int64_t)S.feat0 + S.n_feat > n_feats)
                MATCH_REFUSE(LBA_E_ARG, "lba_match_project: a search's features outside the array or overlapping the search before");
            if (S.n_jobs < 0 || S.job0 < job_end || (int64_t)S.job0 + S.n_jobs > n_jobs)
                MATCH_REFUSE(LBA_E_ARG, "lba_match_project: a search's jobs outside the array or overlapping the search before");
            cam_end = S.cam0 + S.n_cam; feat_end = S.feat0 + S.n_feat; job_end = S.job0 + S.n_jobs;
            const int64_t n_cells = (int64_t)S.n_cam * MATCH_CELLS;
            if (S.cell0 < 0 || S.cell0 + n_cells + 1 > n_cell_start)
                MATCH_REFUSE(LBA_E_ARG, "lba_match_project: a search's cell_start outside the array");
            if (P.stereo_cam < -1 || P.stereo_cam >= S.n_cam)
                MATCH_REFUSE(LBA_E_ARG, "lba_match_project: stereo_cam outside [-1, n_cam)");
            const int32_t* cs = cell_start + S.cell0;
            if (cs[0] != 0) MATCH_REFUSE(LBA_E_ARG, "lba_match_project: cell_start does not begin at 0");
            for (int64_t c = 0; c < n_cells; ++c)
                if (cs[c + 1] < cs[c]) MATCH_REFUSE(LBA_E_ARG, "lba_match_project: cell_start decreases");
            if (S.cf0 < 0 || (int64_t)S.cf0 + cs[n_cells] > n_cell_feat)
                MATCH_REFUSE(LBA_E_ARG, "lba_match_project: a search's cell_feat outside the array");
            const lba_match_feat* F = feats + S.feat0;
            for (int f = 0; f < S.n_feat; ++f)
                if (F[f].cam < 0 || F[f].cam >= S.n_cam || F[f].octave < 0 || F[f].octave > 255)
                    MATCH_REFUSE(LBA_E_ARG, "lba_match_project: a feature's camera outside [0, n_cam) or octave outside [0, 255]");
            const int32_t* cf = cell_feat + S.cf0;
            for (int c = 0; c < S.n_cam; ++c)
                for (int k = cs[(size_t)c * MATCH_CELLS]; k < cs[(size_t)(c + 1) * MATCH_CELLS]; ++k)
                    if (cf[k] < 0 || cf[k] >= S.n_feat || F[cf[k]].cam != c)
                        MATCH_REFUSE(LBA_E_ARG, "lba_match_project: a cell names a feature outside the search or of another camera");
            const lba_match_job* J = jobs + S.job0;
            for (int k = 0; k < S.n_jobs; ++k) {
                if (J[k].cam < 0 || J[k].cam >= S.n_cam)
                    MATCH_REFUSE(LBA_E_ARG, "lba_match_project: a job's camera outside [0, n_cam)");
                if (J[k].max_level >= 0 && J[k].min_level > J[k].max_level)
                    MATCH_REFUSE(LBA_E_ARG, "lba_match_project: a job's level range is not ordered");
            }
            n_camrec += (size_t)S.n_cam;
        }
        // the limit after the argument checks: features per camera
        std::vector<int> per_cam;
        for (int s = 0; s < n_searches; ++s) {
            const lba_match_search& S = searches[s];
            per_cam.assign(S.n_cam, 0);
            for (int f = 0; f < S.n_feat; ++f)
                if (++per_cam[feats[S.feat0 + f].cam] > LBA_MATCH_MAX_FEAT)
                    MATCH_REFUSE(LBA_E_LIMIT, "lba_match_project: more than 8192 features in one camera");
        }
    }
    if (n_searches == 0) return LBA_OK;
    // ---- the arena: inputs (one upload), outputs (one download), work; the pinned image covers inputs and outputs
    const size_t nj = (size_t)n_jobs, nf = (size_t)n_feats;
    ArenaPlan plan;
    const Sec<lba_match_search> o_searches = plan.in<lba_match_search>((size_t)n_searches);
    const Sec<lba_match_cam> o_cams = plan.in<lba_match_cam>((size_t)n_cams);
    const Sec<int32_t> o_cs = plan.in<int32_t>((size_t)n_cell_start), o_cf = plan.in<int32_t>((size_t)n_cell_feat);
    const Sec<lba_match_feat> o_feats = plan.in<lba_match_feat>(nf);
    const Sec<lba_match_job> o_jobs = plan.in<lba_match_job>(nj);
    const Sec<int> o_jsearch = plan.in<int>(nj), o_flocal = plan.in<int>(nf);
    const Sec<unsigned> o_loff = plan.in<unsigned>(nj + 1);
    const Sec<MatchCamRec> o_camrec = plan.in<MatchCamRec>(n_camrec);
    const Sec<int> o_cjobs = plan.in<int>(nj), o_cfeats = plan.in<int>(nf);
    const Sec<int> o_status = plan.out<int>(4 * nj), o_fjob = plan.out<int>(nf), o_rounds = plan.out<int>(n_camrec);
    const Sec<int> o_ncand = plan.work<int>(nj);
    if (plan.over_2gb()) MATCH_REFUSE(LBA_E_LIMIT, "lba_match_project: the batch exceeds 2 GB");
    char* h = nullptr;
    try {
        ArenaCall call{t, plan, t->match_timer};
        h = call.pin();
        std::memcpy(o_searches.at(h), searches, (size_t)n_searches * sizeof(lba_match_search));
        if (n_cams) std::memcpy(o_cams.at(h), cams, (size_t)n_cams * sizeof(lba_match_cam));
        if (n_cell_start) std::memcpy(o_cs.at(h), cell_start, (size_t)n_cell_start * sizeof(int32_t));
        if (n_cell_feat) std::memcpy(o_cf.at(h), cell_feat, (size_t)n_cell_feat * sizeof(int32_t));
        if (nf) std::memcpy(o_feats.at(h), feats, nf * sizeof(lba_match_feat));
        if (nj) std::memcpy(o_jobs.at(h), jobs, nj * sizeof(lba_match_job));
        int *jsearch = o_jsearch.at(h), *flocal = o_flocal.at(h), *cjobs = o_cjobs.at(h), *cfeats = o_cfeats.at(h);
        unsigned* loff = o_loff.at(h);
        MatchCamRec* camrec = o_camrec.at(h);
        for (size_t g = 0; g < nj; ++g) jsearch[g] = -1;
        for (size_t g = 0; g <= nj; ++g) loff[g] = 0;   // capacities first, offsets by the prefix sum below
        for (size_t f = 0; f < nf; ++f) flocal[f] = 0;
        size_t r = 0, at_j = 0, at_f = 0;
        std::vector<int> fill;
        for (int s = 0; s < n_searches; ++s) {
            const lba_match_search& S = searches[s];
            // a camera's jobs and features, each in its own order
            for (int c = 0; c < S.n_cam; ++c) camrec[r + c] = MatchCamRec{0, 0, 0, 0, S.job0, S.feat0};
            for (int k = 0; k < S.n_jobs; ++k) ++camrec[r + jobs[S.job0 + k].cam].n_jobs;
            for (int f = 0; f < S.n_feat; ++f) ++camrec[r + feats[S.feat0 + f].cam].n_feat;
            for (int c = 0; c < S.n_cam; ++c) {
                camrec[r + c].jobs0 = (int)at_j; at_j += (size_t)camrec[r + c].n_jobs;
                camrec[r + c].feats0 = (int)at_f; at_f += (size_t)camrec[r + c].n_feat;
            }
            fill.assign(S.n_cam, 0);
            for (int k = 0; k < S.n_jobs; ++k) {
                const int g = S.job0 + k, c = jobs[g].cam;
                cjobs[camrec[r + c].jobs0 + fill[c]++] = g;
                jsearch[g] = s;
                loff[g + 1] = (unsigned)match_capacity(jobs[g], cams[S.cam0 + c], cell_start + S.cell0);
            }
            fill.assign(S.n_cam, 0);
            for (int f = 0; f < S.n_feat; ++f) {
                const int g = S.feat0 + f, c = feats[g].cam;
                flocal[g] = fill[c];
                cfeats[camrec[r + c].feats0 + fill[c]++] = g;
            }
            r += (size_t)S.n_cam;
        }
        uint64_t total = 0;
        for (size_t g = 0; g < nj; ++g) {
            total += loff[g + 1];
            if (total > 0x7fffffffu) throw TrackerError{LBA_E_LIMIT, "lba_match_project: the batch exceeds 2 GB"};
            loff[g + 1] = (unsigned)total;
        }
        // the candidate lists: their size is known only now, from the filled image
        const Sec<uint32_t> o_cand = plan.work<uint32_t>((size_t)total);
        if (plan.over_2gb()) throw TrackerError{LBA_E_LIMIT, "lba_match_project: the batch exceeds 2 GB"};
        char* d = call.place();
        call.upload();
        MatchArgs a;
        a.searches = o_searches.at(d); a.cams = o_cams.at(d); a.cell_start = o_cs.at(d); a.cell_feat = o_cf.at(d);
        a.feats = o_feats.at(d); a.jobs = o_jobs.at(d); a.job_search = o_jsearch.at(d); a.feat_local = o_flocal.at(d);
        a.list_off = o_loff.at(d); a.camrec = o_camrec.at(d); a.cam_jobs = o_cjobs.at(d); a.cam_feats = o_cfeats.at(d);
        a.cand = o_cand.at(d); a.n_cand = o_ncand.at(d);
        a.status = o_status.at(d); a.feat_job = o_fjob.at(d); a.rounds = o_rounds.at(d);
        a.n_jobs = n_jobs;
        a.mode = P.mode; a.th_high = P.th_high; a.stereo_cam = P.stereo_cam; a.ur_truncate = P.ur_truncate;
        a.nn_ratio = P.nn_ratio;
        hipStream_t st = t->stream;
        call.mark();
        if (n_jobs) {
            hipLaunchKernelGGL(k_match_gather, dim3((unsigned)n_jobs), dim3(MG_WG), 0, st, a);
            TR_HIP(hipGetLastError());
        }
        call.mark();
        hipLaunchKernelGGL(k_match_resolve, dim3((unsigned)n_camrec), dim3(MR_WG), 0, st, a);
        TR_HIP(hipGetLastError());
        call.mark();
        call.finish();
    } catch (const TrackerError& e) {
        return tracker_fail(t, e);
    }
    // ---- scatter: the jobs' and features' outputs, the cameras' rounds; then the rotation pass and the counts
    const int *r_status = o_status.at(h), *r_fjob = o_fjob.at(h), *r_rounds = o_rounds.at(h);
    size_t r = 0;
    for (int s = 0; s < n_searches; ++s) {
        lba_match_search& S = searches[s];
        for (int k = 0; k < S.n_jobs; ++k) {
            const size_t g = (size_t)S.job0 + k;
            jobs[g].status = r_status[g];
            jobs[g].feat = r_status[nj + g];
            jobs[g].best_dist = r_status[2 * nj + g];
            jobs[g].best_dist2 = r_status[3 * nj + g];
        }
        for (int f = 0; f < S.n_feat; ++f) feats[S.feat0 + f].job = r_fjob[S.feat0 + f];
        for (int c = 0; c < S.n_cam; ++c) cams[S.cam0 + c].rounds = r_rounds[r + c];
        r += (size_t)S.n_cam;
        match_finish(S, P, jobs + S.job0, feats + S.feat0);
    }
    return LBA_OK;
}
