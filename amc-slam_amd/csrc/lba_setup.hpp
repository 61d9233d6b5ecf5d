// lba_setup.hpp — the host stages of lba_set_problem: the caller's window into the layout every kernel reads
// (activity and numbering, GP pairs and samples, landmark order, tiles, slab slots, device-order observations).
// Host code only: no HIP runtime call, no lba_problem.  set_problem (lba_host.hip) runs the stages in order and
// uploads their outputs; each stage reads the earlier stages' structs (const) and returns its own.  The
// observation-sized arrays live in SetupScratch, which the caller keeps between windows.
//
// Every parallel pass splits its work into a fixed number of pieces (SETUP_PIECES; piece_range), so the layout
// never depends on the thread count.
#pragma once

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_device.hpp"
#include "lba_math.hpp"

namespace lba_setup {

using namespace lba;

struct ApiError {
    int code;
    std::string msg;
};

// f(i) for i in [0, n) on up to SETUP_THREADS_MAX (16) host threads, at most the CPUs this process may run on
// (LBA_SETUP_THREADS overrides; 1: serial).  Round 3 measured 16 threads no faster than 8
// (profiles/r3ai_setup_threads.txt); round 4's parallel tile-list concatenation and device-order records made
// the 16-piece passes scale, and 16 is the default since (profiles/r4z_setup_phases.txt).  Callers split work into a fixed number of pieces, so the
// results never depend on the thread count.  The workers persist (a set-up makes a dozen parallel passes;
// spawning threads per pass cost ~0.1 ms each) and, after a pass, poll for the next one for a while before
// they sleep: a set-up's passes follow each other within a millisecond, and an OS wake-up of the workers per
// pass cost more than many of the passes themselves.  Pieces are claimed from one counter that packs
// (pass, piece), so a worker that arrives late takes no piece of a later pass for an earlier one; the caller
// waits for the pieces to be finished, not for every worker to have looked in.  A pass that finds the pool
// busy (another problem setting up on another thread) runs on its caller's thread alone.
constexpr int SETUP_THREADS_MAX = 16;
// the fixed number of pieces every parallel pass of the set-up splits its work into (the results do not depend on
// the thread count; tiles never straddle a piece boundary)
constexpr int SETUP_PIECES = 16;
class SetupPool {
  public:
    static SetupPool& get() {
        static SetupPool pool;
        return pool;
    }
    int size() const { return (int)workers_.size() + 1; }
    // false: the pool is in use (the caller runs the pass itself)
    template <class F>
    bool run(int n, F& f) {
        std::unique_lock<std::mutex> busy(busy_, std::try_to_lock);
        if (!busy.owns_lock()) return false;
        std::function<void(int)> job = [&](int i) { f(i); };
        job_ = &job;
        n_.store(n, std::memory_order_relaxed);
        done_.store(0, std::memory_order_relaxed);
        err_ = nullptr;
        const unsigned long long g = ++pass_;
        {
            std::lock_guard<std::mutex> lk(m_);
            claim_.store(g << 32, std::memory_order_release);   // publishes job_ / n_ with the pass number
        }
        cv_.notify_all();
        work(g);   // the caller takes pieces too
        for (int spins = 0; done_.load(std::memory_order_acquire) < n; ++spins)
            if (spins > 4096) std::this_thread::yield();
        // close the pass before any field of the next one is written: a worker that loaded this pass's
        // last claim word (every piece taken) and was preempted before its bound check would otherwise
        // pass that check against the next pass's larger n_ and win its CAS against the unchanged word,
        // running a piece of the next job ahead of its publication
        claim_.store((g << 32) | CLOSED, std::memory_order_release);
        job_ = nullptr;
        if (err_) std::rethrow_exception(err_);
        return true;
    }

  private:
    static constexpr int POLL_US = 3000;   // how long an idle worker polls for the next pass before it sleeps
    static constexpr unsigned long long CLOSED = 0x7fffffffull;   // piece word of a finished pass (>= any n)
    SetupPool() {
        const char* e = std::getenv("LBA_SETUP_THREADS");
        const int v = e ? std::atoi(e) : 0;
        int avail = (int)std::thread::hardware_concurrency();
        cpu_set_t cs;
        if (sched_getaffinity(0, sizeof(cs), &cs) == 0) avail = std::min(avail > 0 ? avail : CPU_COUNT(&cs), CPU_COUNT(&cs));
        const int nt = v > 0 ? v : std::max(1, std::min(SETUP_THREADS_MAX, avail));
        for (int t = 1; t < nt; ++t)
            workers_.emplace_back([this] {
                unsigned long long seen = 0;
                while (true) {
                    auto fresh = [&] { return stop_.load(std::memory_order_acquire) ||
                                              (claim_.load(std::memory_order_acquire) >> 32) != seen; };
                    const auto t0 = std::chrono::steady_clock::now();
                    while (!fresh()) {
                        for (int k = 0; k < 64 && !fresh(); ++k) __builtin_ia32_pause();
                        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(POLL_US)) {
                            std::unique_lock<std::mutex> lk(m_);
                            cv_.wait(lk, fresh);
                        }
                    }
                    if (stop_.load(std::memory_order_acquire)) return;
                    seen = claim_.load(std::memory_order_acquire) >> 32;
                    work(seen);
                }
            });
    }
    ~SetupPool() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_.store(true, std::memory_order_release);
        }
        cv_.notify_all();
        for (auto& w : workers_) w.join();
    }
    // claim pieces of pass g until none is left (or the pass is over); every piece claimed is counted done
    void work(unsigned long long g) {
        for (;;) {
            unsigned long long c = claim_.load(std::memory_order_acquire);
            int i;
            do {
                if ((c >> 32) != g || (int)(c & 0xffffffffu) >= n_.load(std::memory_order_relaxed)) return;
                i = (int)(c & 0xffffffffu);
            } while (!claim_.compare_exchange_weak(c, c + 1, std::memory_order_acq_rel, std::memory_order_acquire));
            try {
                (*job_)(i);
            } catch (...) {
                std::lock_guard<std::mutex> lk(m_);
                if (!err_) err_ = std::current_exception();
            }
            done_.fetch_add(1, std::memory_order_acq_rel);
        }
    }
    std::vector<std::thread> workers_;
    std::mutex busy_, m_;
    std::condition_variable cv_;
    std::function<void(int)>* job_ = nullptr;
    std::atomic<int> n_{0};
    unsigned long long pass_ = 0;
    std::atomic<unsigned long long> claim_{0};   // pass << 32 | next piece
    std::atomic<int> done_{0};
    std::atomic<bool> stop_{false};
    std::exception_ptr err_;
};

template <class F>
void par_for(int n, F f) {
    SetupPool& pool = SetupPool::get();
    if (n <= 1 || pool.size() <= 1 || !pool.run(n, f))
        for (int i = 0; i < n; ++i) f(i);
}

// piece `piece` of `pieces` of [0, n): [lo, hi)
struct Range {
    int lo, hi;
};
inline Range piece_range(int n, int piece, int pieces) {
    return {(int)((long long)n * piece / pieces), (int)((long long)n * (piece + 1) / pieces)};
}

inline bool is_gp(int kind) { return kind == LBA_MONO_GP || kind == LBA_STEREO_GP; }
inline int obs_dim(int kind) { return (kind == LBA_STEREO_GP || kind == LBA_STEREO) ? 3 : 2; }

inline int ublock_id(int n_pb, int bi, int bj) { return bi * n_pb - bi * (bi - 1) / 2 + (bj - bi); }

inline void normalize_q(const double* q, double* o) {
    const Quat n = qnormalize(Quat{q[0], q[1], q[2], q[3]});
    o[0] = n.x; o[1] = n.y; o[2] = n.z; o[3] = n.w;
}

// the LDS limits of one k_lin_schur workgroup
inline bool tile_fits(int no, int nr, int npair, int nlmt, int nkf, int ns, int ne) {
    return no <= TILE_OBS && nr <= TILE_ROWS && npair <= TILE_PAIRS && nlmt <= TILE_LMS && nkf <= TILE_KF &&
           ns <= TILE_SMP && ne <= TILE_PROWS;
}

struct Span {
    const int* p; size_t n;
    const int* begin() const { return p; }
    const int* end() const { return p + n; }
    size_t size() const { return n; }
    int operator[](size_t i) const { return p[i]; }
};

// LBA_SETUP_TIMING: wall time of the set-up phases on stderr; sub: finer stamps inside a phase (only then)
struct SetupClock {
    bool on;
    std::chrono::steady_clock::time_point tlast, tsub;
    explicit SetupClock(bool on_) : on(on_), tlast(std::chrono::steady_clock::now()), tsub(tlast) {}
    void sub(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "    %-22s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tsub).count());
        tsub = now;
    }
    double phase(const char* what) {   // ms since the last phase boundary
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - tlast).count();
        if (on) std::fprintf(stderr, "set_problem %-12s %8.3f ms\n", what, ms);
        tlast = tsub = now;
        return ms;
    }
};

// the caller's window (lba_set_problem's arguments)
struct Window {
    const lba_kf* kfs; int n_kf;
    const double* lm_xyz; int n_lm;
    const lba_obs* obs; int n_obs;
    const lba_prior* priors; int n_priors;
    const int32_t* vel_kfs; int n_vel;
    const lba_cam* cams; int n_cam;
};

// Observation-sized host arrays of the stages, kept between calls: resizing to the same length touches nothing
// (no allocation, page faults or zeroing per window; the stage that owns an array writes every element).
// Written by: validate_window (lm_cnt), number_vertices (lo_of), number_gp (smp_of), order_landmarks (obs_of),
// tile_inputs (dhb .. dsmp), the tile passes (ob_row, pair_lk), device_order (ob_*).
struct SetupScratch {
    std::vector<int> lm_cnt;   // [piece][landmark] observation counts, then the pieces' offsets
    std::vector<int> lo_of;    // observations by original landmark (stable)
    std::vector<int> smp_of;   // original observation -> pose sample
    std::vector<int> gp_of, sample_of;   // number_gp's own: a GP observation's pair and GP sample
    std::vector<int> obs_of;   // device observation -> original observation
    // per observation in device order, what the tiling reads (contiguous instead of through obs_of):
    // pose blocks of KF b / KF a / the extrinsic (-1: none or fixed), rows, pose sample
    std::vector<int> dhb, dha, dhx, ddim, dsmp;
    std::vector<int> ob_meta, ob_kfa, ob_kfb, ob_smp, ob_lm;   // the device-order observation arrays
    // the tiles' per-observation LDS row (| tile-local sample << 16 in regular tiles) and, per (KF, landmark) pair,
    // tile-local KF | tile-local landmark << 8 (regular pairs; 0 for a heavy landmark's)
    std::vector<int> ob_row, pair_lk;
    std::vector<int> pair_r0, lm_r0;   // per pair / landmark slot (then the segments'): its run in pair_rows / lm_rows
    std::vector<double> ob_z, ob_w;
};
// The stages' own large work arrays (each allocated and filled by its stage, read by no other).  The caller frees them
// together when the set-up ends, as when the stages were one function: with each freed at the end of its stage (the
// later stages' arrays then take other heap memory) the set-up measured slower on 16 threads
// (profiles/setup_stages_ab.txt).
struct StageWork {
    std::vector<char> kf_act, heavy;
    std::vector<std::vector<std::pair<int, int>>> gp_by_b;
    std::vector<int> lmin, lmax, lm_npl;
    std::vector<int> mcnt, mfill, gcnt, hfill, gfill, gpcnt, sfill, gpfill;
};
template <class T>
std::vector<T>& sized(std::vector<T>& v, size_t n) {   // (contents unspecified: the caller writes every element)
    v.resize(n);
    return v;
}

// ---- stage outputs ------------------------------------------------------------------------------
struct Checks {
    bool lm_hist = false;            // scr.lm_cnt holds the per-piece landmark histogram
    std::vector<char> kf_mark;       // [piece][KF]: an observation of the piece touches it
    std::vector<int> ext_cams;       // cameras with a free extrinsic, ascending (g2o vertex ids iniMPid + c + 1)
};
struct Vertices {
    std::vector<int> lo0;            // per original landmark: its observations in scr.lo_of
    std::vector<char> lm_act;
    std::vector<lba_prior> pri;      // the active motion priors / velocity edges
    std::vector<int> vel;
    int n_ext = 0, n_kfs = 0;        // free extrinsics; KF slots (keyframes, then the extrinsics)
    std::vector<int> cam_slot;       // camera -> its extrinsic's KF slot, or -1
    std::vector<int> kf_hidx;        // KF slot -> pose block, or -1
    int n_pb = 0, n_pb_kf = 0, np = 0, np_ext = 0;
    std::vector<int> pose_ext;
};
struct GpSamples {
    std::vector<int> gp_a, gp_b;     // GP pair -> (prev KF, KF), in order of first appearance
    std::vector<int> gp_s0;          // per pair: its samples, contiguous
    std::vector<double> gps_t;       // per sample: time, camera (-1 unless the camera's extrinsic is free)
    std::vector<int> gps_cam;
    int n_gps = 0, n_smp = 0;        // GP samples; all pose samples (then one per KF slot)
};
struct LmOrder {
    std::vector<int> order;          // device landmark -> original (lm_dev_of: the way back)
    int nl = 0, n_reg = 0;           // device landmarks; the regular ones (heavy landmarks go last)
    std::vector<int> lobs0;          // per device landmark: its observations in scr.obs_of
    std::vector<int> lm_pair0, pair_lm, pair_kf;   // (KF, landmark) pairs per device landmark, ascending pose block
    int n_pairs = 0;
    // the landmark's pose blocks (ascending) = its pairs' blocks
    Span kfs(int d) const { return Span{pair_kf.data() + lm_pair0[d], (size_t)(lm_pair0[d + 1] - lm_pair0[d])}; }
};

// The per-tile descriptors and lists, declared once: a run of consecutive tiles builds its share in one TileLists,
// the runs' shares are concatenated into the window's (concat_runs walks TILE_CATS).  Second column: the list into
// which the values index, so a run's values shift by the run's offset into that list (nullptr: as they are).
#define LBA_TILE_LISTS(X)                                                                                        \
    X(t_obs0, nullptr) X(t_nobs, nullptr) X(t_lm0, nullptr) X(t_nlm, nullptr) X(t_pair0, nullptr)                \
    X(t_npair, nullptr) X(t_smp0, &TileLists::tsm_smp) X(t_nsmp, nullptr) X(t_sent0, &TileLists::sent_l1)        \
    X(t_nsent, nullptr) X(t_kf0, &TileLists::tkf_list) X(t_nkf, nullptr) X(tkf_list, nullptr)                    \
    X(tsm_smp, nullptr) X(tsm_rows, nullptr) X(sent_l1, nullptr) X(sent_l2, nullptr) X(sent_k1, nullptr)         \
    X(sent_k2, nullptr) X(pair_rows, nullptr) X(lm_rows, nullptr)
struct TileLists {
#define X(name, base) std::vector<int> name;
    LBA_TILE_LISTS(X)
#undef X
};
struct TileCat {
    std::vector<int> TileLists::*list;
    std::vector<int> TileLists::*base;
};
#define X(name, base) {&TileLists::name, base},
inline constexpr TileCat TILE_CATS[] = {LBA_TILE_LISTS(X)};
#undef X
constexpr int N_TILE_CATS = (int)(sizeof(TILE_CATS) / sizeof(TILE_CATS[0]));

struct Tiles {
    TileLists l;                     // regular tiles [0, n_stiles), then the heavy landmarks' segment tiles
    // heavy landmarks: segments (landmark slots nl + s), segment pairs (pair slots n_pairs + c) and, per
    // canonical pair of a heavy landmark, the segment pairs that sum into it
    std::vector<int> hv_lm, hv_seg0{0}, hv_hp0{0}, hp_src0{0}, hp_src;
    int n_stiles = 0, n_seg = 0, n_segpairs = 0;
    int n_tiles() const { return (int)l.t_obs0.size(); }
};
struct Slots {
    std::vector<int> ms0, tsm_meta;  // (tile, sample) M / g partials: per sample, its tiles in tile order
    int n_mslots = 0;
    int n_ublocks = 0;
    std::vector<int> ub_i, ub_j;
    std::vector<int> ent_a, ent_b, ent_e, ent_cam;   // Hpp / b_p slab entries
    int n_entries = 0;
    std::vector<int> hcnt, scnt;     // per upper block: Hpp / Schur partials
    std::vector<int> hs0, gs0, seg_slot, seg_gslot, hs_prod, gs_prod;
    std::vector<int> ss0, gps0, sslot, tkf_gslot;
    std::vector<int> hv_ss0{0}, hv_sslot, hp_gslot;   // (after the regular tiles' slots of each target)
    int n_hslots = 0, n_gslots = 0, n_sslots = 0, n_gpslots = 0;
};
struct DevOrder {
    std::vector<double> camd, kst, lst, ep_data;
    std::vector<int> kf_cam, ep_kf, pri_a, pri_b;
};
struct Fingerprint {
    uint32_t hash = 0;
    int n_tiles = 0;
    int32_t shapes[LBA_TILE_SHAPES] = {};
};

// the extrinsic block an observation links (EdgeMonoGPExtrinsic's vertex 3), or -1
inline int ext_block(const lba_obs& o, const int* cam_slot, const int* kf_hidx) {
    return o.kind == LBA_MONO_GP && cam_slot[o.cam] >= 0 ? kf_hidx[cam_slot[o.cam]] : -1;
}

// ---- stage 1: the window's checks.  The first invalid observation (pieces in parallel; the serial pass below names
// it).  The same pass counts each piece's observations per landmark (the counting sort into observations by
// landmark, number_vertices) and marks the keyframes the piece touches (activity): the caller's 64-byte records
// are read once for the three
inline Checks validate_window(const Window& W, bool partitioned, SetupScratch& scr) {
    const lba_kf* kfs = W.kfs;
    const lba_obs* obs = W.obs;
    const int n_kf = W.n_kf, n_lm = W.n_lm, n_obs = W.n_obs, n_cam = W.n_cam;
    constexpr int VP = SETUP_PIECES;
    Checks C;
    int first_bad = n_obs;
    const bool lm_hist = C.lm_hist = n_lm > 0 && (long long)n_lm * VP <= (8LL << 20);   // (else: the serial counting sort)
    std::vector<int>& lm_cnt = sized(scr.lm_cnt, lm_hist ? (size_t)VP * n_lm : 0);
    std::vector<char>& kf_mark = C.kf_mark;
    kf_mark.assign((size_t)VP * std::max(n_kf, 1), 0);
    {
        int bad_at[VP];
        par_for(VP, [&](int piece) {
            // (every parallel body of the set-up first copies the tables and counts its loop reads into locals:
            // through the captured references every int store may alias them, and they are reloaded per element)
            const lba_kf* const kfs = W.kfs;
            const lba_obs* const obs = W.obs;
            const int n_kf = W.n_kf, n_lm = W.n_lm, n_obs = W.n_obs, n_cam = W.n_cam;
            const Range r = piece_range(n_obs, piece, VP);
            bad_at[piece] = n_obs;
            int* hc = lm_hist ? lm_cnt.data() + (size_t)piece * n_lm : nullptr;
            if (hc) std::fill(hc, hc + n_lm, 0);
            char* km = kf_mark.data() + (size_t)piece * std::max(n_kf, 1);
            for (int i = r.lo; i < r.hi; ++i) {
                const lba_obs& o = obs[i];
                bool ok = o.kind >= LBA_MONO_GP && o.kind <= LBA_STEREO && o.kf_b >= 0 && o.kf_b < n_kf && o.lm >= 0 &&
                          o.lm < n_lm && o.cam >= 0 && o.cam < n_cam && o.cam <= 255;
                if (ok && (o.kind == LBA_MONO_GP || o.kind == LBA_STEREO_GP))
                    ok = o.kf_a >= 0 && o.kf_a < n_kf && o.kf_a != o.kf_b &&
                         std::fabs(kfs[o.kf_b].time - kfs[o.kf_a].time) > 1e-6;
                if (!ok) { bad_at[piece] = i; break; }
                if (hc) ++hc[o.lm];
                km[o.kf_b] = 1;
                if (is_gp(o.kind)) km[o.kf_a] = 1;
            }
        });
        for (int piece = 0; piece < VP; ++piece) first_bad = std::min(first_bad, bad_at[piece]);
    }
    for (int i = first_bad; i < n_obs; ++i) {
        const lba_obs& o = obs[i];
        if (o.kind < LBA_MONO_GP || o.kind > LBA_STEREO) throw ApiError{LBA_E_ARG, "obs " + std::to_string(i) + ": bad kind"};
        if (o.kf_b < 0 || o.kf_b >= n_kf || o.lm < 0 || o.lm >= n_lm || o.cam < 0 || o.cam >= n_cam || o.cam > 255)
            throw ApiError{LBA_E_ARG, "obs " + std::to_string(i) + ": index out of range"};
        if (is_gp(o.kind)) {
            if (o.kf_a < 0 || o.kf_a >= n_kf || o.kf_a == o.kf_b)
                throw ApiError{LBA_E_ARG, "obs " + std::to_string(i) + ": bad kf_a"};
            if (!(std::fabs(kfs[o.kf_b].time - kfs[o.kf_a].time) > 1e-6))   // QiInv assert (GaussianProcess.h:32)
                throw ApiError{LBA_E_ARG, "obs " + std::to_string(i) + ": keyframe times too close"};
        }
    }
    for (int i = 0; i < W.n_priors; ++i) {
        const lba_prior& e = W.priors[i];
        if (e.kf_a < 0 || e.kf_a >= n_kf || e.kf_b < 0 || e.kf_b >= n_kf || e.kf_a == e.kf_b)
            throw ApiError{LBA_E_ARG, "prior " + std::to_string(i) + ": bad vertex"};
        if (!(std::fabs(kfs[e.kf_b].time - kfs[e.kf_a].time) > 1e-6))
            throw ApiError{LBA_E_ARG, "prior " + std::to_string(i) + ": keyframe times too close"};
    }
    for (int i = 0; i < W.n_vel; ++i)
        if (W.vel_kfs[i] < 0 || W.vel_kfs[i] >= n_kf) throw ApiError{LBA_E_ARG, "velocity edge: bad vertex"};
    for (int c = 0; c < n_cam; ++c)
        if (W.cams[c].ext_free) C.ext_cams.push_back(c);
    if (!C.ext_cams.empty()) {
        if (partitioned) throw ApiError{LBA_E_LIMIT, "free extrinsics are not supported in a partitioned problem"};
        for (int i = 0; i < n_obs; ++i)   // EdgeStereoGP projects through the static MultiKeyFrame::mTbc
            if (obs[i].kind == LBA_STEREO_GP && W.cams[obs[i].cam].ext_free)
                throw ApiError{LBA_E_ARG, "obs " + std::to_string(i) + ": stereo GP observation of a camera with a free extrinsic"};
    }
    return C;
}

// ---- stage 2: active vertices (SparseOptimizer::initializeOptimization: a vertex is active if an edge
//      that is not all-fixed touches it, sparse_optimizer.cpp:197-267), observations by original landmark and the
//      pose-block numbering
inline Vertices number_vertices(const Window& W, const Checks& C, bool partitioned, SetupScratch& scr, StageWork& wk) {
    const lba_kf* kfs = W.kfs;
    const lba_obs* obs = W.obs;
    const int n_kf = W.n_kf, n_lm = W.n_lm, n_obs = W.n_obs, n_cam = W.n_cam;
    constexpr int VP = SETUP_PIECES;
    Vertices V;
    std::vector<char>& kf_act = wk.kf_act;
    kf_act.assign(n_kf, 0);
    std::vector<char>& lm_act = V.lm_act;
    lm_act.assign(n_lm, 0);
    for (int piece = 0; piece < VP; ++piece)
        for (int k = 0; k < n_kf; ++k) kf_act[k] |= C.kf_mark[(size_t)piece * std::max(n_kf, 1) + k];
    // observations by original landmark (stable): a counting sort, the counts from the validation pass
    std::vector<int>& lo0 = V.lo0;
    lo0.assign(n_lm + 1, 0);
    std::vector<int>& lo_of = sized(scr.lo_of, n_obs);
    if (C.lm_hist) {
        std::vector<int>& lm_cnt = scr.lm_cnt;
        par_for(VP, [&](int piece) {   // per landmark: its total, and every piece's offset (its earlier pieces' counts)
            const int nlm = n_lm;
            int* const cnt = lm_cnt.data();
            int* const lz = lo0.data();
            const Range r = piece_range(nlm, piece, VP);
            for (int l = r.lo; l < r.hi; ++l) {
                int run = 0;
                for (int q = 0; q < VP; ++q) {
                    int& c = cnt[(size_t)q * nlm + l];
                    const int v = c;
                    c = run;
                    run += v;
                }
                lz[l + 1] = run;
            }
        });
        for (int l = 0; l < n_lm; ++l) lo0[l + 1] += lo0[l];
        par_for(VP, [&](int piece) {
            int* const off = lm_cnt.data() + (size_t)piece * n_lm;
            const lba_obs* const ob = obs;
            const int* const lz = lo0.data();
            int* const lo = lo_of.data();
            const Range r = piece_range(n_obs, piece, VP);
            for (int i = r.lo; i < r.hi; ++i) {
                const int l = ob[i].lm;
                lo[lz[l] + off[l]++] = i;
            }
        });
    } else {
        for (int i = 0; i < n_obs; ++i) lo0[obs[i].lm + 1]++;
        for (int l = 0; l < n_lm; ++l) lo0[l + 1] += lo0[l];
        std::vector<int> fill(lo0.begin(), lo0.end() - 1);
        for (int i = 0; i < n_obs; ++i) lo_of[fill[obs[i].lm]++] = i;
    }
    for (int l = 0; l < n_lm; ++l) lm_act[l] = lo0[l + 1] > lo0[l];
    for (int i = 0; i < W.n_priors; ++i)
        if (!(kfs[W.priors[i].kf_a].fixed && kfs[W.priors[i].kf_b].fixed)) {
            V.pri.push_back(W.priors[i]);
            kf_act[W.priors[i].kf_a] = kf_act[W.priors[i].kf_b] = 1;
        }
    for (int i = 0; i < W.n_vel; ++i)
        if (!kfs[W.vel_kfs[i]].fixed) {
            V.vel.push_back(W.vel_kfs[i]);
            kf_act[W.vel_kfs[i]] = 1;
        }
    // partitioned: every rank carries every non-fixed keyframe (activity is the union over the ranks'
    // edges; the caller's global graph connects them all through the motion priors on rank 0)
    if (partitioned)
        for (int k = 0; k < n_kf; ++k)
            if (!kfs[k].fixed) kf_act[k] = 1;
    // free extrinsics (always active: their EdgeExtrinsicPrior is not all-fixed) as KF slots after the
    // keyframes, pose blocks after the keyframes' (g2o orders the active vertices by id)
    const int n_ext = V.n_ext = (int)C.ext_cams.size(), n_kfs = V.n_kfs = n_kf + n_ext;
    V.cam_slot.assign(n_cam, -1);
    V.kf_hidx.assign(n_kfs, -1);
    int n_pb = 0;
    for (int k = 0; k < n_kf; ++k)
        if (kf_act[k] && !kfs[k].fixed) V.kf_hidx[k] = n_pb++;
    const int n_pb_kf = V.n_pb_kf = n_pb;
    for (int e = 0; e < n_ext; ++e) {
        V.cam_slot[C.ext_cams[e]] = n_kf + e;
        V.kf_hidx[n_kf + e] = n_pb++;
    }
    V.n_pb = n_pb;
    V.np = 12 * n_pb;
    V.np_ext = 12 * n_pb_kf + 6 * n_ext;
    V.pose_ext.assign(V.np, -1);
    for (int i = 0; i < V.np; ++i)
        if (i < 12 * n_pb_kf) V.pose_ext[i] = i;
        else if (i % 12 < 6) V.pose_ext[i] = 12 * n_pb_kf + 6 * ((i - 12 * n_pb_kf) / 12) + i % 12;
    return V;
}

// ---- stage 3: GP pairs, GP pose samples and every observation's pose sample (scr.smp_of)
inline GpSamples number_gp(const Window& W, const Vertices& V, SetupClock& clock, SetupScratch& scr, StageWork& wk) {
    const lba_obs* obs = W.obs;
    const int n_kf = W.n_kf, n_obs = W.n_obs;
    constexpr int VP = SETUP_PIECES;
    GpSamples G;
    // GP (prev KF, KF) pairs, numbered in order of first appearance; gp_of: each GP observation's pair
    // (per KF b a short list of its pairs: (KF a, pair index); usually one, the previous keyframe)
    // (in parallel: every piece lists its distinct pairs in first-appearance order; the pieces' lists, merged in
    // piece order, give the pairs in first appearance over all observations; then every GP observation's pair)
    std::vector<std::vector<std::pair<int, int>>>& gp_by_b = wk.gp_by_b;
    gp_by_b.assign(n_kf, {});
    std::vector<int>&gp_a = G.gp_a, &gp_b = G.gp_b;
    std::vector<int>& gp_of = sized(scr.gp_of, n_obs);   // (written and read for GP observations only)
    {
        std::vector<std::vector<std::pair<int, int>>> first(VP);   // per piece: (kf_a, kf_b) in first-appearance order
        par_for(VP, [&](int piece) {
            std::vector<std::vector<int>> seen_a(n_kf);   // per KF b: the KFs a this piece has listed
            auto& out = first[piece];
            const lba_obs* const ob = obs;
            const Range r = piece_range(n_obs, piece, VP);
            for (int i = r.lo; i < r.hi; ++i) {
                const lba_obs& o = ob[i];
                if (!is_gp(o.kind)) continue;
                std::vector<int>& sa = seen_a[o.kf_b];
                if (std::find(sa.begin(), sa.end(), o.kf_a) != sa.end()) continue;
                sa.push_back(o.kf_a);
                out.emplace_back(o.kf_a, o.kf_b);
            }
        });
        for (int piece = 0; piece < VP; ++piece)
            for (const auto& ab : first[piece]) {
                auto& lst = gp_by_b[ab.second];
                bool have = false;
                for (const auto& e : lst)
                    if (e.first == ab.first) { have = true; break; }
                if (have) continue;
                lst.emplace_back(ab.first, (int)gp_a.size());
                gp_a.push_back(ab.first);
                gp_b.push_back(ab.second);
            }
        par_for(VP, [&](int piece) {
            const lba_obs* const ob = obs;
            const std::vector<std::pair<int, int>>* const by_b = gp_by_b.data();
            int* const gof = gp_of.data();
            const Range r = piece_range(n_obs, piece, VP);
            for (int i = r.lo; i < r.hi; ++i) {
                const lba_obs& o = ob[i];
                if (!is_gp(o.kind)) continue;
                for (const auto& e : by_b[o.kf_b])
                    if (e.first == o.kf_a) { gof[i] = e.second; break; }
            }
        });
    }
    clock.sub("  GP pair numbering");

    // GP pose samples: distinct observation times per GP pair (one per camera time stamp in
    // LocalGPBA), contiguous per pair; observations of a camera with a free extrinsic get samples of
    // their own (key: time, camera), so a sample couples at most one extrinsic block
    std::vector<int>&gp_s0 = G.gp_s0, &gps_cam = G.gps_cam;
    std::vector<double>& gps_t = G.gps_t;
    gp_s0.assign(gp_a.size() + 1, 0);
    std::vector<int>& sample_of = sized(scr.sample_of, n_obs);   // (GP observations only, as gp_of)
    {
        typedef std::pair<double, int> SKey;
        auto skey = [](const lba_obs& o, const int* cslot, const int* H) {
            return SKey(o.t, ext_block(o, cslot, H) >= 0 ? o.cam : -1);
        };
        // distinct keys per pair are few: each of the observation pieces keeps up to KC distinct keys per pair
        // inline (flat arrays), more in a per-piece overflow list; then per pair the union, sorted
        const int ng = (int)gp_a.size();
        constexpr int KC = 16, NPC = SETUP_PIECES;
        std::vector<SKey> pk((size_t)NPC * std::max(ng, 1) * KC);
        std::vector<int> pc((size_t)NPC * std::max(ng, 1), 0);
        std::vector<std::vector<std::pair<int, SKey>>> pov(NPC);
        par_for(NPC, [&](int piece) {
            SKey* K = pk.data() + (size_t)piece * ng * KC;
            int* C = pc.data() + (size_t)piece * ng;
            const lba_obs* const ob = obs;
            const int *const gof = gp_of.data(), *const cslot = V.cam_slot.data(), *const H = V.kf_hidx.data();
            const Range r = piece_range(n_obs, piece, NPC);
            for (int i = r.lo; i < r.hi; ++i)
                if (is_gp(ob[i].kind)) {
                    const int g = gof[i];
                    const SKey k = skey(ob[i], cslot, H);
                    SKey* v = K + (size_t)g * KC;
                    bool seen = false;
                    for (int c = 0; c < C[g]; ++c)
                        if (v[c] == k) { seen = true; break; }
                    if (seen) continue;
                    if (C[g] < KC) v[C[g]++] = k;
                    else pov[piece].emplace_back(g, k);
                }
        });
        std::vector<std::vector<SKey>> ts(ng);
        for (int piece = 0; piece < NPC; ++piece) {
            const SKey* K = pk.data() + (size_t)piece * ng * KC;
            const int* C = pc.data() + (size_t)piece * ng;
            for (int g = 0; g < ng; ++g) ts[g].insert(ts[g].end(), K + (size_t)g * KC, K + (size_t)g * KC + C[g]);
            for (const auto& e : pov[piece]) ts[e.first].push_back(e.second);
        }
        clock.sub("  GP sample keys");
        std::vector<SKey> keys;
        for (size_t g = 0; g < ts.size(); ++g) {
            std::sort(ts[g].begin(), ts[g].end());
            ts[g].erase(std::unique(ts[g].begin(), ts[g].end()), ts[g].end());
            gp_s0[g + 1] = gp_s0[g] + (int)ts[g].size();
            for (const SKey& k : ts[g]) { gps_t.push_back(k.first); gps_cam.push_back(k.second); keys.push_back(k); }
        }
        clock.sub("  GP sample sort");
        par_for(SETUP_PIECES, [&](int piece) {
            const lba_obs* const ob = obs;
            const int *const gof = gp_of.data(), *const s0 = gp_s0.data(), *const cslot = V.cam_slot.data(),
                      *const H = V.kf_hidx.data();
            const SKey* const ky = keys.data();
            int* const sof = sample_of.data();
            const Range r = piece_range(n_obs, piece, SETUP_PIECES);
            for (int i = r.lo; i < r.hi; ++i)
                if (is_gp(ob[i].kind)) {
                    const int g = gof[i];
                    const SKey* b = ky + s0[g];
                    sof[i] = s0[g] + (int)(std::lower_bound(b, b + (s0[g + 1] - s0[g]), skey(ob[i], cslot, H)) - b);
                }
        });
    }

    clock.sub("GP pairs + samples");
    // pose sample of every observation: its GP sample, or the KF pose record n_gps + kf_b
    const int n_gps = G.n_gps = (int)gps_t.size();
    G.n_smp = n_gps + V.n_kfs;
    std::vector<int>& smp_of = sized(scr.smp_of, n_obs);
    par_for(VP, [&](int piece) {
        const lba_obs* const ob = obs;
        const int* const sof = sample_of.data();
        int* const so = smp_of.data();
        const int ngps = n_gps;
        const Range r = piece_range(n_obs, piece, VP);
        for (int i = r.lo; i < r.hi; ++i) so[i] = is_gp(ob[i].kind) ? sof[i] : ngps + ob[i].kf_b;
    });
    return G;
}

// ---- stage 4: heavy landmarks: a landmark whose observations / keyframes exceed one tile of k_lin_schur (a
//      long track: LocalGPBA adds every observation of a local point, up to every keyframe of the
//      window plus GP observations from non-keyframes, src/Optimizer.cc:1050-1200) is linearised in
//      segment tiles and merged / eliminated by k_expand (heavy_item); heavy landmarks go last in
//      device order.  Then the landmark order, the observations (scr.obs_of) and the (KF, landmark) pairs by
//      device landmark
inline LmOrder order_landmarks(const Window& W, const Vertices& V, const GpSamples& G, SetupClock& clock,
                               SetupScratch& scr, StageWork& wk) {
    const lba_obs* obs = W.obs;
    const int n_lm = W.n_lm, n_obs = W.n_obs, n_pb = V.n_pb, n_gps = G.n_gps, n_kfs = V.n_kfs;
    const std::vector<int>&H = V.kf_hidx, &lo0 = V.lo0, &lo_of = scr.lo_of, &smp_of = scr.smp_of;
    const std::vector<char>& lm_act = V.lm_act;
    LmOrder L;
    // per landmark: the span of non-fixed KFs observing it (device order key), heavy or not
    std::vector<int>&lmin = wk.lmin, &lmax = wk.lmax, &lm_npl = wk.lm_npl;
    std::vector<char>& heavy = wk.heavy;
    lmin.assign(n_lm, INT_MAX);
    lmax.assign(n_lm, INT_MAX);
    lm_npl.assign(n_lm, 0);
    heavy.assign(n_lm, 0);
    par_for(SETUP_PIECES, [&](int piece) {
        // distinct pose blocks / samples of a landmark counted by stamping (stamp = landmark + 1)
        std::vector<int> kst_((size_t)std::max(n_pb, 1), 0), sst_((size_t)std::max(n_gps + n_kfs, 1), 0);
        // (plain pointers and per-landmark locals: through the vectors every int store could alias every int
        // load, and the compiler reloaded the tables per observation)
        int* __restrict__ kst = kst_.data();
        int* __restrict__ sst = sst_.data();
        const int* __restrict__ Hh = H.data();
        const int* __restrict__ lo = lo_of.data();
        const int* __restrict__ lz = lo0.data();
        const int* __restrict__ so = smp_of.data();
        const int* __restrict__ cslot = V.cam_slot.data();
        const Range r = piece_range(n_lm, piece, SETUP_PIECES);
        for (int l = r.lo; l < r.hi; ++l) {
            if (!lm_act[l]) continue;
            int nr = 0, ne = 0, npl = 0, ns = 0, mn = INT_MAX, mx = INT_MAX;
            const int stamp = l + 1;
            for (int q = lz[l]; q < lz[l + 1]; ++q) {
                const int oi = lo[q];
                const lba_obs& o = obs[oi];
                const int hb = Hh[o.kf_b], ha = is_gp(o.kind) ? Hh[o.kf_a] : -1;
                const int hx = (o.kind == LBA_MONO_GP && cslot[o.cam] >= 0) ? Hh[cslot[o.cam]] : -1;   // ext_block(o)
                for (int k : {hb, ha})
                    if (k >= 0) {
                        mn = mn == INT_MAX ? k : std::min(mn, k);
                        mx = mx == INT_MAX ? k : std::max(mx, k);
                    }
                for (int k : {hb, ha, hx})
                    if (k >= 0 && kst[k] != stamp) { kst[k] = stamp; ++npl; }
                ne += (hb >= 0) + (ha >= 0) + (hx >= 0);
                nr += obs_dim(o.kind);
                const int sm = so[oi];
                if (sst[sm] != stamp) { sst[sm] = stamp; ++ns; }
            }
            lmin[l] = mn;
            lmax[l] = mx;
            heavy[l] = !tile_fits(lz[l + 1] - lz[l], nr, npl, 1, npl, ns, ne);
            lm_npl[l] = npl;   // (its distinct pose blocks: its (KF, landmark) pairs below)
        }
    });
    clock.sub("heavy classification");
    std::vector<int>& order = L.order;
    int n_heavy_lm = 0;
    {   // stable order by (heavy, lmin, lmax) (INT_MAX = observed by fixed KFs only, after every block):
        // three stable counting passes (lmax, lmin, heavy) over the active landmarks in index order
        auto key = [&](int v) { return v == INT_MAX ? n_pb : v; };
        std::vector<int> a, b;
        a.reserve(n_lm);
        for (int l = 0; l < n_lm; ++l)
            if (lm_act[l]) { a.push_back(l); n_heavy_lm += heavy[l]; }
        b.resize(a.size());
        std::vector<int> cnt((size_t)std::max(n_pb + 2, 3));
        auto pass = [&](auto kf, int nk) {
            std::fill(cnt.begin(), cnt.begin() + nk + 1, 0);
            for (int l : a) cnt[kf(l) + 1]++;
            for (int k = 0; k < nk; ++k) cnt[k + 1] += cnt[k];
            for (int l : a) b[cnt[kf(l)]++] = l;
            a.swap(b);
        };
        pass([&](int l) { return key(lmax[l]); }, n_pb + 1);
        pass([&](int l) { return key(lmin[l]); }, n_pb + 1);
        pass([&](int l) { return (int)heavy[l]; }, 2);
        order.swap(a);
    }
    const int nl = L.nl = (int)order.size();
    L.n_reg = nl - n_heavy_lm;

    clock.sub("landmark order");
    // observations grouped by device landmark (stable)
    std::vector<int>& lobs0 = L.lobs0;
    lobs0.assign(nl + 1, 0);
    std::vector<int>& obs_of = sized(scr.obs_of, n_obs);
    for (int d = 0; d < nl; ++d) lobs0[d + 1] = lobs0[d] + (lo0[order[d] + 1] - lo0[order[d]]);
    par_for(SETUP_PIECES, [&](int piece) {
        const int *const ord = order.data(), *const lo = lo_of.data(), *const lz = lo0.data(), *const lb = lobs0.data();
        int* const oo = obs_of.data();
        const Range r = piece_range(nl, piece, SETUP_PIECES);
        for (int d = r.lo; d < r.hi; ++d) {
            const int l = ord[d];
            std::copy(lo + lz[l], lo + lz[l + 1], oo + lb[d]);
        }
    });

    clock.sub("obs by landmark");
    // (KF, landmark) pairs, per device landmark, ascending pose block
    std::vector<int>&lm_pair0 = L.lm_pair0, &pair_lm = L.pair_lm, &pair_kf = L.pair_kf;
    lm_pair0.assign(nl + 1, 0);
    // the pose blocks of the landmark with observations oo[q0 .. q1), ascending, distinct
    auto lm_blocks = [](const lba_obs* ob, const int* oo, int q0, int q1, const int* Hh, const int* cslot,
                        std::vector<int>& ks) {
        ks.clear();
        for (int q = q0; q < q1; ++q) {
            const lba_obs& o = ob[oo[q]];
            if (Hh[o.kf_b] >= 0) ks.push_back(Hh[o.kf_b]);
            if (is_gp(o.kind) && Hh[o.kf_a] >= 0) ks.push_back(Hh[o.kf_a]);
            if (ext_block(o, cslot, Hh) >= 0) ks.push_back(ext_block(o, cslot, Hh));
        }
        std::sort(ks.begin(), ks.end());
        ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
    };
    // counts (the distinct pose blocks the heavy classification counted), then the pairs themselves
    for (int d = 0; d < nl; ++d) lm_pair0[d + 1] = lm_pair0[d] + lm_npl[order[d]];
    const int n_pairs = L.n_pairs = lm_pair0[nl];
    pair_lm.resize(n_pairs);
    pair_kf.resize(n_pairs);
    par_for(SETUP_PIECES, [&](int piece) {
        std::vector<int> ks;
        const lba_obs* const ob = obs;
        const int *const oo = obs_of.data(), *const lb = lobs0.data(), *const lp0 = lm_pair0.data(), *const Hh = H.data(),
                  *const cslot = V.cam_slot.data();
        int *const plm = pair_lm.data(), *const pkf = pair_kf.data();
        const Range r = piece_range(nl, piece, SETUP_PIECES);
        for (int d = r.lo; d < r.hi; ++d) {
            lm_blocks(ob, oo, lb[d], lb[d + 1], Hh, cslot, ks);
            for (size_t i = 0; i < ks.size(); ++i) { plm[lp0[d] + i] = d; pkf[lp0[d] + i] = ks[i]; }
        }
    });
    return L;
}

// original landmark -> device index (-1 inactive), into the caller's array
inline void lm_dev_of(const LmOrder& L, int n_lm, std::vector<int>& lm_dev) {
    lm_dev.assign(n_lm, -1);
    for (int d = 0; d < L.nl; ++d) lm_dev[L.order[d]] = d;
}

// ---- stage 5: tiles: consecutive regular landmarks under the limits of one k_lin_schur workgroup (tile_fits),
//      then the segment tiles of the heavy landmarks.
// Regular tiles: the landmarks [0, n_reg) in SETUP_PIECES contiguous pieces, each cut greedily into tiles
// on its own thread (tiles never straddle a piece boundary, so the tiling is the same for any thread
// count).  The tiles' lists depend only on their own landmarks: they are built in a second pass, in
// parallel over runs of consecutive tiles, and concatenated with their offsets.  (A window below 256
// landmarks per piece is one piece: its cut is serial, its lists -- most of the work -- are not.)

// what the tiling reads per observation, in device order (scr.dhb .. scr.dsmp)
inline void tile_inputs(const Window& W, const Vertices& V, SetupScratch& scr) {
    const lba_obs* obs = W.obs;
    const int n_obs = W.n_obs;
    const std::vector<int>&H = V.kf_hidx, &obs_of = scr.obs_of, &smp_of = scr.smp_of;
    std::vector<int>&dhb = sized(scr.dhb, n_obs), &dha = sized(scr.dha, n_obs), &dhx = sized(scr.dhx, n_obs),
                     &ddim = sized(scr.ddim, n_obs), &dsmp = sized(scr.dsmp, n_obs);
    par_for(SETUP_PIECES, [&](int piece) {
        const lba_obs* const obsv = obs;
        const int *const Hh = H.data(), *const cslot = V.cam_slot.data(), *const oo = obs_of.data(), *const so = smp_of.data();
        int *const hb = dhb.data(), *const ha = dha.data(), *const hx = dhx.data(), *const dd = ddim.data(),
            *const ds = dsmp.data();
        const Range r = piece_range(n_obs, piece, SETUP_PIECES);
        for (int q = r.lo; q < r.hi; ++q) {
            const lba_obs& ob = obsv[oo[q]];
            hb[q] = Hh[ob.kf_b];
            ha[q] = is_gp(ob.kind) ? Hh[ob.kf_a] : -1;
            hx[q] = ext_block(ob, cslot, Hh);
            dd[q] = obs_dim(ob.kind);
            ds[q] = so[oo[q]];
        }
    });
}

#ifndef LBA_TILE_OBS_CAP
#define LBA_TILE_OBS_CAP TILE_OBS
#endif

// pass 1, the cut: tile t holds the regular landmarks [tl_d[t], tl_d[t + 1])
inline std::vector<int> cut_tiles(const LmOrder& L, int n_pb, int n_smp, const SetupScratch& scr) {
    const int n_reg = L.n_reg;
    const int n_pieces = n_reg >= 256 * SETUP_PIECES ? SETUP_PIECES : 1;
    const int obs_cap = LBA_TILE_OBS_CAP;   // (a smaller cap: A/B builds only, scripts/exp_build.sh)
    std::vector<std::vector<int>> cut(n_pieces);   // the first landmark of every tile, per piece
    par_for(n_pieces, [&](int piece) {
        const int* lobs0 = L.lobs0.data();
        const int* lm_pair0 = L.lm_pair0.data();
        const int* pair_kf = L.pair_kf.data();
        const int *dhb = scr.dhb.data(), *dha = scr.dha.data(), *dhx = scr.dhx.data(), *ddim = scr.ddim.data(),
                  *dsmp = scr.dsmp.data();
        const int cap = obs_cap;
        const Range r = piece_range(n_reg, piece, n_pieces);
        const int d_end = r.hi;
        int d = r.lo;
        // the tile's sample / KF sets grow by the landmark's new elements, found through membership
        // marks (1: in the tile, 2: new for the landmark being tried)
        std::vector<int> uni, usm, new_s, new_k;
        std::vector<char> kmark((size_t)std::max(n_pb, 1), 0), smark((size_t)std::max(n_smp, 1), 0);
        uni.reserve(TILE_PAIRS + 8);
        usm.reserve(TILE_SMP + 8);
        while (d < d_end) {
            int nobs = 0, rows = 0, npair = 0, nlmt = 0, nent = 0;
            uni.clear();
            usm.clear();
            int e = d;
            while (e < d_end) {
                int no = lobs0[e + 1] - lobs0[e], nr = 0, ne = 0;
                new_s.clear();
                new_k.clear();
                for (int q = lobs0[e]; q < lobs0[e + 1]; ++q) {
                    nr += ddim[q];
                    if (!smark[dsmp[q]]) { smark[dsmp[q]] = 2; new_s.push_back(dsmp[q]); }
                    ne += (dhb[q] >= 0) + (dha[q] >= 0) + (dhx[q] >= 0);
                }
                for (int q = lm_pair0[e]; q < lm_pair0[e + 1]; ++q) {   // the landmark's pose blocks
                    const int k = pair_kf[q];
                    if (!kmark[k]) { kmark[k] = 2; new_k.push_back(k); }
                }
                const int npl = lm_pair0[e + 1] - lm_pair0[e];
                const bool fits = tile_fits(nobs + no, rows + nr, npair + npl, nlmt + 1,
                                            (int)(uni.size() + new_k.size()), (int)(usm.size() + new_s.size()),
                                            nent + ne) &&
                                  (nlmt == 0 || nobs + no <= cap);
                for (int v : new_s) smark[v] = fits ? 1 : 0;
                for (int k : new_k) kmark[k] = fits ? 1 : 0;
                if (!fits) {
                    if (e == d)   // (the heavy classification takes every landmark a tile cannot hold)
                        throw ApiError{LBA_E_LIMIT, "internal: landmark " + std::to_string(L.order[e]) + " does not fit a tile"};
                    break;
                }
                nobs += no; rows += nr; npair += npl; nlmt += 1; nent += ne;
                usm.insert(usm.end(), new_s.begin(), new_s.end());
                uni.insert(uni.end(), new_k.begin(), new_k.end());
                ++e;
            }
            for (int v : usm) smark[v] = 0;
            for (int k : uni) kmark[k] = 0;
            cut[piece].push_back(d);
            d = e;
        }
    });
    std::vector<int> tl_d;
    for (const auto& c : cut) tl_d.insert(tl_d.end(), c.begin(), c.end());
    tl_d.push_back(n_reg);
    return tl_d;
}

// pass 2, the lists: runs of consecutive tiles, each into its own TileLists; a run also writes its landmarks' part
// of scr.ob_row, scr.pair_lk and (run-local offsets until concat_runs) scr.pair_r0 / scr.lm_r0
inline std::vector<TileLists> tile_run_lists(const LmOrder& L, int n_pb, int n_smp, const std::vector<int>& tl_d,
                                             SetupScratch& scr, Tiles& T) {
    const int n_rt = (int)tl_d.size() - 1, n_runs = std::min(SETUP_PIECES, n_rt);
    std::vector<TileLists> outs(n_runs);
    par_for(n_runs, [&](int run) {
        TileLists& O = outs[run];
        const int* lobs0 = L.lobs0.data();
        const int* lm_pair0 = L.lm_pair0.data();
        const int* pair_kf = L.pair_kf.data();
        const int *dhb = scr.dhb.data(), *dha = scr.dha.data(), *dhx = scr.dhx.data(), *ddim = scr.ddim.data(),
                  *dsmp = scr.dsmp.data();
        int *ob_row = scr.ob_row.data(), *pair_r0 = scr.pair_r0.data(), *lm_r0 = scr.lm_r0.data(), *pair_lk = scr.pair_lk.data();
        auto lm_kfs = [&](int l) { return Span{pair_kf + lm_pair0[l], (size_t)(lm_pair0[l + 1] - lm_pair0[l])}; };
        const Range tr = piece_range(n_rt, run, n_runs);
        const int ta = tr.lo, tb = tr.hi;
        std::vector<int> uni, usm;
        std::vector<char> kmark((size_t)std::max(n_pb, 1), 0), smark((size_t)std::max(n_smp, 1), 0);
        std::vector<int> sloc_v((size_t)std::max(n_smp, 1), 0);   // sample -> its rank in the tile
        int* sloc = sloc_v.data();
        int srows[TILE_SMP + 1];
        uni.reserve(TILE_PAIRS + 8);
        usm.reserve(TILE_SMP + 8);
        {   // capacity for the run's share of the outputs (no regrowth while building)
            const int la = tl_d[ta], lb = tl_d[tb];
            const int no_p = lobs0[lb] - lobs0[la], np_p = lm_pair0[lb] - lm_pair0[la];
            const int nt_est = tb - ta + 1;
            O.pair_rows.reserve((size_t)np_p * 4 + 16);
            O.lm_rows.reserve((size_t)no_p * 3 + 16);
            O.tsm_smp.reserve((size_t)nt_est * TILE_SMP / 2);
            O.tsm_rows.reserve((size_t)nt_est * TILE_SMP / 2);
            O.sent_l1.reserve((size_t)nt_est * 48); O.sent_l2.reserve((size_t)nt_est * 48);
            O.sent_k1.reserve((size_t)nt_est * 48); O.sent_k2.reserve((size_t)nt_est * 48);
            O.tkf_list.reserve((size_t)nt_est * TILE_KF);
        }
        for (int t = ta; t < tb; ++t) {
            const int d = tl_d[t], e = tl_d[t + 1];
            const int nobs = lobs0[e] - lobs0[d], npair = lm_pair0[e] - lm_pair0[d], nlmt = e - d;
            // the tile's pose blocks (uni) and pose samples (usm), sorted
            uni.clear();
            usm.clear();
            for (int l = d; l < e; ++l) {
                for (int q = lobs0[l]; q < lobs0[l + 1]; ++q)
                    if (!smark[dsmp[q]]) { smark[dsmp[q]] = 1; usm.push_back(dsmp[q]); }
                for (int k : lm_kfs(l))
                    if (!kmark[k]) { kmark[k] = 1; uni.push_back(k); }
            }
            for (int v : usm) smark[v] = 0;
            for (int k : uni) kmark[k] = 0;
            std::sort(uni.begin(), uni.end());
            std::sort(usm.begin(), usm.end());
            for (size_t i = 0; i < usm.size(); ++i) sloc[usm[i]] = (int)i;
            O.t_obs0.push_back(lobs0[d]); O.t_nobs.push_back(nobs);
            O.t_lm0.push_back(d); O.t_nlm.push_back(nlmt);
            O.t_pair0.push_back(lm_pair0[d]); O.t_npair.push_back(npair);
            O.t_kf0.push_back((int)O.tkf_list.size()); O.t_nkf.push_back((int)uni.size());
            for (int k : uni) O.tkf_list.push_back(k);
            auto local = [&](int k) { return (int)(std::lower_bound(uni.begin(), uni.end(), k) - uni.begin()); };
            // LDS rows grouped by pose sample: every sample of the tile owns one contiguous row run, the
            // samples ascending, observations ascending within a sample (a counting pass over the
            // tile's sorted sample list).  (Not segment_tiles' emit_rows: this one also writes the tile-local
            // sample into ob_row's bits 16 and up.)
            O.t_smp0.push_back((int)O.tsm_smp.size());
            {
                const int ns = (int)usm.size();
                std::fill(srows, srows + ns + 1, 0);
                for (int q = lobs0[d]; q < lobs0[e]; ++q) srows[sloc[dsmp[q]] + 1] += ddim[q];
                for (int i = 0; i < ns; ++i) srows[i + 1] += srows[i];
                for (int i = 0; i < ns; ++i) {
                    O.tsm_smp.push_back(usm[i]);
                    O.tsm_rows.push_back(srows[i] | ((srows[i + 1] - srows[i]) << 16));
                }
                for (int q = lobs0[d]; q < lobs0[e]; ++q) {
                    const int i = sloc[dsmp[q]];
                    ob_row[q] = srows[i] | (i << 16);   // (+ the tile-local sample: k_update's back-substitution)
                    srows[i] += ddim[q];
                }
            }
            O.t_nsmp.push_back((int)O.tsm_smp.size() - O.t_smp0.back());
            // entry lists per pair, row lists per landmark, the pairs' tile-local (KF, landmark);
            // pair_r0 / lm_r0 hold run-local offsets until the concatenation.  (The entry list is the one
            // segment_tiles emits per segment pair, there over the segment's observations with the segment's base.)
            for (int l = d; l < e; ++l) {
                for (int q = lm_pair0[l]; q < lm_pair0[l + 1]; ++q) {
                    const int k = pair_kf[q];
                    for (int o = lobs0[l]; o < lobs0[l + 1]; ++o) {
                        if (dhb[o] == k) O.pair_rows.push_back((o - lobs0[d]) | (1 << 16));
                        if (dha[o] == k) O.pair_rows.push_back(o - lobs0[d]);
                        if (dhx[o] == k) O.pair_rows.push_back((o - lobs0[d]) | (2 << 16));
                    }
                    pair_r0[q + 1] = (int)O.pair_rows.size();
                    pair_lk[q] = local(k) | ((l - d) << 8);
                }
                for (int o = lobs0[l]; o < lobs0[l + 1]; ++o)
                    for (int r = 0; r < ddim[o]; ++r) O.lm_rows.push_back((ob_row[o] & 0xffff) + r);
                lm_r0[l + 1] = (int)O.lm_rows.size();
            }
            // Schur entries: every (k1 <= k2) pose-block pair co-observed by a landmark of the tile, in
            // (k1, k2) order (k_lin_schur writes C's blocks of exactly these KF pairs)
            {
                bool co[TILE_KF][TILE_KF] = {};
                int lk[TILE_KF];
                for (int l = d; l < e; ++l) {
                    const Span ks = lm_kfs(l);
                    for (size_t a = 0; a < ks.size(); ++a) lk[a] = local(ks[a]);
                    for (size_t a = 0; a < ks.size(); ++a)
                        for (size_t b = a; b < ks.size(); ++b) co[lk[a]][lk[b]] = true;
                }
                const int nu = (int)uni.size();
                O.t_sent0.push_back((int)O.sent_l1.size());
                int nen = 0;
                // the diagonal entries (every tile KF has one) first: k_lin_schur gives them 6 tasks (their
                // strictly lower 6 x 6 corner is never assembled), the others 8
                for (int i = 0; i < nu; ++i) {
                    ++nen;
                    O.sent_l1.push_back(i); O.sent_l2.push_back(i);
                    O.sent_k1.push_back(uni[i]); O.sent_k2.push_back(uni[i]);
                }
                for (int i = 0; i < nu; ++i)
                    for (int j = i + 1; j < nu; ++j)
                        if (co[i][j]) {
                            ++nen;
                            O.sent_l1.push_back(i); O.sent_l2.push_back(j);
                            O.sent_k1.push_back(uni[i]); O.sent_k2.push_back(uni[j]);
                        }
                O.t_nsent.push_back(nen);
            }
        }
    });
    return outs;
}

// the runs' lists concatenated into T.l: every list's per-run offsets first, then the runs copied in parallel
// (a serial element-wise concatenation cost most of the tiling's wall time on 16 threads); scr.pair_r0 / scr.lm_r0
// become offsets into the concatenated pair_rows / lm_rows
inline void concat_runs(const std::vector<TileLists>& outs, const std::vector<int>& tl_d, const LmOrder& L,
                        SetupScratch& scr, Tiles& T) {
    const int n_runs = (int)outs.size(), n_rt = (int)tl_d.size() - 1;
    constexpr int NC = N_TILE_CATS;
    // off[c][run]: where the run's part of list c starts
    std::vector<std::vector<size_t>> off(NC, std::vector<size_t>(n_runs + 1, 0));
    for (int c = 0; c < NC; ++c) {
        for (int run = 0; run < n_runs; ++run) off[c][run + 1] = off[c][run] + (outs[run].*(TILE_CATS[c].list)).size();
        (T.l.*(TILE_CATS[c].list)).resize(off[c][n_runs]);
    }
    auto at = [&](std::vector<int> TileLists::*m) {   // index of a list in TILE_CATS
        for (int c = 0; c < NC; ++c)
            if (TILE_CATS[c].list == m) return c;
        return -1;
    };
    int c_base[NC];
    for (int c = 0; c < NC; ++c) c_base[c] = TILE_CATS[c].base ? at(TILE_CATS[c].base) : -1;
    const int c_pr = at(&TileLists::pair_rows), c_lr = at(&TileLists::lm_rows);
    par_for(n_runs, [&](int run) {
        const TileLists& O = outs[run];
        for (int c = 0; c < NC; ++c) {
            const std::vector<int>& src = O.*(TILE_CATS[c].list);
            const int a = c_base[c] >= 0 ? (int)off[c_base[c]][run] : 0;
            int* d = (T.l.*(TILE_CATS[c].list)).data() + off[c][run];
            for (size_t k = 0; k < src.size(); ++k) d[k] = src[k] + a;
        }
        const Range tr = piece_range(n_rt, run, n_runs);
        const int d0 = tl_d[tr.lo], d1 = tl_d[tr.hi];
        const int o_pr = (int)off[c_pr][run], o_lr = (int)off[c_lr][run];
        int *const pr0 = scr.pair_r0.data(), *const lr0 = scr.lm_r0.data();
        for (int q = L.lm_pair0[d0], q1 = L.lm_pair0[d1]; q < q1; ++q) pr0[q + 1] += o_pr;
        for (int l = d0; l < d1; ++l) lr0[l + 1] += o_lr;
    });
}

// the heavy landmarks' segment tiles, appended to T.l: runs of a heavy landmark's observations under the limits
// of k_lin_schur's phases 1-4 (no elimination: no KF-union limit; a segment's pairs are its distinct pose blocks)
inline void segment_tiles(const LmOrder& L, int n_pb, int n_smp, SetupScratch& scr, Tiles& T) {
    const std::vector<int>&lobs0 = L.lobs0, &lm_pair0 = L.lm_pair0, &pair_kf = L.pair_kf;
    const std::vector<int>&dhb = scr.dhb, &dha = scr.dha, &dhx = scr.dhx, &ddim = scr.ddim, &dsmp = scr.dsmp;
    const int nl = L.nl, n_reg = L.n_reg, n_pairs = L.n_pairs;
    TileLists& O = T.l;
    std::vector<int>&ob_row = scr.ob_row, &pair_r0 = scr.pair_r0, &lm_r0 = scr.lm_r0;
    std::vector<unsigned long long> tob;
    // LDS rows of a tile's observations [q0, q1) grouped by pose sample: every sample of the tile owns
    // one contiguous row run (stable by observation within a sample).  (By sorting; the regular tiles' counting
    // pass in tile_run_lists differs in what it puts into ob_row.)
    auto emit_rows = [&](int q0, int q1) {
        tob.clear();
        for (int q = q0; q < q1; ++q) tob.push_back(((unsigned long long)(unsigned)dsmp[q] << 32) | (unsigned)q);
        std::sort(tob.begin(), tob.end());
        O.t_smp0.push_back((int)O.tsm_smp.size());
        int row = 0;
        for (size_t i = 0; i < tob.size();) {
            const int sm = (int)(tob[i] >> 32), r0 = row;
            size_t j = i;
            for (; j < tob.size() && (int)(tob[j] >> 32) == sm; ++j) {
                const int q = (int)(tob[j] & 0xffffffffu);
                ob_row[q] = row;
                row += ddim[q];
            }
            O.tsm_smp.push_back(sm);
            O.tsm_rows.push_back(r0 | ((row - r0) << 16));
            i = j;
        }
        O.t_nsmp.push_back((int)O.tsm_smp.size() - O.t_smp0.back());
    };
    // entry list of the pair of KF block k over observations [q0, q1) (tile-local observation | side << 16)
    auto emit_pair_rows = [&](int k, int q0, int q1, int obase) {
        for (int o = q0; o < q1; ++o) {
            if (dhb[o] == k) O.pair_rows.push_back((o - obase) | (1 << 16));
            if (dha[o] == k) O.pair_rows.push_back(o - obase);
            if (dhx[o] == k) O.pair_rows.push_back((o - obase) | (2 << 16));
        }
    };
    // heavy landmarks: their canonical pairs and landmark slots get no rows of their own
    for (int q = lm_pair0[n_reg]; q < n_pairs; ++q) pair_r0[q + 1] = (int)O.pair_rows.size();
    for (int l = n_reg; l < nl; ++l) lm_r0[l + 1] = (int)O.lm_rows.size();
    std::vector<int> uni, usm;
    std::vector<char> kmark((size_t)std::max(n_pb, 1), 0), smark((size_t)std::max(n_smp, 1), 0);
    for (int l = n_reg; l < nl; ++l) {
        T.hv_lm.push_back(l);
        const int cp0 = lm_pair0[l], ncp = lm_pair0[l + 1] - cp0;
        std::vector<std::vector<int>> src(ncp);
        int q0 = lobs0[l];
        while (q0 < lobs0[l + 1]) {
            int q1 = q0, nr = 0, ne = 0;
            usm.clear();
            uni.clear();
            while (q1 < lobs0[l + 1]) {
                const int neq = (dhb[q1] >= 0) + (dha[q1] >= 0) + (dhx[q1] >= 0);
                const int ns = (int)usm.size() + !smark[dsmp[q1]];
                int nk = (int)uni.size();
                for (int k : {dhb[q1], dha[q1], dhx[q1]})
                    if (k >= 0 && !kmark[k]) { kmark[k] = 2; ++nk; }
                const bool fits = q1 - q0 + 1 <= TILE_OBS && nr + ddim[q1] <= TILE_ROWS && nk <= TILE_PAIRS &&
                                  ns <= TILE_SMP && ne + neq <= TILE_PROWS;
                for (int k : {dhb[q1], dha[q1], dhx[q1]})
                    if (k >= 0 && kmark[k] == 2) {
                        kmark[k] = fits ? 1 : 0;
                        if (fits) uni.push_back(k);
                    }
                if (!fits) break;
                if (!smark[dsmp[q1]]) { smark[dsmp[q1]] = 1; usm.push_back(dsmp[q1]); }
                nr += ddim[q1];
                ne += neq;
                ++q1;
            }
            for (int v : usm) smark[v] = 0;
            for (int k : uni) kmark[k] = 0;
            std::sort(uni.begin(), uni.end());
            const int s = T.n_seg++, sp0 = T.n_segpairs;
            O.t_obs0.push_back(q0); O.t_nobs.push_back(q1 - q0);
            O.t_lm0.push_back(nl + s); O.t_nlm.push_back(1);
            O.t_pair0.push_back(n_pairs + sp0); O.t_npair.push_back((int)uni.size());
            O.t_kf0.push_back((int)O.tkf_list.size()); O.t_nkf.push_back(0);
            O.t_sent0.push_back((int)O.sent_l1.size()); O.t_nsent.push_back(0);
            emit_rows(q0, q1);
            for (size_t c = 0; c < uni.size(); ++c) {
                emit_pair_rows(uni[c], q0, q1, q0);
                pair_r0.push_back((int)O.pair_rows.size());
                const int* kb = pair_kf.data() + cp0;
                src[std::lower_bound(kb, kb + ncp, uni[c]) - kb].push_back(n_pairs + sp0 + (int)c);
            }
            T.n_segpairs += (int)uni.size();
            for (int o = q0; o < q1; ++o)
                for (int r = 0; r < ddim[o]; ++r) O.lm_rows.push_back(ob_row[o] + r);
            lm_r0.push_back((int)O.lm_rows.size());
            q0 = q1;
        }
        T.hv_seg0.push_back(T.n_seg);
        for (int j = 0; j < ncp; ++j) {
            for (int v : src[j]) T.hp_src.push_back(v);
            T.hp_src0.push_back((int)T.hp_src.size());
        }
        T.hv_hp0.push_back(T.hv_hp0.back() + ncp);
    }
}

inline Tiles build_tiles(const Window& W, const Vertices& V, const GpSamples& G, const LmOrder& L, SetupClock& clock,
                         SetupScratch& scr) {
    Tiles T;
    // the tiles' observation- and pair-sized arrays live in the scratch and take no fill: every observation's row and
    // every regular pair's entry is written by its tile.  As fresh zero-filled vectors they were 1.5 MB of serial
    // stores per window into heap memory that the worker threads had written a moment before (number_gp's per-piece key
    // tables, just freed): 0.24 ms at config 1 (profiles/setup_stages_ab.txt)
    sized(scr.ob_row, W.n_obs);
    sized(scr.pair_r0, L.n_pairs + 1)[0] = 0;   // (every later element is written by its tile, or below for a heavy landmark)
    sized(scr.lm_r0, L.nl + 1)[0] = 0;
    sized(scr.pair_lk, std::max(L.n_pairs, 1));
    std::fill(scr.pair_lk.begin() + (L.n_pairs ? L.lm_pair0[L.n_reg] : 0), scr.pair_lk.end(), 0);
    tile_inputs(W, V, scr);
    clock.sub("tile inputs");
    const std::vector<int> tl_d = cut_tiles(L, V.n_pb, G.n_smp, scr);
    const std::vector<TileLists> runs = tile_run_lists(L, V.n_pb, G.n_smp, tl_d, scr, T);   // (freed after the segments)
    concat_runs(runs, tl_d, L, scr, T);
    T.n_stiles = T.n_tiles();
    clock.sub("regular tiles");
    segment_tiles(L, V.n_pb, G.n_smp, scr, T);
    return T;
}

inline std::vector<int> prefix_sums(const std::vector<int>& c) {   // exclusive
    std::vector<int> s(c.size(), 0);
    for (size_t i = 1; i < c.size(); ++i) s[i] = s[i - 1] + c[i - 1];
    return s;
}

// ---- stage 6: partial-sum slots, sorted by reduction target
inline Slots build_slots(const Window& W, const Vertices& V, const GpSamples& G, const LmOrder& L, const Tiles& T,
                         StageWork& wk) {
    const int n_kf = W.n_kf, n_ext = V.n_ext, n_pb = V.n_pb, n_smp = G.n_smp, n_gps = G.n_gps;
    const std::vector<int>& H = V.kf_hidx;
    const std::vector<int>&tsm_smp = T.l.tsm_smp, &tsm_rows = T.l.tsm_rows, &sent_k1 = T.l.sent_k1, &sent_k2 = T.l.sent_k2,
                    &tkf_list = T.l.tkf_list;
    const int n_sent = (int)T.l.sent_l1.size(), n_heavy = (int)T.hv_lm.size();
    Slots S;
    // (tile, sample) M / g partials: per sample, its tiles in tile order
    std::vector<int>& mcnt = wk.mcnt;
    mcnt.assign(n_smp + 1, 0);
    for (int sm : tsm_smp) mcnt[sm]++;
    S.ms0 = prefix_sums(mcnt);
    std::vector<int>& mfill = wk.mfill = S.ms0;
    S.tsm_meta.assign(2 * std::max(tsm_smp.size(), (size_t)1), 0);
    for (size_t i = 0; i < tsm_smp.size(); ++i) {
        S.tsm_meta[2 * i] = tsm_rows[i];
        S.tsm_meta[2 * i + 1] = mfill[tsm_smp[i]]++;
    }
    S.n_mslots = S.ms0[n_smp];
    // Hpp / b_p slab entries: pose samples (N^T M N: aa, ab, bb over their KFs a, b), then motion priors,
    // then velocity edges
    const int n_ublocks = S.n_ublocks = n_pb * (n_pb + 1) / 2;
    std::vector<int>&ub_i = S.ub_i, &ub_j = S.ub_j;
    ub_i.resize(n_ublocks);
    ub_j.resize(n_ublocks);
    for (int bi = 0; bi < n_pb; ++bi)
        for (int bj = bi; bj < n_pb; ++bj) {
            const int id = ublock_id(n_pb, bi, bj);
            ub_i[id] = bi; ub_j[id] = bj;
        }
    // (a sample of a camera with a free extrinsic also couples its block e: ae, be, ee, b_e; then the
    // extrinsic priors on their blocks as "b")
    std::vector<int>&ent_a = S.ent_a, &ent_b = S.ent_b, &ent_e = S.ent_e, &ent_cam = S.ent_cam;
    for (int sm = 0; sm < n_smp; ++sm) {
        ent_e.push_back(-1); ent_cam.push_back(-1);
        if (mcnt[sm] == 0) { ent_a.push_back(-1); ent_b.push_back(-1); continue; }   // unobserved
        if (sm < n_gps) {
            const int g = (int)(std::upper_bound(G.gp_s0.begin(), G.gp_s0.end(), sm) - G.gp_s0.begin()) - 1;
            ent_a.push_back(H[G.gp_a[g]]); ent_b.push_back(H[G.gp_b[g]]);
            if (G.gps_cam[sm] >= 0) { ent_e.back() = H[V.cam_slot[G.gps_cam[sm]]]; ent_cam.back() = G.gps_cam[sm]; }
        } else {
            ent_a.push_back(-1); ent_b.push_back(H[sm - n_gps]);
        }
    }
    for (auto& e : V.pri) { ent_a.push_back(H[e.kf_a]); ent_b.push_back(H[e.kf_b]); ent_e.push_back(-1); ent_cam.push_back(-1); }
    for (int k : V.vel) { ent_a.push_back(-1); ent_b.push_back(H[k]); ent_e.push_back(-1); ent_cam.push_back(-1); }
    for (int e = 0; e < n_ext; ++e) { ent_a.push_back(-1); ent_b.push_back(H[n_kf + e]); ent_e.push_back(-1); ent_cam.push_back(-1); }
    const int n_entries = S.n_entries = (int)ent_a.size();
    std::vector<int>& hcnt = S.hcnt;
    hcnt.assign(n_ublocks + 1, 0);
    std::vector<int>& gcnt = wk.gcnt;
    gcnt.assign(n_pb + 1, 0);
    for (int en = 0; en < n_entries; ++en) {
        const int a = ent_a[en], b = ent_b[en], x = ent_e[en];
        if (a >= 0) { hcnt[ublock_id(n_pb, a, a)]++; gcnt[a]++; }
        if (b >= 0) { hcnt[ublock_id(n_pb, b, b)]++; gcnt[b]++; }
        if (a >= 0 && b >= 0) hcnt[ublock_id(n_pb, std::min(a, b), std::max(a, b))]++;
        if (x >= 0) {   // extrinsic blocks follow every KF block: (a, x), (b, x) are upper as they stand
            hcnt[ublock_id(n_pb, x, x)]++; gcnt[x]++;
            if (a >= 0) hcnt[ublock_id(n_pb, a, x)]++;
            if (b >= 0) hcnt[ublock_id(n_pb, b, x)]++;
        }
    }
    const std::vector<int>&hs0 = S.hs0 = prefix_sums(hcnt), &gs0 = S.gs0 = prefix_sums(gcnt);
    std::vector<int>&hfill = wk.hfill = hs0, &gfill = wk.gfill = gs0;
    std::vector<int>&seg_slot = S.seg_slot, &seg_gslot = S.seg_gslot;
    seg_slot.assign(SEG_STRIDE * (size_t)std::max(n_entries, 1), -1);
    seg_gslot.assign(GSEG_STRIDE * (size_t)std::max(n_entries, 1), -1);
    for (int en = 0; en < n_entries; ++en) {
        const int a = ent_a[en], b = ent_b[en], x = ent_e[en];
        int* sl = seg_slot.data() + SEG_STRIDE * (size_t)en;
        int* gl = seg_gslot.data() + GSEG_STRIDE * (size_t)en;
        sl[3] = 0;
        if (a >= 0) { sl[0] = hfill[ublock_id(n_pb, a, a)]++; gl[0] = gfill[a]++; }
        if (a >= 0 && b >= 0) { sl[1] = hfill[ublock_id(n_pb, std::min(a, b), std::max(a, b))]++; sl[3] = a > b; }
        if (b >= 0) { sl[2] = hfill[ublock_id(n_pb, b, b)]++; gl[1] = gfill[b]++; }
        if (x >= 0) {
            if (a >= 0) sl[4] = hfill[ublock_id(n_pb, a, x)]++;
            if (b >= 0) sl[5] = hfill[ublock_id(n_pb, b, x)]++;
            sl[6] = hfill[ublock_id(n_pb, x, x)]++;
            sl[7] = ent_cam[en];
            gl[2] = gfill[x]++;
        }
    }
    // the pose sample that writes each Hpp / b_p slot (fused expansion + assembly; -1: an edge item)
    S.hs_prod.assign(std::max(hs0[n_ublocks], 1), -1);
    S.gs_prod.assign(std::max(gs0[n_pb], 1), -1);
    for (int en = 0; en < n_smp; ++en) {
        const int* sl = seg_slot.data() + SEG_STRIDE * (size_t)en;
        const int* gl = seg_gslot.data() + GSEG_STRIDE * (size_t)en;
        for (int q : {0, 1, 2, 4, 5, 6})
            if (sl[q] >= 0) S.hs_prod[sl[q]] = en;
        for (int q = 0; q < 3; ++q)
            if (gl[q] >= 0) S.gs_prod[gl[q]] = en;
    }
    // Schur partial blocks per (tile, KF pair) and rhs partials per (tile, KF)
    std::vector<int>& scnt = S.scnt;
    scnt.assign(n_ublocks + 1, 0);
    std::vector<int>& gpcnt = wk.gpcnt;
    gpcnt.assign(n_pb + 1, 0);
    for (int s = 0; s < n_sent; ++s) scnt[ublock_id(n_pb, sent_k1[s], sent_k2[s])]++;
    for (int k : tkf_list) gpcnt[k]++;
    for (int h = 0; h < n_heavy; ++h) {   // a heavy landmark: every pair (a <= b) of its KFs, every KF
        const Span ks = L.kfs(T.hv_lm[h]);
        for (size_t a = 0; a < ks.size(); ++a) {
            gpcnt[ks[a]]++;
            for (size_t b = a; b < ks.size(); ++b) scnt[ublock_id(n_pb, ks[a], ks[b])]++;
        }
    }
    const std::vector<int>&ss0 = S.ss0 = prefix_sums(scnt), &gps0 = S.gps0 = prefix_sums(gpcnt);
    std::vector<int>&sfill = wk.sfill = ss0, &gpfill = wk.gpfill = gps0;
    S.sslot.resize(std::max(n_sent, 1));
    S.tkf_gslot.resize(std::max((int)tkf_list.size(), 1));
    for (int s = 0; s < n_sent; ++s) S.sslot[s] = sfill[ublock_id(n_pb, sent_k1[s], sent_k2[s])]++;
    for (size_t t = 0; t < tkf_list.size(); ++t) S.tkf_gslot[t] = gpfill[tkf_list[t]]++;
    for (int h = 0; h < n_heavy; ++h) {
        const Span ks = L.kfs(T.hv_lm[h]);
        for (size_t a = 0; a < ks.size(); ++a) {
            S.hp_gslot.push_back(gpfill[ks[a]]++);
            for (size_t b = a; b < ks.size(); ++b) S.hv_sslot.push_back(sfill[ublock_id(n_pb, ks[a], ks[b])]++);
        }
        S.hv_ss0.push_back((int)S.hv_sslot.size());
    }
    S.n_hslots = hs0[n_ublocks]; S.n_gslots = gs0[n_pb]; S.n_sslots = ss0[n_ublocks]; S.n_gpslots = gps0[n_pb];
    return S;
}

// ---- stage 7: observations in device order (scr.ob_*), camera records and the initial state.  lm_dev: lm_dev_of.
//      obs_dev: original observation -> device index, into the caller's array (it keeps its capacity)
inline DevOrder device_order(const Window& W, const Checks& C, const Vertices& V, const LmOrder& L,
                             const std::vector<int>& lm_dev, SetupClock& clock, SetupScratch& scr,
                             std::vector<int>& obs_dev) {
    DevOrder D;
    const lba_kf* kfs = W.kfs;
    const lba_obs* obs = W.obs;
    const lba_cam* cams = W.cams;
    const int n_kf = W.n_kf, n_obs = W.n_obs, n_cam = W.n_cam, n_ext = V.n_ext, n_kfs = V.n_kfs, nl = L.nl;
    const std::vector<int>&obs_of = scr.obs_of, &smp_of = scr.smp_of;
    std::vector<int>&ob_meta = sized(scr.ob_meta, n_obs), &ob_kfa = sized(scr.ob_kfa, n_obs), &ob_kfb = sized(scr.ob_kfb, n_obs),
                     &ob_smp = sized(scr.ob_smp, n_obs), &ob_lm = sized(scr.ob_lm, n_obs);
    std::vector<double>&ob_z = sized(scr.ob_z, 3 * (size_t)n_obs), &ob_w = sized(scr.ob_w, n_obs);
    obs_dev.assign(n_obs, -1);
    par_for(SETUP_PIECES, [&](int piece) {
        const lba_obs* const obsv = obs;
        const int *const oo = obs_of.data(), *const so = smp_of.data(), *const ld = lm_dev.data();
        int *const odev = obs_dev.data(), *const meta = ob_meta.data(), *const kfa = ob_kfa.data(), *const kfb = ob_kfb.data(),
            *const smp = ob_smp.data(), *const olm = ob_lm.data();
        double *const z = ob_z.data(), *const w = ob_w.data();
        const Range r = piece_range(n_obs, piece, SETUP_PIECES);
        for (int q = r.lo; q < r.hi; ++q) {
            const lba_obs& o = obsv[oo[q]];
            odev[oo[q]] = q;
            meta[q] = o.kind | (o.cam << 4);
            kfa[q] = is_gp(o.kind) ? o.kf_a : -1;
            kfb[q] = o.kf_b;
            smp[q] = so[oo[q]];
            olm[q] = ld[o.lm];
            z[3 * (size_t)q] = o.z[0]; z[3 * (size_t)q + 1] = o.z[1]; z[3 * (size_t)q + 2] = o.z[2];
            w[q] = o.w;
        }
    });
    clock.sub("device-order observations");
    // cameras: Tcb = Tbc^-1 as matrix (MultiKeyFrame::mTbc[c].cast<double>() normalises) and the
    // extrinsic factor Ad(Tbc) (lba::cam_record)
    D.camd.assign(CAMD_STRIDE * (size_t)std::max(n_cam, 1), 0.0);
    auto cam_se3 = [&](int c) {
        SE3 T;
        double q[4];
        normalize_q(cams[c].q, q);
        T.q = Quat{q[0], q[1], q[2], q[3]};
        for (int i = 0; i < 3; ++i) T.t[i] = cams[c].t[i];
        return T;
    };
    for (int c = 0; c < n_cam; ++c)
        cam_record(cam_se3(c), cams[c].fx, cams[c].fy, cams[c].cx, cams[c].cy, D.camd.data() + CAMD_STRIDE * c);
    // keyframe / landmark state (then the free extrinsics: Tbc as the pose, no velocity)
    std::vector<double>&kst = D.kst, &lst = D.lst;
    kst.assign(KF_STRIDE * (size_t)std::max(n_kfs, 1), 0.0);
    lst.assign(3 * (size_t)std::max(nl, 1), 0.0);
    for (int k = 0; k < n_kf; ++k) {
        double* o = kst.data() + KF_STRIDE * k;
        normalize_q(kfs[k].q, o);
        for (int i = 0; i < 3; ++i) o[4 + i] = kfs[k].t[i];
        for (int i = 0; i < 6; ++i) o[7 + i] = kfs[k].vel[i];
        o[13] = kfs[k].time;
        o[14] = kfs[k].bf;
    }
    D.kf_cam.assign(std::max(n_kfs, 1), -1);
    D.ep_kf.assign(std::max(n_ext, 1), 0);
    D.ep_data.assign(16 * (size_t)std::max(n_ext, 1), 0.0);
    for (int e = 0; e < n_ext; ++e) {
        const int c = C.ext_cams[e];
        const SE3 T = cam_se3(c);
        double* o = kst.data() + KF_STRIDE * (size_t)(n_kf + e);
        o[0] = T.q.x; o[1] = T.q.y; o[2] = T.q.z; o[3] = T.q.w;
        for (int i = 0; i < 3; ++i) o[4 + i] = T.t[i];
        D.kf_cam[n_kf + e] = c;
        D.ep_kf[e] = n_kf + e;
        // EdgeExtrinsicPrior(R): R_ = R.inverse() of the widened, normalised mRbc_ini (so3.hpp:229-231)
        double qi[4];
        normalize_q(cams[c].rbc_ini, qi);
        const Quat ri = qinv(Quat{qi[0], qi[1], qi[2], qi[3]});
        double* d = D.ep_data.data() + 16 * (size_t)e;
        d[0] = ri.x; d[1] = ri.y; d[2] = ri.z; d[3] = ri.w;
        for (int i = 0; i < 9; ++i) d[4 + i] = cams[c].rbc_info[i];
    }
    for (int d = 0; d < nl; ++d)
        for (int i = 0; i < 3; ++i) lst[3 * (size_t)d + i] = W.lm_xyz[3 * (size_t)L.order[d] + i];
    for (auto& e : V.pri) { D.pri_a.push_back(e.kf_a); D.pri_b.push_back(e.kf_b); }
    return D;
}

// (lba_setup_host_profile) a fingerprint of the tiling and the slab layout, and the largest tile shapes
// (lba_setup_tile_shapes): regular tiles in [0..8], segment tiles in [9..13]
inline Fingerprint layout_fingerprint(const Tiles& T, const Slots& S, const SetupScratch& scr) {
    const TileLists& l = T.l;
    Fingerprint F;
    uint32_t h = 2166136261u;
    auto mix = [&](const std::vector<int>& v) {
        for (int x : v) { h ^= (uint32_t)x; h *= 16777619u; }
    };
    mix(l.t_obs0); mix(l.t_lm0); mix(S.tsm_meta); mix(l.pair_rows); mix(l.lm_rows); mix(scr.pair_lk); mix(l.sent_l1);
    mix(l.sent_l2); mix(S.sslot); mix(S.tkf_gslot); mix(S.seg_slot); mix(scr.ob_row);
    mix(l.t_nobs); mix(l.t_nlm); mix(l.t_pair0); mix(l.t_npair); mix(l.t_smp0); mix(l.t_nsmp); mix(l.t_sent0);
    mix(l.t_nsent); mix(l.t_kf0); mix(l.t_nkf); mix(l.tkf_list); mix(l.sent_k1); mix(l.sent_k2); mix(scr.pair_r0);
    mix(scr.lm_r0);
    F.hash = h;
    const int n_tiles = F.n_tiles = T.n_tiles();
    int32_t* sh = F.shapes;
    auto up = [](int32_t& m, int v) { m = std::max<int32_t>(m, v); };
    for (int t = 0; t < n_tiles; ++t) {
        const bool reg = t < T.n_stiles;
        const int rows = scr.lm_r0[l.t_lm0[t] + l.t_nlm[t]] - scr.lm_r0[l.t_lm0[t]];
        int srows = 0;
        for (int s = l.t_smp0[t]; s < l.t_smp0[t] + l.t_nsmp[t]; ++s) srows = std::max(srows, l.tsm_rows[s] >> 16);
        ++sh[reg ? 0 : 9];
        up(sh[reg ? 1 : 10], l.t_nobs[t]);
        up(sh[reg ? 2 : 11], rows);
        up(sh[reg ? 3 : 12], l.t_nsmp[t]);
        if (reg) {
            up(sh[4], srows);
            up(sh[5], l.t_nlm[t]);
            up(sh[6], l.t_npair[t]);
            up(sh[7], l.t_nkf[t]);
            up(sh[8], l.t_nsent[t]);
        } else {
            up(sh[13], l.t_npair[t]);
        }
    }
    return F;
}

}  // namespace lba_setup
