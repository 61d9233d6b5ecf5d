// lba_tracker.hpp — the tracking handle shared by its entry points: lba_track (lba_track.hip),
// lba_track_vel_ransac (lba_track_vel.hip), lba_sim3_ransac (lba_sim3_ransac.hip), lba_sim3_optimize (lba_sim3.hip),
// lba_posegraph_* (lba_posegraph.hip), lba_triangulate (lba_triangulate.hip), lba_match_project (lba_match.hip),
// lba_match_epipolar (lba_epipolar.hip), lba_match_bow (lba_bow.hip), lba_match_sim3_project (lba_sim3_project.hip),
// lba_match_fuse (lba_fuse.hip) and lba_mappoint_refresh (lba_mappoint.hip), and what they have in common on the host: the error path, the call arena (its typed sections and its plan are in
// lba_arena.hpp), the runner of a call on the pinned image (ArenaCall) and the camera records.
// One stream, device buffers that grow and are reused across calls.  Calls on a tracker are serial.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_arena.hpp"
#include "lba_math.hpp"

constexpr int TR_MAXS = 16;   // pose samples per frame: distinct camera time stamps + the frame's own pose

// the event bracket of one entry point (lba_*_profile): switched by the caller, read back after a timed call
struct CallTimer {
    bool on = false;
    double ms[6] = {-1.0, -1.0, -1.0, -1.0, -1.0, -1.0};   // between consecutive marks of the last timed call; -1 before the first
    int profile(int32_t on_, double* last_ms, int n) {
        on = on_ != 0;
        for (int i = 0; last_ms && i < n; ++i) last_ms[i] = ms[i];
        return LBA_OK;
    }
};

struct lba_tracker {
    lba_config cfg{};
    hipStream_t stream = nullptr;
    // lba_track: its nine buffers, each grown on its own
    lba_track_frame* d_frames = nullptr;
    lba_track_obs* d_obs = nullptr;
    int *d_obs_smp = nullptr, *d_smp0 = nullptr, *d_smp_obs0 = nullptr, *d_smp_kf = nullptr;
    double *d_smp_t = nullptr, *d_camd = nullptr, *d_chi2 = nullptr;
    size_t cap[9] = {};   // capacities of the buffers above, in elements
    // every other entry point: one arena per call (inputs, outputs, work)
    char* d_arena = nullptr;
    size_t arena_cap = 0;                // in bytes
    // lba_sim3_optimize / lba_sim3_ransac / lba_triangulate / lba_match_project / lba_match_epipolar / lba_match_bow:
    // the pinned host image of the arena's inputs and outputs, and the events of whichever of them is timed
    char* h_arena = nullptr;
    size_t h_arena_cap = 0;
    hipEvent_t ev[7] = {};   // (lba_match_sim3_project marks seven times)
    CallTimer sim3_timer, s3r_timer, tri_timer;   // one bracket around the launch(es)
    CallTimer match_timer;                        // k_match_gather, k_match_resolve
    CallTimer epi_timer;                          // k_epi_tables, k_epi_match
    CallTimer bow_timer;                          // k_bow_match
    CallTimer s3p_timer;                          // lba_match_sim3_project's six stretches
    CallTimer fuse_timer;                         // k_fuse
    CallTimer mp_timer;                           // k_mp_geom, k_mp_desc_wave, k_mp_desc_block
    // lba_match_sim3_project: its candidate lists, sized by a readback between two launches (the arena cannot grow there)
    char* d_cand = nullptr;
    size_t cand_cap = 0;                 // in bytes
    double pg_ms[3] = {-1.0, -1.0, -1.0};   // lba_posegraph_profile: planning, upload, device of the last optimize
    std::string err;
    // every buffer and event is freed here and nowhere else (lba_tracker_destroy: device, synchronise, stream, delete)
    ~lba_tracker() {
        void* bufs[] = {d_frames, d_obs, d_obs_smp, d_smp0, d_smp_obs0, d_smp_kf, d_smp_t, d_camd, d_chi2, d_arena, d_cand};
        for (void* b : bufs)
            if (b) (void)hipFree(b);
        if (h_arena) (void)hipHostFree(h_arena);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// ---- the error path: an entry point throws TrackerError inside its try block and returns tracker_fail(t, e)
struct TrackerError {
    int code;
    const char* msg;
};
#define TR_HIP(x)                                                           \
    do {                                                                    \
        if ((x) != hipSuccess) throw TrackerError{LBA_E_HIP, "HIP error"};  \
    } while (0)

inline int tracker_fail(lba_tracker* t, const TrackerError& e) {
    t->err = e.msg;
    return e.code;
}

// p holds at least `need` bytes afterwards; a buffer that grows is allocated anew with `alloc` bytes (the caller's
// policy), pinned host memory or device memory.  What p held is lost.
inline void grow_bytes(char*& p, size_t& cap, size_t need, size_t alloc, bool pinned = false) {
    if (need <= cap && p) return;
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
    if (pinned) TR_HIP(hipHostMalloc(reinterpret_cast<void**>(&p), alloc, hipHostMallocDefault));
    else TR_HIP(hipMalloc(reinterpret_cast<void**>(&p), alloc));
    cap = alloc;
}

// ---- a call on the pinned image, in this order: pin, fill the image, place, upload, mark, launch (the entry point's
// own hipLaunchKernelGGL and hipGetLastError), mark after each timed stretch, finish.  Every step throws TrackerError.
struct ArenaCall {
    lba_tracker* t;
    const ArenaPlan& plan;   // (by reference: a work section may join it between pin and place)
    CallTimer& timer;
    int marks = 0;
    // the host image of [0, down_end); a buffer that grows is allocated at twice the need
    char* pin() {
        TR_HIP(hipSetDevice(t->cfg.device));
        grow_bytes(t->h_arena, t->h_arena_cap, plan.down_end, plan.down_end * 2, true);
        return t->h_arena;
    }
    // the device arena of the whole plan, the same policy
    char* place() {
        if (plan.misordered) throw TrackerError{LBA_E_ARG, "the call arena's sections are out of order"};
        grow_bytes(t->d_arena, t->arena_cap, plan.total(), plan.total() * 2);
        return t->d_arena;
    }
    void upload() { TR_HIP(hipMemcpyAsync(t->d_arena, t->h_arena, plan.up_end, hipMemcpyHostToDevice, t->stream)); }
    // the next event, when this entry point is timed (the events are made by the first timed call)
    void mark() {
        if (!timer.on) return;
        if (!t->ev[0])
            for (hipEvent_t& e : t->ev) TR_HIP(hipEventCreate(&e));
        TR_HIP(hipEventRecord(t->ev[marks++], t->stream));
    }
    // the outputs into the image; the times between the marks (an untimed call leaves the timer's as they were)
    void finish() {
        TR_HIP(hipMemcpyAsync(t->h_arena + plan.up_end, t->d_arena + plan.up_end, plan.down_end - plan.up_end,
                              hipMemcpyDeviceToHost, t->stream));
        TR_HIP(hipStreamSynchronize(t->stream));
        for (int i = 0; i + 1 < marks; ++i) {
            float ms = -1.f;
            TR_HIP(hipEventElapsedTime(&ms, t->ev[i], t->ev[i + 1]));
            timer.ms[i] = ms;
        }
    }
};

// ---- the camera records of a call: lba_cam[] as [n_cam][CAMD_N]
inline std::vector<double> camd_pack(const lba_cam* cams, int n_cam) {
    std::vector<double> camd((size_t)n_cam * lba::CAMD_N);
    for (int c = 0; c < n_cam; ++c) {
        lba::Cam cm;
        for (int i = 0; i < 4; ++i) cm.q[i] = cams[c].q[i];
        for (int i = 0; i < 3; ++i) cm.t[i] = cams[c].t[i];
        cm.fx = cams[c].fx; cm.fy = cams[c].fy; cm.cx = cams[c].cx; cm.cy = cams[c].cy;
        lba::CamD d;
        lba::cam_derive(cm, &d);
        lba::camd_store(d, camd.data() + (size_t)c * lba::CAMD_N);
    }
    return camd;
}
