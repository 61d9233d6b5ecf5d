// lba_tracker.hpp — the tracking handle shared by its entry points: lba_track (lba_track.hip),
// lba_track_vel_ransac (lba_track_vel.hip), lba_sim3_optimize (lba_sim3.hip) and lba_posegraph_* (lba_posegraph.hip).
// One stream, device buffers that grow and are reused across calls.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/amc_lba.h"

constexpr int TR_MAXS = 16;   // pose samples per frame: distinct camera time stamps + the frame's own pose

struct lba_tracker {
    lba_config cfg{};
    hipStream_t stream = nullptr;
    lba_track_frame* d_frames = nullptr;
    lba_track_obs* d_obs = nullptr;
    int *d_obs_smp = nullptr, *d_smp0 = nullptr, *d_smp_obs0 = nullptr, *d_smp_kf = nullptr;
    double *d_smp_t = nullptr, *d_camd = nullptr, *d_chi2 = nullptr;
    size_t cap[9] = {};   // capacities of the buffers above, in elements
    char* d_vel = nullptr;   // lba_track_vel_ransac / lba_sim3_optimize: one arena per call (inputs, outputs, masks);
    size_t vel_cap = 0;      // its capacity in bytes.  Calls on a tracker are serial, so the two share it
    bool sim3_timed = false;             // lba_sim3_profile: bracket the launch with events
    hipEvent_t sim3_ev[2] = {nullptr, nullptr};
    double sim3_ms = -1.0;
    char* h_sim3 = nullptr;              // lba_sim3_optimize: the pinned host image of its arena
    size_t sim3_pin_cap = 0;
    char* d_pg = nullptr;                // lba_posegraph_*: the arena of a call (graph, lists, tiles, vectors)
    size_t pg_cap = 0;
    double pg_ms[3] = {-1.0, -1.0, -1.0};   // lba_posegraph_profile: planning, upload, device of the last optimize
    std::string err;
    ~lba_tracker() {
        for (hipEvent_t e : sim3_ev)
            if (e) (void)hipEventDestroy(e);
        if (h_sim3) (void)hipHostFree(h_sim3);
        if (d_pg) (void)hipFree(d_pg);
    }
};
