// lba_tracker.hpp — the tracking handle shared by its entry points: lba_track (lba_track.hip),
// lba_track_vel_ransac (lba_track_vel.hip), lba_sim3_ransac (lba_sim3_ransac.hip), lba_sim3_optimize (lba_sim3.hip),
// lba_posegraph_* (lba_posegraph.hip), lba_triangulate (lba_triangulate.hip) and lba_match_project (lba_match.hip),
// and what they have in common on the host: the error path, the per-call arena and the camera records.
// One stream, device buffers that grow and are reused across calls.  Calls on a tracker are serial.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_math.hpp"

constexpr int TR_MAXS = 16;   // pose samples per frame: distinct camera time stamps + the frame's own pose

struct lba_tracker {
    lba_config cfg{};
    hipStream_t stream = nullptr;
    // lba_track: its nine buffers, each grown on its own
    lba_track_frame* d_frames = nullptr;
    lba_track_obs* d_obs = nullptr;
    int *d_obs_smp = nullptr, *d_smp0 = nullptr, *d_smp_obs0 = nullptr, *d_smp_kf = nullptr;
    double *d_smp_t = nullptr, *d_camd = nullptr, *d_chi2 = nullptr;
    size_t cap[9] = {};   // capacities of the buffers above, in elements
    // lba_track_vel_ransac / lba_sim3_optimize / lba_posegraph_*: one arena per call (inputs, outputs, work)
    char* d_arena = nullptr;
    size_t arena_cap = 0;                // in bytes
    char* h_sim3 = nullptr;              // lba_sim3_optimize / lba_sim3_ransac / lba_triangulate / lba_match_project: the pinned host image of the arena
    size_t sim3_pin_cap = 0;
    bool sim3_timed = false;             // lba_sim3_profile: bracket the launch with events
    hipEvent_t sim3_ev[2] = {nullptr, nullptr};
    double sim3_ms = -1.0;
    bool s3r_timed = false;              // lba_sim3_ransac_profile: the same bracket (and events) for its two launches
    double s3r_ms = -1.0;
    bool tri_timed = false;              // lba_triangulate_profile: the same bracket (and events) for its launch
    double tri_ms = -1.0;
    bool match_timed = false;            // lba_match_profile: events around lba_match_project's two launches
    hipEvent_t match_ev[3] = {nullptr, nullptr, nullptr};
    double match_ms[2] = {-1.0, -1.0};   // k_match_gather, k_match_resolve
    double pg_ms[3] = {-1.0, -1.0, -1.0};   // lba_posegraph_profile: planning, upload, device of the last optimize
    std::string err;
    // every buffer and event is freed here and nowhere else (lba_tracker_destroy: device, synchronise, stream, delete)
    ~lba_tracker() {
        void* bufs[] = {d_frames, d_obs, d_obs_smp, d_smp0, d_smp_obs0, d_smp_kf, d_smp_t, d_camd, d_chi2, d_arena};
        for (void* b : bufs)
            if (b) (void)hipFree(b);
        if (h_sim3) (void)hipHostFree(h_sim3);
        for (hipEvent_t e : sim3_ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : match_ev)
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

// ---- the arena of a call: sections at 256-byte offsets, laid out on the host, one allocation on the device
struct ArenaLayout {
    size_t total = 0;
    size_t take(size_t bytes) {
        const size_t o = total;
        total += (bytes + 255) & ~size_t(255);
        return o;
    }
};

// host image of an arena's leading sections (the upload); `lay` goes on handing out the sections behind it
struct ArenaImage {
    ArenaLayout lay;
    std::vector<char> bytes;
    template <typename T>
    size_t put(const T* p, size_t count) {
        const size_t o = lay.take(count * sizeof(T));
        bytes.resize(lay.total, 0);
        if (count) std::memcpy(bytes.data() + o, p, count * sizeof(T));
        return o;
    }
    template <typename T>
    size_t put(const std::vector<T>& v) { return put(v.data(), v.size()); }
};

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
