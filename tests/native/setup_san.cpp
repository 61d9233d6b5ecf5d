// Stand-alone program for a sanitizer build of lba_set_problem's host stages (amc-slam_amd/csrc/lba_setup.hpp):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__
//         -I<rocm>/include -pthread
// It builds three small synthetic windows, runs the stages in set_problem's order and prints each window's layout
// fingerprint.  Without arguments it runs itself twice as a child (LBA_SETUP_THREADS=1 and =8: the worker pool is
// sized once per process), compares the two outputs and exits non-zero if they differ or a child failed.
// tests/test_setup_san.py builds and runs it; it needs no GPU.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unistd.h>
#include <vector>

#include "../../amc-slam_amd/csrc/lba_setup.hpp"

using namespace lba_setup;

namespace {

struct Win {
    std::vector<lba_kf> kfs;
    std::vector<double> lm;
    std::vector<lba_obs> obs;
    std::vector<lba_prior> pri;
    std::vector<int32_t> vel;
    std::vector<lba_cam> cams;
    Window view() const {
        return Window{kfs.data(), (int)kfs.size(), lm.data(), (int)(lm.size() / 3), obs.data(), (int)obs.size(),
                      pri.data(), (int)pri.size(), vel.data(), (int)vel.size(), cams.data(), (int)cams.size()};
    }
};

unsigned rnd(unsigned& s) { return s = s * 1664525u + 1013904223u; }

// n_kf keyframes 0.1 s apart (the first fixed), n_lm landmarks each seen from 2 to 5 consecutive keyframes by
// keyframe observations (mono / stereo) and GP observations between keyframes; landmark 0 is seen seven times
// from every keyframe (more than TILE_KF pose blocks and TILE_OBS observations: a heavy landmark with several segment
// tiles).  ext: camera 1 has a free extrinsic.
Win make_window(int n_kf, int n_lm, bool ext, unsigned seed) {
    Win w;
    for (int k = 0; k < n_kf; ++k) {
        lba_kf kf{};
        kf.q[3] = 1.0;
        kf.t[0] = 0.3 * k;
        kf.time = 0.1 * k;
        kf.bf = 40.0;
        kf.fixed = k == 0;
        w.kfs.push_back(kf);
        if (k) w.pri.push_back(lba_prior{k - 1, k});
        w.vel.push_back(k);
    }
    for (int c = 0; c < 2; ++c) {
        lba_cam cam{};
        cam.q[3] = 1.0;
        cam.q[0] = 0.01 * c;
        cam.t[1] = 0.05 * c;
        cam.fx = cam.fy = 500.0;
        cam.cx = 320.0;
        cam.cy = 240.0;
        cam.ext_free = ext && c == 1;
        cam.rbc_ini[3] = 1.0;
        for (int i = 0; i < 3; ++i) cam.rbc_info[4 * i] = 0.2;
        w.cams.push_back(cam);
    }
    for (int l = 0; l < n_lm; ++l) {
        const int k0 = l == 0 ? 0 : (int)(rnd(seed) % (unsigned)(n_kf - 1));
        const int k1 = l == 0 ? n_kf : std::min(n_kf, k0 + 2 + (int)(rnd(seed) % 4u));
        w.lm.push_back(0.3 * k0 + 0.001 * l);
        w.lm.push_back(0.2);
        w.lm.push_back(4.0 + 0.01 * (l % 50));
        for (int kr = (l == 0 ? 7 : 1) * k0; kr < (l == 0 ? 7 : 1) * k1; ++kr) {
            const int k = kr / (l == 0 ? 7 : 1);
            lba_obs o{};
            o.lm = l;
            o.kf_b = k;
            o.w = 1.0;
            o.z[0] = 300.0 + l % 7; o.z[1] = 200.0 + k; o.z[2] = 290.0;
            const unsigned pick = rnd(seed) % 4u;
            if (k > 0 && pick < 2) {   // a GP observation between keyframes k - 1 and k, of camera 0 or 1
                o.kind = (pick == 1 && !ext) ? LBA_STEREO_GP : LBA_MONO_GP;
                o.kf_a = k - 1;
                o.cam = (int)(rnd(seed) % 2u);
                o.t = 0.1 * k - 0.025 * (1 + (int)(rnd(seed) % 3u));
            } else {
                o.kind = pick == 3 ? LBA_STEREO : LBA_MONO;
                o.kf_a = -1;
                o.cam = 1;
                o.t = 0.1 * k;
            }
            w.obs.push_back(o);
        }
    }
    return w;
}

// the stages in set_problem's order (lba_host.hip), then the fingerprint
Fingerprint host_stages(const Win& w, int* n_heavy, int* n_seg) {
    const Window W = w.view();
    SetupScratch scr;
    SetupClock clock(false);
    StageWork wk;
    const Checks C = validate_window(W, false, scr);
    const Vertices V = number_vertices(W, C, false, scr, wk);
    const GpSamples G = number_gp(W, V, clock, scr, wk);
    const LmOrder L = order_landmarks(W, V, G, clock, scr, wk);
    const Tiles T = build_tiles(W, V, G, L, clock, scr);
    const Slots S = build_slots(W, V, G, L, T, wk);
    std::vector<int> lm_dev;
    lm_dev_of(L, W.n_lm, lm_dev);
    std::vector<int> obs_dev;
    const DevOrder O = device_order(W, C, V, L, lm_dev, clock, scr, obs_dev);
    *n_heavy = (int)T.hv_lm.size();
    *n_seg = T.n_seg;
    if ((int)obs_dev.size() != W.n_obs || (int)O.kst.size() != KF_STRIDE * std::max(V.n_kfs, 1)) std::abort();
    return layout_fingerprint(T, S, scr);
}

int child() {
    struct Case { const char* name; Win w; bool heavy; };
    const Case cases[] = {{"gp_heavy", make_window(24, 4500, false, 1u), true},
                          {"free_extrinsic", make_window(20, 300, true, 2u), true},
                          {"empty", Win{}, false}};
    for (const Case& c : cases) {
        int n_heavy = 0, n_seg = 0;
        const Fingerprint F = host_stages(c.w, &n_heavy, &n_seg);
        std::printf("%s hash %08x tiles %d heavy %d segments %d\n", c.name, F.hash, F.n_tiles, n_heavy, n_seg);
        if (c.heavy && (n_heavy < 1 || n_seg < 2)) {
            std::fprintf(stderr, "%s: expected a heavy landmark with segment tiles\n", c.name);
            return 1;
        }
    }
    return 0;
}

bool run_child(const char* threads, std::string& out) {
    setenv("LBA_SETUP_THREADS", threads, 1);
    char self[4096];
    const ssize_t n = readlink("/proc/self/exe", self, sizeof self - 1);
    if (n <= 0) return false;
    self[n] = 0;
    FILE* f = popen(("'" + std::string(self) + "' child").c_str(), "r");
    if (!f) return false;
    char buf[256];
    while (std::fgets(buf, sizeof buf, f)) out += buf;
    return pclose(f) == 0;
}

}  // namespace

int main(int argc, char**) {
    if (argc > 1) return child();
    std::string one, eight;
    if (!run_child("1", one) || !run_child("8", eight)) {
        std::fprintf(stderr, "a child run failed\n%s%s", one.c_str(), eight.c_str());
        return 1;
    }
    std::printf("1 thread:\n%s8 threads:\n%s", one.c_str(), eight.c_str());
    if (one != eight || one.empty()) {
        std::fprintf(stderr, "the layouts differ between 1 and 8 threads\n");
        return 1;
    }
    return 0;
}
