// Host build of amc-slam_amd/csrc/lba_fuse_math.hpp for tests/test_fuse_host.py: one job's projection and a whole search
// run sequentially, behind a C interface.  With -DFUSE_HARNESS_MAIN it is a stand-alone program that runs a generated
// problem in both modes (the sanitizer build).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../amc-slam_amd/csrc/lba_fuse_math.hpp"

using namespace lba;

// out: status, level; xyr: x, y, radius, ur
extern "C" void fh_project(const lba_fuse_target* T, const lba_fuse_cam* cam, const lba_s3p_point* P, const float* sf,
                           int mode, int c, float th, int* out, float* xyr) {
    const FuseJob J = fuse_project(*cam, *P, mode, c, T->n_cam, th, T->bf, T->log_scale_factor, T->n_levels, sf + T->sf0);
    out[0] = J.status; out[1] = J.level;
    xyr[0] = J.x; xyr[1] = J.y; xyr[2] = J.radius; xyr[3] = J.ur;
}

extern "C" int fh_search(const lba_fuse_target* T, const lba_fuse_cam* fcams, const lba_match_cam* gcams, const float* sf,
                         const float* sigma, const int32_t* cell_start, const int32_t* cell_feat,
                         const lba_match_feat* feats, const lba_fuse_search* S, const lba_s3p_point* points, int th_low,
                         lba_fuse_row* rows) {
    return fuse_search(*T, fcams, gcams, sf, sigma, cell_start, cell_feat, feats, *S, points, th_low, rows);
}

#ifdef FUSE_HARNESS_MAIN
int main() {
    uint32_t seed = 777u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    auto uni = [&rnd](float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffff) / 65536.0f; };
    const int n_cam = 3, n_feat = 900, n_points = 700, n_levels = 8;
    std::vector<float> sf(n_levels, 1.0f), sigma(n_levels, 1.0f);
    for (int i = 1; i < n_levels; ++i) sf[i] = sf[i - 1] * 1.2f;
    for (int i = 0; i < n_levels; ++i) sigma[i] = 1.0f / (sf[i] * sf[i]);
    lba_fuse_target T{};
    T.n_cam = n_cam; T.n_feat = n_feat; T.bf = 40.f; T.log_scale_factor = logf(1.2f); T.n_levels = n_levels;
    std::vector<lba_fuse_cam> fc(n_cam);
    std::vector<lba_match_cam> gc(n_cam, lba_match_cam{0.f, 0.f, 0.1f, 0.1f, 0});
    for (int c = 0; c < n_cam; ++c) {
        fc[c] = lba_fuse_cam{};
        fc[c].q_cw[1] = sinf(0.3f * c); fc[c].q_cw[3] = cosf(0.3f * c);
        fc[c].t_cw[0] = 0.05f * c;
        fc[c].fx = fc[c].fy = 320.f; fc[c].cx = 320.f; fc[c].cy = 240.f; fc[c].max_x = 640.f; fc[c].max_y = 480.f;
        fc[c].ow[0] = -0.05f * c;
    }
    std::vector<lba_match_feat> feats(n_feat);
    std::vector<std::vector<int>> cells((size_t)n_cam * MATCH_CELLS);
    for (int f = 0; f < n_feat; ++f) {
        lba_match_feat& Ft = feats[f];
        Ft = lba_match_feat{};
        Ft.x = uni(0.f, 640.f); Ft.y = uni(0.f, 480.f); Ft.cam = f % n_cam; Ft.octave = (int)(rnd() % 9);
        Ft.u_right = rnd() % 3 ? -1.f : uni(0.f, 600.f);
        for (uint32_t& d : Ft.desc) d = rnd() % 16 ? 0u : rnd();
        const int px = (int)roundf(Ft.x * 0.1f), py = (int)roundf(Ft.y * 0.1f);
        if (px >= 0 && px < MATCH_COLS && py >= 0 && py < MATCH_ROWS)
            cells[(size_t)Ft.cam * MATCH_CELLS + px * MATCH_ROWS + py].push_back(f);
    }
    std::vector<int32_t> cell_start(1, 0), cell_feat;
    for (const auto& c : cells) {
        cell_feat.insert(cell_feat.end(), c.begin(), c.end());
        cell_start.push_back((int32_t)cell_feat.size());
    }
    const float bad[] = {NAN, INFINITY, -INFINITY, 1e30f, -1e30f, 0.f};
    std::vector<lba_s3p_point> pts(n_points);
    for (int p = 0; p < n_points; ++p) {
        lba_s3p_point& P = pts[p];
        P = lba_s3p_point{};
        P.pos[0] = uni(-6.f, 6.f); P.pos[1] = uni(-4.f, 4.f); P.pos[2] = uni(-2.f, 12.f);
        P.normal[2] = 1.f; P.normal[0] = uni(-0.5f, 0.5f);
        P.min_dist = 0.1f; P.max_dist = 40.f; P.max_distance = uni(0.5f, 60.f); P.skip = rnd() % 20 == 0;
        if (p % 40 == 3) P.pos[p % 3] = bad[(p / 40) % 6];
        if (p % 40 == 5) P.max_distance = bad[(p / 40) % 6];
        if (p % 40 == 9) { P.pos[0] = P.pos[1] = P.pos[2] = 0.f; P.min_dist = 0.f; }   // dist == 0 in camera 0
        for (uint32_t& d : P.desc) d = rnd() % 16 ? 0u : rnd();
    }
    int total = 0;
    for (int mode = 0; mode < 2; ++mode) {
        lba_fuse_search S{};
        S.n_points = n_points; S.mode = mode; S.th = mode ? 4.f : 3.f;
        std::vector<lba_fuse_row> rows((size_t)n_points * n_cam);
        const int n = fh_search(&T, fc.data(), gc.data(), sf.data(), sigma.data(), cell_start.data(), cell_feat.data(),
                                feats.data(), &S, pts.data(), 50, rows.data());
        int live = 0;
        for (const auto& r : rows) {
            live += r.status <= LBA_FUSE_TOO_FAR;
            if (r.status <= LBA_FUSE_TOO_FAR && (r.level < 0 || r.level >= n_levels)) return 1;
            if (r.status == LBA_FUSE_OK && (r.feat < 0 || r.feat >= n_feat)) return 1;
        }
        std::printf("mode %d: %d accepted, %d live jobs\n", mode, n, live);
        total += live;
    }
    std::printf("fuse harness: %d live jobs, clean\n", total);
    return total > 0 ? 0 : 1;
}
#endif
