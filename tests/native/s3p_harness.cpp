// Host build of amc-slam_amd/csrc/lba_s3p_math.hpp for tests/test_s3p_host.py: the pose chain, one job's projection and
// a whole search resolved sequentially, behind a C interface.  With -DS3P_HARNESS_MAIN it is a stand-alone program
// that runs a generated problem (the sanitizer build).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../amc-slam_amd/csrc/lba_s3p_math.hpp"

using namespace lba;

extern "C" void sh_pose(const lba_s3p_kf* kf, const lba_s3p_cam* cam, const lba_s3p_search* S, double* tcw) {
    s3p_pose(*kf, *cam, S->q, S->t, S->s, tcw);
}

// out: status, level; xyr: x, y, radius
extern "C" void sh_project(const float* tcw, const lba_s3p_kf* kf, const lba_s3p_cam* cam, const lba_s3p_point* P,
                           const float* sf, const lba_s3p_params* prm, int* out, float* xyr) {
    const S3pJob J = s3p_project(tcw, *cam, *P, prm->th, prm->proj_form, kf->log_scale_factor, kf->n_levels, sf);
    out[0] = J.status; out[1] = J.level;
    xyr[0] = J.x; xyr[1] = J.y; xyr[2] = J.radius;
}

// PredictScale's quotient before the ceil, as s3p_level forms it (for the M_LEVEL measurement)
extern "C" double sh_quotient(float max_distance, float dist, float log_scale_factor) {
    const float ratio = max_distance / dist;
    return log((double)ratio) / (double)log_scale_factor;
}

extern "C" int sh_level(float max_distance, float dist, float log_scale_factor, int n_levels) {
    return s3p_level(max_distance, dist, log_scale_factor, n_levels);
}

extern "C" int sh_capacity(float x, float y, float r, const lba_match_cam* gc, const int32_t* cam_cell_start) {
    return s3p_capacity(x, y, r, *gc, cam_cell_start);
}

extern "C" int sh_search(const lba_s3p_kf* kf, const lba_s3p_cam* kcams, const lba_match_cam* gcams, const float* sf,
                         const int32_t* cell_start, const int32_t* cell_feat, const lba_match_feat* feats, int n_feat,
                         const lba_s3p_search* S, const lba_s3p_point* points, const uint8_t* taken,
                         const lba_s3p_params* prm, lba_s3p_row* rows, int32_t* feat_point, lba_s3p_pose* poses) {
    return s3p_search_host(*kf, kcams, gcams, sf, cell_start, cell_feat, feats, n_feat, *S, points, taken, *prm, rows,
                           feat_point, poses);
}

// the host half of the way without this entry point: the poses and every job's projection of one hypothesis
extern "C" void sh_project_all(const lba_s3p_kf* kf, const lba_s3p_cam* kcams, const float* sf, const lba_s3p_search* S,
                               const lba_s3p_point* points, const lba_s3p_params* prm, lba_s3p_row* rows,
                               lba_s3p_pose* poses) {
    for (int c = 0; c < kf->n_cam; ++c) {
        s3p_pose(*kf, kcams[c], S->q, S->t, S->s, poses[c].tcw_d);
        for (int i = 0; i < 12; ++i) poses[c].tcw[i] = (float)poses[c].tcw_d[i];
    }
    for (int p = 0; p < S->n_points; ++p)
        for (int c = 0; c < kf->n_cam; ++c) {
            const S3pJob J = s3p_project(poses[c].tcw, kcams[c], points[S->point0 + p], prm->th, prm->proj_form,
                                         kf->log_scale_factor, kf->n_levels, sf);
            rows[(size_t)p * kf->n_cam + c] = lba_s3p_row{J.status, -1, 256, J.level, J.x, J.y, J.radius, 0};
        }
}

extern "C" int sh_params_ok(const lba_s3p_params* prm) { return s3p_params_error(*prm) == nullptr; }

#ifdef S3P_HARNESS_MAIN
int main() {
    uint32_t seed = 4242u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    auto uni = [&rnd](float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffff) / 65536.0f; };
    const int n_cam = 3, n_feat = 900, n_points = 700, n_levels = 8;
    lba_s3p_kf K{};
    K.stamp = 10.1; K.stamp_prev = 10.0;
    const float q[4] = {0.05f, -0.02f, 0.01f, 0.998f}, qp[4] = {0.04f, -0.02f, 0.015f, 0.998f};
    for (int i = 0; i < 4; ++i) { K.q[i] = q[i]; K.q_prev[i] = qp[i]; }
    K.t[0] = 0.3f; K.t[1] = -0.1f; K.t[2] = 0.2f; K.t_prev[0] = 0.25f; K.t_prev[1] = -0.1f; K.t_prev[2] = 0.15f;
    for (int i = 0; i < 6; ++i) { K.v[i] = uni(-0.5f, 0.5f); K.v_prev[i] = uni(-0.5f, 0.5f); }
    K.log_scale_factor = logf(1.2f); K.has_prev = 1; K.n_levels = n_levels; K.n_cam = n_cam;
    std::vector<float> sf(n_levels, 1.0f);
    for (int i = 1; i < n_levels; ++i) sf[i] = sf[i - 1] * 1.2f;
    std::vector<lba_s3p_cam> kc(n_cam);
    std::vector<lba_match_cam> gc(n_cam, lba_match_cam{0.f, 0.f, 0.1f, 0.1f, 0});
    for (int c = 0; c < n_cam; ++c) {
        kc[c] = lba_s3p_cam{};
        kc[c].stamp = 10.0 + 0.1 * (c + 1) / n_cam;
        kc[c].q_bc[1] = sinf(0.4f * c); kc[c].q_bc[3] = cosf(0.4f * c);
        kc[c].t_bc[0] = 0.05f * c;
        kc[c].fx = kc[c].fy = 320.f; kc[c].cx = 320.f; kc[c].cy = 240.f; kc[c].max_x = 640.f; kc[c].max_y = 480.f;
        kc[c].ow[0] = -0.3f; kc[c].ow[1] = 0.1f; kc[c].ow[2] = -0.2f;
    }
    std::vector<lba_match_feat> feats(n_feat);
    std::vector<std::vector<int>> cells((size_t)n_cam * MATCH_CELLS);
    for (int f = 0; f < n_feat; ++f) {
        lba_match_feat& Ft = feats[f];
        Ft = lba_match_feat{};
        Ft.x = uni(0.f, 640.f); Ft.y = uni(0.f, 480.f); Ft.cam = f % n_cam; Ft.octave = (int)(rnd() % 8); Ft.u_right = -1.f;
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
        if (p % 40 == 9) { P.pos[0] = kc[0].ow[0]; P.pos[1] = kc[0].ow[1]; P.pos[2] = kc[0].ow[2]; P.min_dist = 0.f; }   // (h)
        for (uint32_t& d : P.desc) d = rnd() % 16 ? 0u : rnd();
    }
    std::vector<uint8_t> taken(n_feat);
    for (auto& b : taken) b = rnd() % 10 == 0;
    int total = 0;
    for (int form = 0; form < 2; ++form) {
        lba_s3p_search S{};
        S.q[0] = 0.05f; S.q[1] = -0.021f; S.q[2] = 0.01f; S.q[3] = 0.998f;
        S.t[0] = 0.31f; S.t[1] = -0.1f; S.t[2] = 0.2f; S.s = 1.02f;
        S.n_points = n_points;
        const lba_s3p_params prm{8, 50, 1.5f, form};
        std::vector<lba_s3p_row> rows((size_t)n_points * n_cam);
        std::vector<int32_t> fp(n_feat);
        std::vector<lba_s3p_pose> poses(n_cam);
        const int n = sh_search(&K, kc.data(), gc.data(), sf.data(), cell_start.data(), cell_feat.data(), feats.data(), n_feat,
                                &S, pts.data(), form ? taken.data() : nullptr, &prm, rows.data(), fp.data(), poses.data());
        int live = 0;
        for (const auto& r : rows) {
            live += r.status <= LBA_S3P_TOO_FAR;
            if (r.status <= LBA_S3P_TOO_FAR && (r.level < 0 || r.level >= n_levels)) return 1;
        }
        std::printf("form %d: %d matches, %d live jobs\n", form, n, live);
        total += n;
    }
    const lba_s3p_params g{8, 50, 6.0f, 0};
    if (sh_params_ok(&g) || sh_level(0.f, 0.f, 0.18f, 8) != 0 || sh_level(1.f, 0.f, 0.18f, 8) != 7) return 1;
    std::printf("s3p harness: %d matches, clean\n", total);
    return total > 0 ? 0 : 1;
}
#endif
