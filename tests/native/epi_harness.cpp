// Host build of lba_epi_math.hpp for tests/test_epi_host.py (g++ -O2 -ffp-contract=off -shared) and
// scripts/bench_epipolar.py.  With -DEPI_HARNESS_MAIN it is a stand-alone program that runs all of it on generated
// keyframes, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan -DEPI_HARNESS_MAIN tests/native/epi_harness.cpp -o epi_harness_san && ./epi_harness_san
#include "../../amc-slam_amd/csrc/lba_epi_math.hpp"

#include <cstdio>

using namespace lba;

extern "C" void eh_table(const lba_tri_cam* c1, const lba_tri_cam* c2, double* tab) { epi_table(*c1, *c2, tab); }

extern "C" int eh_stereo(int cam, int n_cam, float u_right) { return epi_stereo(cam, n_cam, u_right); }

extern "C" int eh_near_epipole(const double* tab, const lba_epi_feat* f2) {
    return epi_near_epipole(tab, f2->x, f2->y, f2->scale);
}

extern "C" int eh_gate(const double* tab, const lba_epi_feat* f1, const lba_epi_feat* f2) {
    return epi_gate(tab, f1->x, f1->y, f2->x, f2->y, f2->sigma2);
}

// a whole pair: rows [n_feat(kf1)]; returns nmatches
extern "C" int eh_search(const lba_epi_kf* e1, const lba_epi_kf* e2, const lba_tri_cam* cams1, const lba_tri_cam* cams2,
                         int n_cam, const lba_epi_feat* feats, const int32_t* node_id, const int32_t* node_start,
                         const int32_t* node_feat, const lba_epi_params* prm, lba_epi_row* rows) {
    return epi_search_host(*e1, *e2, cams1, cams2, n_cam, feats, node_id, node_start, node_feat,
                           epi_params_or_default(prm), rows);
}

#ifdef EPI_HARNESS_MAIN
int main() {
    // two keyframes of two cameras, 300 keypoints each in 7 nodes (some in none), near-duplicate descriptors, some
    // with points, the last camera partly stereo; cameras a step apart, one pair also with equal centres (F12 = 0)
    uint32_t seed = 4711u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    auto uni = [&rnd](float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffff) / 65536.0f; };
    const int n_cam = 2, n_feat = 300, n_nodes = 7;
    std::vector<lba_tri_cam> cams(3 * n_cam);
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < n_cam; ++c) {
            lba_tri_cam& C = cams[k * n_cam + c];
            C = lba_tri_cam{};
            const double t[3] = {k == 1 ? -0.7 : 0.0, 0.1 * c, k == 1 ? 0.2 : 0.0};
            for (int i = 0; i < 3; ++i) { C.Tcw[4 * i + i] = 1.0; C.Tcw[4 * i + 3] = t[i]; C.Ow[i] = -t[i]; }
            C.fx = C.fy = 500.0; C.cx = 480.0; C.cy = 300.0; C.invfx = C.invfy = 1.0 / 500.0;
        }
    std::vector<lba_epi_feat> feats(2 * n_feat);
    std::vector<lba_epi_kf> ekfs(2);
    std::vector<int32_t> node_id, node_start, node_feat;
    for (int k = 0; k < 2; ++k) {
        std::vector<std::vector<int>> lists(n_nodes);
        for (int f = 0; f < n_feat; ++f) {
            lba_epi_feat& F = feats[k * n_feat + f];
            F = lba_epi_feat{};
            F.x = uni(0.f, 960.f); F.y = uni(0.f, 600.f); F.angle = uni(0.f, 360.f);
            F.cam = f % n_cam; F.has_point = rnd() % 7 == 0;
            F.u_right = F.cam == n_cam - 1 && rnd() % 2 ? F.x - uni(0.f, 20.f) : -1.f;
            F.scale = 1.f + 0.2f * (float)(rnd() % 4); F.sigma2 = F.scale * F.scale;
            for (uint32_t& d : F.desc) d = rnd() % 8 ? 0u : rnd() & 0x10101u;
            if (rnd() % 11) lists[rnd() % n_nodes].push_back(f);
        }
        ekfs[k] = lba_epi_kf{k * n_feat, n_feat, (int)node_id.size(), 0, (int)node_feat.size(), 0};
        int at = 0;
        for (int n = k; n < n_nodes; n += 1 + k) {     // the second keyframe holds every other node
            node_id.push_back(3 * n);
            node_start.push_back(at);
            node_feat.insert(node_feat.end(), lists[n].begin(), lists[n].end());
            at += (int)lists[n].size();
            ++ekfs[k].n_node;
        }
        node_id.push_back(-1);
        node_start.push_back(at);
    }
    long sum = 0;
    std::vector<lba_epi_row> rows(n_feat);
    for (int variant = 0; variant < 8; ++variant) {
        const lba_epi_params prm{variant == 7 ? 0 : 50, variant & 1, (variant >> 1) & 1, (variant >> 2) & 1};
        for (int other = 1; other < 3; ++other)     // a step apart; the same centres
            sum += epi_search_host(ekfs[0], ekfs[1], cams.data(), cams.data() + other * n_cam, n_cam, feats.data(),
                                   node_id.data(), node_start.data(), node_feat.data(), prm, rows.data());
        sum += epi_search_host(ekfs[1], ekfs[1], cams.data(), cams.data(), n_cam, feats.data(), node_id.data(),
                               node_start.data(), node_feat.data(), prm, rows.data());
    }
    const lba_epi_kf none{0, 0, 0, 0, 0, 0};
    sum += epi_search_host(none, ekfs[1], cams.data(), cams.data(), n_cam, feats.data(), node_id.data(), node_start.data(),
                           node_feat.data(), epi_params_or_default(nullptr), rows.data());
    sum += epi_search_host(ekfs[0], none, cams.data(), cams.data(), n_cam, feats.data(), node_id.data(), node_start.data(),
                           node_feat.data(), epi_params_or_default(nullptr), rows.data());
    std::printf("clean: %ld matches over the variants\n", sum);
    return sum > 0 ? 0 : 1;
}
#endif
