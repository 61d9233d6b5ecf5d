// Host build of amc-slam_amd/csrc/lba_mp_math.hpp for tests/test_mp_host.py and scripts/bench_mappoint.py: a batch of
// points refreshed one after the other on one thread, behind a C interface.  With -DMP_HARNESS_MAIN it is a stand-alone
// program that runs a generated batch both ways (the sanitizer build).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../amc-slam_amd/csrc/lba_mp_math.hpp"

using namespace lba;

// bisect != 0: the descriptor is chosen with mp_row_median, as the kernels choose it
extern "C" void mh_refresh(lba_mp_point* points, int n_points, const lba_mp_obs* obs, const lba_tri_kf* kfs,
                           const lba_epi_kf* ekfs, const lba_tri_cam* cams, const lba_epi_feat* feats,
                           const int32_t* kf_bad, float scale_top, int bisect) {
    for (int p = 0; p < n_points; ++p) mp_refresh_point(points[p], obs, kfs, ekfs, cams, feats, kf_bad, scale_top, bisect != 0);
}

#ifdef MP_HARNESS_MAIN
int main() {
    uint32_t seed = 4242u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    auto uni = [&rnd](float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffff) / 65536.0f; };
    const int n_kf = 40, n_cam = 3, per_cam = 5, n_points = 400;
    std::vector<lba_tri_kf> kfs(n_kf);
    std::vector<lba_epi_kf> ekfs(n_kf);
    std::vector<lba_tri_cam> cams((size_t)n_kf * n_cam);
    std::vector<lba_epi_feat> feats((size_t)n_kf * n_cam * per_cam);
    std::vector<int32_t> kf_bad(n_kf);
    for (int k = 0; k < n_kf; ++k) {
        kfs[k] = lba_tri_kf{};
        kfs[k].cam0 = k * n_cam;
        ekfs[k] = lba_epi_kf{k * n_cam * per_cam, n_cam * per_cam, 0, 0, 0, 0};
        kf_bad[k] = rnd() % 6 == 0;
        for (int c = 0; c < n_cam; ++c) {
            lba_tri_cam& C = cams[(size_t)k * n_cam + c];
            C = lba_tri_cam{};
            for (double& o : C.Ow) o = uni(-3.f, 3.f);
            for (int j = 0; j < per_cam; ++j) {
                lba_epi_feat& F = feats[(size_t)(k * n_cam + c) * per_cam + j];
                F = lba_epi_feat{};
                F.cam = c;
                F.scale = powf(1.2f, (float)(rnd() % 8));
                for (uint32_t& d : F.desc) d = rnd() % 4 ? rnd() * 977u : 0u;
            }
        }
    }
    std::vector<lba_mp_obs> obs;
    std::vector<lba_mp_point> pts(n_points);
    const float odd[] = {NAN, INFINITY, -INFINITY, 1e30f, -1e30f, 0.f};
    for (int p = 0; p < n_points; ++p) {
        lba_mp_point& P = pts[p];
        P = lba_mp_point{};
        for (float& x : P.pos) x = uni(-8.f, 8.f);
        if (p % 30 == 3) P.pos[p % 3] = odd[(p / 30) % 6];
        P.obs0 = (int)obs.size();
        const int n = p % 25 == 0 ? 0 : p % 40 == 7 ? 300 + (int)(rnd() % 700) : 1 + (int)(rnd() % 70);
        for (int i = 0; i < n; ++i) {
            const int k = (int)((int64_t)i * n_kf / n);   // keyframes ascending
            obs.push_back(lba_mp_obs{k, (int)(rnd() % (n_cam * per_cam))});
        }
        P.n_obs = n;
        P.ref_kf = n && rnd() % 10 ? obs[(size_t)P.obs0 + rnd() % n].kf : -1;
        P.bad = rnd() % 30 == 0;
        P.ops = 1 + (int)(rnd() % 3);
        if (p % 30 == 11 && n) {   // on a camera centre
            const lba_mp_obs o = obs[(size_t)P.obs0];
            const double* O = cams[(size_t)o.kf * n_cam + feats[(size_t)ekfs[o.kf].feat0 + o.feat].cam].Ow;
            for (int i = 0; i < 3; ++i) P.pos[i] = (float)O[i];
        }
    }
    std::vector<lba_mp_point> a = pts, b = pts;
    mh_refresh(a.data(), n_points, obs.data(), kfs.data(), ekfs.data(), cams.data(), feats.data(), kf_bad.data(), 3.583f, 0);
    mh_refresh(b.data(), n_points, obs.data(), kfs.data(), ekfs.data(), cams.data(), feats.data(), nullptr, 3.583f, 0);
    std::vector<lba_mp_point> c = pts;
    mh_refresh(c.data(), n_points, obs.data(), kfs.data(), ekfs.data(), cams.data(), feats.data(), kf_bad.data(), 3.583f, 1);
    int chosen = 0, nan = 0;
    for (int p = 0; p < n_points; ++p) {
        if (a[p].best_obs != c[p].best_obs || a[p].best_median != c[p].best_median ||
            std::memcmp(a[p].desc, c[p].desc, sizeof a[p].desc) != 0) {
            std::printf("point %d: sort and bisection differ\n", p);
            return 1;
        }
        if (a[p].best_obs >= a[p].n_obs || b[p].best_obs >= b[p].n_obs) return 1;
        chosen += a[p].best_obs >= 0;
        nan += std::isnan(a[p].normal[0]);
    }
    std::printf("mp harness: %d points, %d descriptors chosen, %d NaN normals, clean\n", n_points, chosen, nan);
    return chosen > 0 && nan > 0 ? 0 : 1;
}
#endif
