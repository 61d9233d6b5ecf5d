// Host build of the product's projection-search maths (lba_match_math.hpp: the cell rectangle, the capacity, one job's
// gather and decision, a whole search in job order, the rotation pass) for tests/test_match_host.py and
// scripts/bench_match.py.  With -DMATCH_HARNESS_MAIN it is a stand-alone program that runs all of it on a generated
// search, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan -DMATCH_HARNESS_MAIN tests/native/match_harness.cpp -o match_harness_san && ./match_harness_san
#include "../../amc-slam_amd/csrc/lba_match_math.hpp"

#include <cstdio>

using namespace lba;

extern "C" int mh_rect(float x, float y, float r, const lba_match_cam* cam, int* out) {
    MatchRect R;
    if (!match_rect(x, y, r, *cam, &R)) return 0;
    out[0] = R.x0; out[1] = R.x1; out[2] = R.y0; out[3] = R.y1;
    return 1;
}

extern "C" int mh_capacity(const lba_match_job* job, const lba_match_cam* cams, const int32_t* cell_start) {
    return match_capacity(*job, cams[job->cam], cell_start);
}

// one job's candidate list as k_match_gather writes it; returns its length (at most cap entries are stored)
extern "C" int mh_gather(const lba_match_job* job, const lba_match_cam* cams, const int32_t* cell_start,
                         const int32_t* cell_feat, const lba_match_feat* feats, const lba_match_params* prm, int* feat,
                         int* dist, int cap) {
    std::vector<int> f, d;
    match_gather_host(*job, cams[job->cam], cell_start, cell_feat, feats, *prm, &f, &d);
    for (size_t i = 0; i < f.size() && (int)i < cap; ++i) { feat[i] = f[i]; dist[i] = d[i]; }
    return (int)f.size();
}

// one job's decision on its list against `taken`: out = {status, idx, best, best2}
extern "C" void mh_decide(const int* feat, const int* dist, const int* octave, int n, const int* taken,
                          const lba_match_params* prm, int* out) {
    MatchPick p;
    for (int i = 0; i < n; ++i)
        if (!taken[feat[i]]) match_pick(p, prm->mode, dist[i], octave[i], feat[i]);
    out[0] = match_decide(p, prm->mode, prm->th_high, prm->nn_ratio);
    out[1] = p.idx; out[2] = p.best; out[3] = p.best2;
}

extern "C" void mh_search(lba_match_search* S, const lba_match_cam* cams, const int32_t* cell_start,
                          const int32_t* cell_feat, lba_match_feat* feats, lba_match_job* jobs,
                          const lba_match_params* prm) {
    match_search_host(*S, cams, cell_start, cell_feat, feats, jobs, *prm);
}

// the rotation pass and the counts on decided jobs
extern "C" void mh_finish(lba_match_search* S, const lba_match_params* prm, lba_match_job* jobs, lba_match_feat* feats) {
    match_finish(*S, *prm, jobs, feats);
}

extern "C" int mh_rot_bin(float a_last, float a_cur) { return match_rot_bin(a_last, a_cur); }

extern "C" void mh_three_maxima(const int* histo, int* out) { match_three_maxima(histo, MATCH_HISTO, out, out + 1, out + 2); }

extern "C" int mh_pack_roundtrip(int local, int dist, int octave) {
    const uint32_t w = match_pack(local, dist, octave);
    return match_local(w) == local && match_wdist(w) == dist && match_octave(w) == octave;
}

#ifdef MATCH_HARNESS_MAIN
int main() {
    // a generated two-camera search: 600 features on a lattice with jitter, 500 jobs, among them the not-finite ones
    uint32_t seed = 12345u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    auto uni = [&rnd](float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffff) / 65536.0f; };
    const int n_cam = 2, n_feat = 600, n_jobs = 500;
    std::vector<lba_match_cam> cams(n_cam, lba_match_cam{0.f, 0.f, 0.1f, 0.1f, 0});
    std::vector<lba_match_feat> feats(n_feat);
    std::vector<std::vector<int>> cells((size_t)n_cam * MATCH_CELLS);
    for (int f = 0; f < n_feat; ++f) {
        lba_match_feat& F = feats[f];
        F = lba_match_feat{};
        F.x = uni(0.f, 640.f); F.y = uni(0.f, 480.f); F.angle = uni(0.f, 360.f);
        F.cam = f % n_cam; F.octave = (int)(rnd() % 8); F.taken = rnd() % 10 == 0;
        F.u_right = F.cam == 1 && rnd() % 2 ? F.x - uni(2.f, 20.f) : -1.f;
        for (uint32_t& d : F.desc) d = rnd() % 16 ? 0u : rnd();
        const int px = (int)roundf(F.x * 0.1f), py = (int)roundf(F.y * 0.1f);
        if (px >= 0 && px < MATCH_COLS && py >= 0 && py < MATCH_ROWS)
            cells[(size_t)F.cam * MATCH_CELLS + px * MATCH_ROWS + py].push_back(f);
    }
    std::vector<int32_t> cell_start(1, 0), cell_feat;
    for (const auto& c : cells) {
        cell_feat.insert(cell_feat.end(), c.begin(), c.end());
        cell_start.push_back((int32_t)cell_feat.size());
    }
    const float bad[] = {NAN, INFINITY, -INFINITY, 1e30f, -1e30f, 3e9f};
    std::vector<lba_match_job> jobs(n_jobs);
    for (int k = 0; k < n_jobs; ++k) {
        lba_match_job& J = jobs[k];
        J = lba_match_job{};
        J.x = uni(-30.f, 670.f); J.y = uni(-30.f, 510.f); J.radius = uni(1.f, 60.f); J.ur = J.x - uni(2.f, 20.f);
        J.angle = uni(0.f, 360.f); J.cam = (int)(rnd() % n_cam); J.blocks = rnd() % 4 != 0;
        J.min_level = (int)(rnd() % 8) - 1; J.max_level = rnd() % 3 ? J.min_level + 2 : -1;
        if (k % 50 == 7) (k % 3 == 0 ? J.x : k % 3 == 1 ? J.y : J.radius) = bad[(k / 50) % 6];
        for (uint32_t& d : J.desc) d = rnd() % 16 ? 0u : rnd();
    }
    int total = 0;
    for (int mode = 0; mode < 2; ++mode) {
        lba_match_params prm{mode, 100, 0.8f, n_cam - 1, mode, mode};
        lba_match_search S{0, n_cam, 0, n_feat, 0, n_jobs, 0, 0, 0, 0};
        std::vector<int> f(n_feat), d(n_feat);
        for (int k = 0; k < n_jobs; ++k) {
            const int cap = mh_capacity(&jobs[k], cams.data(), cell_start.data());
            const int n = mh_gather(&jobs[k], cams.data(), cell_start.data(), cell_feat.data(), feats.data(), &prm,
                                    f.data(), d.data(), n_feat);
            if (n > cap) { std::printf("job %d: %d candidates above the capacity %d\n", k, n, cap); return 1; }
        }
        mh_search(&S, cams.data(), cell_start.data(), cell_feat.data(), feats.data(), jobs.data(), &prm);
        std::printf("mode %d: n_matches %d, mono %d\n", mode, S.n_matches, S.n_matches_mono);
        total += S.n_matches;
    }
    int out[3];
    const int histo[MATCH_HISTO] = {20, 2, 1};
    mh_three_maxima(histo, out);
    if (out[0] != 0 || out[1] != 1 || out[2] != -1 || mh_rot_bin(909.9f, 10.f) != 0 || !mh_pack_roundtrip(8191, 256, 255)) return 1;
    std::printf("match harness: %d matches, clean\n", total);
    return total > 0 ? 0 : 1;
}
#endif
