// Host build of lba_bow_math.hpp for tests/test_bow_host.py (g++ -O2 -ffp-contract=off -shared) and
// scripts/bench_bow.py.  With -DBOW_HARNESS_MAIN it is a stand-alone program that runs all of it on generated
// keyframes, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan -DBOW_HARNESS_MAIN tests/native/bow_harness.cpp -o bow_harness_san && ./bow_harness_san
#include "../../amc-slam_amd/csrc/lba_bow_math.hpp"

#include <cstdio>

using namespace lba;

// the scan of the candidates (dist[i], pos[i]), i < n, in the order given (ascending pos within a part): out = b1, pos1, b2
extern "C" void bh_fold_list(const int* dist, const int* pos, int n, int* out) {
    BowBest s;
    for (int i = 0; i < n; ++i) bow_fold(s, dist[i], pos[i]);
    out[0] = s.b1; out[1] = s.pos1; out[2] = s.b2;
}

extern "C" void bh_merge(const int* a, const int* b, int* out) {
    const BowBest r = bow_merge(BowBest{a[0], a[1], a[2]}, BowBest{b[0], b[1], b[2]});
    out[0] = r.b1; out[1] = r.pos1; out[2] = r.b2;
}

extern "C" int bh_accept(int b1, int b2, int mode, int th_low, float nn_ratio) {
    return bow_accept(b1, b2, mode, th_low, nn_ratio);
}

// a whole pair: rows [n_feat(side 1)]; returns nmatches
extern "C" int bh_search(const lba_epi_kf* e1, const lba_epi_kf* e2, const lba_epi_feat* feats, const int32_t* node_id,
                         const int32_t* node_start, const int32_t* node_feat, const lba_bow_params* prm, lba_bow_row* rows) {
    return bow_search_host(*e1, *e2, feats, node_id, node_start, node_feat, bow_params_or_default(prm), rows);
}

// every pair of a batch, one after the other on this thread: rows packed pair after pair; returns the matches' sum
extern "C" long bh_search_batch(const lba_bow_pair* pairs, int n_pairs, const lba_epi_kf* ekfs, const lba_epi_feat* feats,
                                const int32_t* node_id, const int32_t* node_start, const int32_t* node_feat,
                                const lba_bow_params* prm, lba_bow_row* rows, int32_t* n_matches) {
    long sum = 0;
    for (int p = 0; p < n_pairs; ++p) {
        n_matches[p] = bow_search_host(ekfs[pairs[p].kf1], ekfs[pairs[p].kf2], feats, node_id, node_start, node_feat,
                                       bow_params_or_default(prm), rows);
        rows += ekfs[pairs[p].kf1].n_feat;
        sum += n_matches[p];
    }
    return sum;
}

#ifdef BOW_HARNESS_MAIN
int main() {
    uint32_t seed = 1234u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    // ---- the merge against the scan: random lists with many equal distances and some of 256, dealt to 1 .. 64 parts
    // as the kernel deals candidates to lanes, the parts merged in a random order
    for (int trial = 0; trial < 2000; ++trial) {
        const int n = (int)(rnd() % 200);
        std::vector<int> dist(n);
        for (int& d : dist) d = rnd() % 5 ? (int)(rnd() % 12) * 23 : 256;
        BowBest whole;
        for (int i = 0; i < n; ++i) bow_fold(whole, dist[i], i);
        const int parts = 1 + (int)(rnd() % 64);
        std::vector<BowBest> part(parts);
        for (int i = 0; i < n; ++i) bow_fold(part[i % parts], dist[i], i);
        while (part.size() > 1) {
            const size_t a = rnd() % part.size();
            size_t b = rnd() % (part.size() - 1);
            if (b >= a) ++b;
            part[a] = bow_merge(part[a], part[b]);
            part.erase(part.begin() + (long)b);
        }
        if (part[0].b1 != whole.b1 || part[0].pos1 != whole.pos1 || part[0].b2 != whole.b2) {
            std::printf("merge differs from the scan in trial %d\n", trial);
            return 1;
        }
    }
    // ---- whole pairs: three keyframes of 300 keypoints in 7 nodes (some in none), near-duplicate descriptors, most
    // with points; the second keyframe holds every other node, the third none
    const int n_feat = 300, n_nodes = 7;
    std::vector<lba_epi_feat> feats(2 * n_feat);
    std::vector<lba_epi_kf> ekfs(3);
    std::vector<int32_t> node_id, node_start, node_feat;
    for (int k = 0; k < 2; ++k) {
        std::vector<std::vector<int>> lists(n_nodes);
        for (int f = 0; f < n_feat; ++f) {
            lba_epi_feat& F = feats[k * n_feat + f];
            F = lba_epi_feat{};
            F.angle = 360.0f * (float)(rnd() & 0xffff) / 65536.0f;
            F.has_point = rnd() % 7 != 0;
            for (uint32_t& d : F.desc) d = rnd() % 8 ? 0u : rnd() & 0x10101u;
            if (rnd() % 11) lists[rnd() % n_nodes].push_back(f);
        }
        ekfs[k] = lba_epi_kf{k * n_feat, n_feat, (int)node_id.size(), 0, (int)node_feat.size(), 0};
        int at = 0;
        for (int n = k; n < n_nodes; n += 1 + k) {
            node_id.push_back(3 * n);
            node_start.push_back(at);
            node_feat.insert(node_feat.end(), lists[n].begin(), lists[n].end());
            at += (int)lists[n].size();
            ++ekfs[k].n_node;
        }
        node_id.push_back(-1);
        node_start.push_back(at);
    }
    ekfs[2] = lba_epi_kf{0, 0, 0, 0, 0, 0};
    long sum = 0;
    std::vector<lba_bow_row> rows(n_feat);
    const float ratios[] = {0.9f, 0.6f, 0.8f, 1.5f};
    for (int variant = 0; variant < 16; ++variant) {
        const lba_bow_params prm{variant & 1, variant == 15 ? 0 : (variant == 14 ? 255 : 50), ratios[(variant >> 1) & 3], (variant >> 3) & 1};
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                sum += bow_search_host(ekfs[a], ekfs[b], feats.data(), node_id.data(), node_start.data(), node_feat.data(),
                                       prm, rows.data());
    }
    sum += bow_search_host(ekfs[0], ekfs[1], feats.data(), node_id.data(), node_start.data(), node_feat.data(),
                           bow_params_or_default(nullptr), rows.data());
    std::printf("clean: %ld matches over the variants\n", sum);
    return sum > 0 ? 0 : 1;
}
#endif
