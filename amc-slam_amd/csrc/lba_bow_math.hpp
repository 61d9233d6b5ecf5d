// lba_bow_math.hpp — ORBmatcher::SearchByBoW, both overloads: (pKF1, pKF2, vpMatches12) of loop closing
// (src/ORBmatcher.cc:805-945, LBA_BOW_KF) and (pKF, F, vpMapPointMatches) of TrackReferenceKeyFrame (:227-421,
// LBA_BOW_FRAME).  One candidate of the inner loop (bow_fold), the merge of two partial scans (bow_merge), the accept
// test (bow_accept), the rotation pass, and the whole sequential function of one pair (bow_search_host).  The distance,
// the rotation bin and ComputeThreeMaxima are lba_match_math.hpp's.
//
// LBA_HD like lba_math.hpp, so tests/test_bow_host.py runs the code k_bow_match runs.  Everything is integer work
// except the ratio test, two int -> float converts and one float product, written as the reference writes it and with
// contraction off; the device is held to IDENTICAL results.
//
// Why a scan may be split (what k_bow_match relies on).  After the inner loop over the eligible candidates of a node,
//   bestDist1 = min(256, smallest distance), bestDist2 = min(256, second smallest of the MULTISET of distances):
//     a distance enters bestDist2 either when it is displaced from bestDist1 or by the `else if`; a value equal to
//     bestDist1 fails `<` and takes the `else if`, so equal values count twice;
//   bestIdx2 = the FIRST list position that attains bestDist1, `<` being strict; -1 when bestDist1 == 256, since a
//     distance of 256 passes neither comparison.
// Both are functions of the multiset of (distance, position) alone, so any split of the candidates into parts, each
// scanned in ascending position, merges exactly: the best is the smaller key (distance, position), the second the
// smallest of the loser's best and the two seconds.  bow_merge is commutative and associative.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_match_math.hpp"
#include "lba_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace lba {

constexpr int BOW_NONE = 256;          // bestDist1 / bestDist2 before the first candidate
constexpr int BOW_NO_POS = 0xffff;     // the position of "no candidate" in a key: above every list position

// the scan's state: bestDist1, the list position of bestIdx2 (BOW_NO_POS: none), bestDist2
struct BowBest {
    int b1 = BOW_NONE, pos1 = BOW_NO_POS, b2 = BOW_NONE;
};

// (distance, position) as one ordered word: the smaller key is the better candidate, ties to the first position
LBA_HD int bow_key(int dist, int pos) { return (dist << 16) | pos; }

// one candidate of the inner loop (:876-885 / :289-298); `pos` its position in side 2's list.  A part is scanned in
// ascending position.
LBA_HD void bow_fold(BowBest& s, int dist, int pos) {
    if (dist < s.b1) {
        s.b2 = s.b1;
        s.b1 = dist;
        s.pos1 = pos;
    } else if (dist < s.b2) {
        s.b2 = dist;
    }
}

// two parts of one list, in any order
LBA_HD BowBest bow_merge(const BowBest& a, const BowBest& b) {
    const bool a_wins = bow_key(a.b1, a.pos1) <= bow_key(b.b1, b.pos1);
    const BowBest &w = a_wins ? a : b, &l = a_wins ? b : a;
    BowBest r;
    r.b1 = w.b1;
    r.pos1 = w.pos1;
    const int s = w.b2 < l.b2 ? w.b2 : l.b2;
    r.b2 = l.b1 < s ? l.b1 : s;
    return r;
}

// :888-890 / :331-333: LBA_BOW_OK, LBA_BOW_NO_CAND (the threshold) or LBA_BOW_RATIO
LBA_HD int bow_accept(int b1, int b2, int mode, int th_low, float nn_ratio) {
    if (!(mode == LBA_BOW_FRAME ? b1 <= th_low : b1 < th_low)) return LBA_BOW_NO_CAND;
    const float rhs = nn_ratio * static_cast<float>(b2);
    return static_cast<float>(b1) < rhs ? LBA_BOW_OK : LBA_BOW_RATIO;
}

// ---------------------------------------------------------------------------------------------------- host only

inline lba_bow_params bow_params_or_default(const lba_bow_params* prm) {
    return prm ? *prm : lba_bow_params{LBA_BOW_KF, 50, 0.9f, 1};
}

// a row that ran no inner loop
inline lba_bow_row bow_blank_row(int status) { return lba_bow_row{-1, BOW_NONE, BOW_NONE, status}; }

// nmatches and, with check_orientation, the rotation pass (:895-905 and :924-942; :339-352 and :400-418) of one pair
// on its decided rows: the matches of the bins that are NOT one of the three maxima are removed (the ordinary rule;
// SearchForTriangulation's is the opposite).  f1 / f2: the two sides' own features; rows [n1].
inline int bow_finish(const lba_epi_feat* f1, int n1, const lba_epi_feat* f2, int check_orientation, lba_bow_row* rows) {
    int n = 0;
    for (int i = 0; i < n1; ++i) n += rows[i].status == LBA_BOW_OK;
    if (check_orientation) {
        int histo[MATCH_HISTO] = {};
        for (int i = 0; i < n1; ++i)
            if (rows[i].status == LBA_BOW_OK) ++histo[match_rot_bin(f1[i].angle, f2[rows[i].idx2].angle)];
        int i1, i2, i3;
        match_three_maxima(histo, MATCH_HISTO, &i1, &i2, &i3);
        for (int i = 0; i < n1; ++i) {
            if (rows[i].status != LBA_BOW_OK) continue;
            const int bin = match_rot_bin(f1[i].angle, f2[rows[i].idx2].angle);
            if (bin == i1 || bin == i2 || bin == i3) continue;
            rows[i].status = LBA_BOW_ROT;
            --n;
        }
    }
    return n;
}

// The whole function for one pair as the reference's loops run it (no argument checks): rows [e1.n_feat]; returns
// nmatches.  Side 1 is e1 (the keyframe whose points are matched), side 2 is e2 (the other keyframe, or the frame).
inline int bow_search_host(const lba_epi_kf& e1, const lba_epi_kf& e2, const lba_epi_feat* feats, const int32_t* node_id,
                           const int32_t* node_start, const int32_t* node_feat, const lba_bow_params& prm,
                           lba_bow_row* rows) {
    const lba_epi_feat *f1 = feats + e1.feat0, *f2 = feats + e2.feat0;
    for (int i = 0; i < e1.n_feat; ++i) rows[i] = bow_blank_row(LBA_BOW_NO_NODE);
    std::vector<char> matched2((size_t)e2.n_feat, 0);   // vbMatched2, or vpMapPointMatches[idx] != NULL
    const int32_t *id1 = node_id + e1.node0, *id2 = node_id + e2.node0;
    const int32_t *s1 = node_start + e1.node0, *s2 = node_start + e2.node0;
    int a = 0, b = 0;
    while (a < e1.n_node && b < e2.n_node) {
        if (id1[a] == id2[b]) {
            for (int i1 = s1[a]; i1 < s1[a + 1]; ++i1) {
                const int idx1 = node_feat[e1.nf0 + i1];
                if (!f1[idx1].has_point) {
                    rows[idx1] = bow_blank_row(LBA_BOW_NO_POINT);
                    continue;
                }
                int bestDist1 = 256, bestIdx2 = -1, bestDist2 = 256;
                for (int i2 = s2[b]; i2 < s2[b + 1]; ++i2) {
                    const int idx2 = node_feat[e2.nf0 + i2];
                    if (matched2[idx2]) continue;
                    if (prm.mode == LBA_BOW_KF && !f2[idx2].has_point) continue;
                    const int dist = match_dist(f1[idx1].desc, f2[idx2].desc);
                    if (dist < bestDist1) {
                        bestDist2 = bestDist1;
                        bestDist1 = dist;
                        bestIdx2 = idx2;
                    } else if (dist < bestDist2) {
                        bestDist2 = dist;
                    }
                }
                const int status = bow_accept(bestDist1, bestDist2, prm.mode, prm.th_low, prm.nn_ratio);
                if (status == LBA_BOW_OK) matched2[bestIdx2] = 1;
                rows[idx1] = lba_bow_row{bestIdx2, bestDist1, bestDist2, status};
            }
            ++a;
            ++b;
        } else if (id1[a] < id2[b]) {
            while (a < e1.n_node && id1[a] < id2[b]) ++a;   // lower_bound on ascending ids
        } else {
            while (b < e2.n_node && id2[b] < id1[a]) ++b;
        }
    }
    return bow_finish(f1, e1.n_feat, f2, prm.check_orientation, rows);
}

}  // namespace lba
