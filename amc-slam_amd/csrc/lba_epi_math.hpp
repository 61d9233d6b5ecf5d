// lba_epi_math.hpp — ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:947-1131) with Pinhole::project and
// Pinhole::epipolarConstrain (src/CameraModels/Pinhole.cpp:43-49, 107-129): the table of one camera pair (F12 and the
// epipole), the two gates, the stereo rule, one candidate of the inner loop, and the whole sequential function of one
// pair.  The distance, the rotation bin and ComputeThreeMaxima are lba_match_math.hpp's.
//
// LBA_HD like lba_math.hpp, so tests/test_epi_host.py runs the code k_epi_tables and k_epi_match run.
// Precision: the tracker's convention, like lba_tri_math.hpp: fp64 on the float-valued inputs
// widened, in the reference's order, held against the restatement on settled jobs only.  NOT lba_match_math.hpp's
// float-bit convention: F12 goes through Eigen's float 3 x 3 inverse and three matrix products, whose operation order
// nobody can reproduce.  Contraction is off so that the host build and the device evaluate the same operations.
// Quirks of the reference, kept (include/amc_lba.h states them in full): (a) vbMatched2 is never set, no state passes
// between keypoints; (b) ties go to the LAST candidate that passes, `dist > bestDist` is the skip; (c) the rotation
// pass removes the bins that ARE the three maxima; (d) unc is KF2's level sigma2, 3.84 * unc a double product; (e) the
// epipole has no test on z and falls where IEEE puts it; (f) den == 0 fails the gate; (g) a node of one keyframe only
// contributes nothing.
#pragma once

#include <cstdint>

#include "../../include/amc_lba.h"
#include "lba_match_math.hpp"
#include "lba_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace lba {

constexpr int EPI_TAB = 11;   // doubles of one (c1, c2) table: F12 row-major [9], the epipole [2]

// C = A B, each sum in order
LBA_HD void epi_mul33(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// the table of KF1's camera c1 and KF2's camera c2 (:958-973 and Pinhole.cpp:109-112)
LBA_HD void epi_table(const lba_tri_cam& c1, const lba_tri_cam& c2, double* tab) {
    const double *T1 = c1.Tcw, *T2 = c2.Tcw;
    double R12[9], t12[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)   // R1 R2^T
            R12[3 * i + j] = (T1[4 * i] * T2[4 * j] + T1[4 * i + 1] * T2[4 * j + 1]) + T1[4 * i + 2] * T2[4 * j + 2];
        t12[i] = ((T1[4 * i] * c2.Ow[0] + T1[4 * i + 1] * c2.Ow[1]) + T1[4 * i + 2] * c2.Ow[2]) + T1[4 * i + 3];
    }
    const double tx[9] = {0.0, -t12[2], t12[1], t12[2], 0.0, -t12[0], -t12[1], t12[0], 0.0};
    const double K1it[9] = {1.0 / c1.fx, 0.0, 0.0, 0.0, 1.0 / c1.fy, 0.0, -c1.cx / c1.fx, -c1.cy / c1.fy, 1.0};
    const double K2i[9] = {1.0 / c2.fx, 0.0, -c2.cx / c2.fx, 0.0, 1.0 / c2.fy, -c2.cy / c2.fy, 0.0, 0.0, 1.0};
    double A[9], B[9];
    epi_mul33(K1it, tx, A);
    epi_mul33(A, R12, B);
    epi_mul33(B, K2i, tab);
    double C2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        C2[i] = ((T2[4 * i] * c1.Ow[0] + T2[4 * i + 1] * c1.Ow[1]) + T2[4 * i + 2] * c1.Ow[2]) + T2[4 * i + 3];
    tab[9] = c2.fx * C2[0] / C2[2] + c2.cx;
    tab[10] = c2.fy * C2[1] / C2[2] + c2.cy;
}

// bStereo (:1010, :1033): `>= 0`
LBA_HD bool epi_stereo(int cam, int n_cam, float u_right) { return cam == n_cam - 1 && u_right >= 0.0f; }

// the epipole test (:1049-1052): true when the candidate is skipped
LBA_HD bool epi_near_epipole(const double* tab, double x2, double y2, double scale2) {
    const double ex = tab[9] - x2, ey = tab[10] - y2;
    return ex * ex + ey * ey < 100.0 * scale2;
}

// Pinhole::epipolarConstrain (Pinhole.cpp:114-128): unc is the candidate's level sigma2
LBA_HD bool epi_gate(const double* F, double x1, double y1, double x2, double y2, double unc) {
    const double a = (x1 * F[0] + y1 * F[3]) + F[6];
    const double b = (x1 * F[1] + y1 * F[4]) + F[7];
    const double c = (x1 * F[2] + y1 * F[5]) + F[8];
    const double num = (a * x2 + b * y2) + c;
    const double den = a * a + b * b;
    if (den == 0.0) return false;
    const double dsqr = num * num / den;
    return dsqr < 3.84 * unc;
}

struct EpiBest {
    int dist, idx2;   // bestDist, bestIdx2
};

// one pass of the loop over KF2's node list (:1024-1062) for the keypoint f1 (stereo1: its bStereo1).  `tabs`: the
// pair's tables [n_cam][n_cam][EPI_TAB].
LBA_HD void epi_candidate(const lba_epi_feat& f1, bool stereo1, const lba_epi_feat& f2, int idx2, int n_cam,
                          int only_stereo, int coarse, int th_low, const double* tabs, EpiBest& best) {
    if (f2.has_point) return;
    const bool stereo2 = epi_stereo(f2.cam, n_cam, f2.u_right);
    if (only_stereo && !stereo2) return;
    const int dist = match_dist(f1.desc, f2.desc);
    if (dist > th_low || dist > best.dist) return;
    const double* tab = tabs + ((size_t)f1.cam * n_cam + f2.cam) * EPI_TAB;
    if (!stereo1 && !stereo2 && epi_near_epipole(tab, f2.x, f2.y, f2.scale)) return;
    if (coarse || epi_gate(tab, f1.x, f1.y, f2.x, f2.y, f2.sigma2)) {
        best.idx2 = idx2;
        best.dist = dist;
    }
}

// the status of a keypoint of KF1 before its candidates (:1005-1013); LBA_EPI_OK: it searches
LBA_HD int epi_entry_status(const lba_epi_feat& f1, bool stereo1, int only_stereo) {
    if (f1.has_point) return LBA_EPI_HAS_POINT;
    if (only_stereo && !stereo1) return LBA_EPI_NOT_STEREO;
    return LBA_EPI_OK;
}

// ---------------------------------------------------------------------------------------------------- host only

inline lba_epi_params epi_params_or_default(const lba_epi_params* prm) {
    return prm ? *prm : lba_epi_params{50, 0, 0, 0};
}

// nmatches and, with check_orientation, the rotation pass (:1071-1081, :1098-1117, quirk (c)) of one pair on its
// decided rows: f1 / f2 the two keyframes' own features, rows [n1]
inline int epi_finish(const lba_epi_feat* f1, int n1, const lba_epi_feat* f2, int check_orientation, lba_epi_row* rows) {
    int n = 0;
    for (int i = 0; i < n1; ++i) n += rows[i].status == LBA_EPI_OK;
    if (check_orientation) {
        int histo[MATCH_HISTO] = {};
        for (int i = 0; i < n1; ++i)
            if (rows[i].status == LBA_EPI_OK) ++histo[match_rot_bin(f1[i].angle, f2[rows[i].idx2].angle)];
        int i1, i2, i3;
        match_three_maxima(histo, MATCH_HISTO, &i1, &i2, &i3);
        for (int i = 0; i < n1; ++i) {
            if (rows[i].status != LBA_EPI_OK) continue;
            const int bin = match_rot_bin(f1[i].angle, f2[rows[i].idx2].angle);
            if (bin == i1 || bin == i2 || bin == i3) {
                rows[i].status = LBA_EPI_ROT;
                --n;
            }
        }
    }
    return n;
}

// first position in [lo, hi) of the ascending ids with ids[pos] >= key: FeatureVector::lower_bound
inline int epi_lower_bound(const int32_t* ids, int lo, int hi, int32_t key) {
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (ids[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The whole function for one pair as the reference's loops run it (no argument checks): rows [e1.n_feat]; returns
// nmatches.  cams1 / cams2: the n_cam camera records of either keyframe.
inline int epi_search_host(const lba_epi_kf& e1, const lba_epi_kf& e2, const lba_tri_cam* cams1, const lba_tri_cam* cams2,
                           int n_cam, const lba_epi_feat* feats, const int32_t* node_id, const int32_t* node_start,
                           const int32_t* node_feat, const lba_epi_params& prm, lba_epi_row* rows) {
    std::vector<double> tabs((size_t)n_cam * n_cam * EPI_TAB);
    for (int c1 = 0; c1 < n_cam; ++c1)
        for (int c2 = 0; c2 < n_cam; ++c2) epi_table(cams1[c1], cams2[c2], tabs.data() + ((size_t)c1 * n_cam + c2) * EPI_TAB);
    const lba_epi_feat *f1 = feats + e1.feat0, *f2 = feats + e2.feat0;
    for (int i = 0; i < e1.n_feat; ++i) rows[i] = lba_epi_row{-1, prm.th_low, LBA_EPI_NO_NODE, 0};
    const int32_t *id1 = node_id + e1.node0, *id2 = node_id + e2.node0;
    const int32_t *s1 = node_start + e1.node0, *s2 = node_start + e2.node0;
    int a = 0, b = 0;
    while (a < e1.n_node && b < e2.n_node) {
        if (id1[a] == id2[b]) {
            for (int i1 = s1[a]; i1 < s1[a + 1]; ++i1) {
                const int idx1 = node_feat[e1.nf0 + i1];
                const lba_epi_feat& k1 = f1[idx1];
                const bool stereo1 = epi_stereo(k1.cam, n_cam, k1.u_right);
                EpiBest best{prm.th_low, -1};
                int status = epi_entry_status(k1, stereo1, prm.only_stereo);
                if (status == LBA_EPI_OK) {
                    for (int i2 = s2[b]; i2 < s2[b + 1]; ++i2) {
                        const int idx2 = node_feat[e2.nf0 + i2];
                        epi_candidate(k1, stereo1, f2[idx2], idx2, n_cam, prm.only_stereo, prm.coarse, prm.th_low,
                                      tabs.data(), best);
                    }
                    status = best.idx2 >= 0 ? LBA_EPI_OK : LBA_EPI_NO_MATCH;
                }
                rows[idx1] = lba_epi_row{best.idx2, best.dist, status, 0};
            }
            ++a;
            ++b;
        } else if (id1[a] < id2[b]) {
            a = epi_lower_bound(id1, a, e1.n_node, id2[b]);
        } else {
            b = epi_lower_bound(id2, b, e2.n_node, id1[a]);
        }
    }
    return epi_finish(f1, e1.n_feat, f2, prm.check_orientation, rows);
}

}  // namespace lba
