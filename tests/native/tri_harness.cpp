// Host build of the product's CreateNewMapPoints maths (lba_tri_math.hpp: tri_null4, tri_triangulate, the gates,
// tri_row), put together as k_triangulate does, for tests/test_tri_math_host.py and scripts/triangulate_margins.py.
#include "../../amc-slam_amd/csrc/lba_tri_math.hpp"

using namespace lba;

extern "C" int tri_sweeps(void) { return TRI_SWEEPS; }

// A [16] row-major; v [4]: the null vector after `sweeps` sweeps (2 .. 10), *sigma the norm of its A-column
extern "C" int tri_null(const double* A, int sweeps, double* v, double* sigma) {
    switch (sweeps) {
        case 2: tri_null4_sweeps<2>(A, v, sigma); return 0;
        case 3: tri_null4_sweeps<3>(A, v, sigma); return 0;
        case 4: tri_null4_sweeps<4>(A, v, sigma); return 0;
        case 5: tri_null4_sweeps<5>(A, v, sigma); return 0;
        case 6: tri_null4_sweeps<6>(A, v, sigma); return 0;
        case 7: tri_null4_sweeps<7>(A, v, sigma); return 0;
        case 8: tri_null4_sweeps<8>(A, v, sigma); return 0;
        case 9: tri_null4_sweeps<9>(A, v, sigma); return 0;
        case 10: tri_null4_sweeps<10>(A, v, sigma); return 0;
    }
    return -1;
}

extern "C" void tri_A(const double* xn1, const double* T1, const double* xn2, const double* T2, double* A) {
    tri_build_A(xn1, T1, xn2, T2, A);
}

extern "C" int tri_point(const double* xn1, const double* T1, const double* xn2, const double* T2, double* X) {
    return tri_triangulate(xn1, T1, xn2, T2, X) ? 1 : 0;
}

extern "C" double tri_cos(double b, double depth) { return tri_cos_stereo(b, depth); }

extern "C" int tri_unproject(const double* k, double z, const lba_tri_cam* last, const lba_tri_kf* kf, double* X) {
    return tri_unproject_stereo(k, z, *last, *kf, X) ? 1 : 0;
}

extern "C" int tri_reproj(const lba_tri_cam* c, double bf, const double* xyz, const double* kp, double ur, double sigma2) {
    return tri_reproj_fails(*c, bf, xyz[0], xyz[1], xyz[2], kp, ur, sigma2) ? 1 : 0;
}

// every row of every pair as lba_triangulate does it, on the host (no argument checks): rows in place
extern "C" void tri_rows_host(const lba_tri_pair* pairs, int n_pairs, lba_tri_row* rows, const lba_tri_kf* kfs,
                              const lba_tri_cam* cams, int n_cam, double ratio_factor, int far_points, double th_far) {
    for (int p = 0; p < n_pairs; ++p) {
        const lba_tri_kf& k1 = kfs[pairs[p].kf1];
        const lba_tri_kf& k2 = kfs[pairs[p].kf2];
        for (int i = pairs[p].row0; i < pairs[p].row0 + pairs[p].n_rows; ++i) {
            lba_tri_row& r = rows[i];
            TriRow in;
            for (int j = 0; j < 2; ++j) { in.z1[j] = r.z1[j]; in.z2[j] = r.z2[j]; in.k1[j] = r.k1[j]; in.k2[j] = r.k2[j]; }
            in.ur1 = r.ur1; in.ur2 = r.ur2; in.depth1 = r.depth1; in.depth2 = r.depth2;
            in.sigma2_1 = r.sigma2_1; in.sigma2_2 = r.sigma2_2; in.scale1 = r.scale1; in.scale2 = r.scale2;
            double X[3];
            r.status = tri_row(in, cams[k1.cam0 + r.cam1], cams[k2.cam0 + r.cam2], cams[k1.cam0 + n_cam - 1],
                               cams[k2.cam0 + n_cam - 1], k1, k2, ratio_factor, far_points, th_far, &r.stereo_point, X);
            if (r.status == LBA_TRI_OK) { r.X[0] = X[0]; r.X[1] = X[1]; r.X[2] = X[2]; }
        }
    }
}
