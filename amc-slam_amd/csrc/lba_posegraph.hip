// lba_posegraph.hip — the optimisation of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1434-1717): a Sim3 pose
// graph of VertexSim3Expmap / EdgeSim3 under g2o's Levenberg, solved by a sparse tile Cholesky of the full system
// (BlockSolver_7_3 over LinearSolverEigen in the reference: no vertex is marginalised).
//
// Everything is fp64.  An active free vertex takes 8 rows: its 7 dofs and an inert eighth (unit diagonal, zero right
// hand side), so a 32-row panel holds four vertices in array order; the last panel is filled up with inert vertices.
// lba_plan::make_plan orders the panels (nested dissection, leaf 2 so that small graphs dissect) and gives the tiles
// of L with their fill-in.  The host then builds, once per call:
//   - the block jobs: one per 8 x 8 block of the system that has terms, with its gather list (edge, which of J0 / J1
//     on either side) in edge order, and its place in the tiles of L;
//   - the columns by level: level(j) = 1 + the highest level of a column k < j with L(j, k) != 0, so a level's columns
//     need finished columns of lower levels only; per tile (i, j) the pairs (L(i, k), L(j, k)) of its update.
// Per LM trial, on the tracker's stream (plain launches; the order of the launches is the only ordering there is:
// no kernel here waits on another workgroup, there is no flag, ticket or atomic):
//   k_pg_edges<true>   one thread per active edge: e = log(C S0 S1^-1), J0, J1 (lba_pg_math.hpp), chi2_e   [once per
//                      iteration: the trials of an iteration share it]
//   k_pg_assemble      one wave per block job: sum J^T J in list order (+ lambda on the diagonal) into the tile of L,
//                      and -J^T e into b for a diagonal job; the tiles are zeroed before (fill-in, blocks without terms)
//   k_pg_column        per level, one workgroup of four waves per column j, left-looking: D = A(j,j) - sum_k L(j,k)
//                      L(j,k)^T on v_mfma_f64_16x16x4_f64 (a 16 x 16 quadrant per wave), its Cholesky factor and
//                      inverse in LDS, y_j = L_jj^-1 (b_j - sum_k L(j,k) y_k) (the forward substitution rides along:
//                      it has the column's dependencies), then every L(i,j) = (A(i,j) - sum_k L(i,k) L(j,k)^T) L_jj^-T
//   k_pg_back          per level downwards, one wave per column: x_j = L_jj^-T (y_j - sum_i L(i,j)^T x_i)
//   k_pg_update        one thread per vertex: S <- Sim3(dx) S into the trial buffer
//   k_pg_edges<false>  the trial's errors, then k_pg_reduce (one workgroup, fixed order): chi2, x.(lambda x + b), and
//                      the factorisation's failure word
// and one readback of three doubles, on which the host takes g2o's accept / reject decision (a deliberate limit: a
// call costs a few tens of readbacks).  A non-positive pivot makes the trial one with chi2 = DBL_MAX, k_track's rule.
// Every sum has a fixed order, so results are bitwise reproducible.  The controller of that decision is lba_lm.hpp's,
// the arena and the error path lba_tracker.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/amc_lba.h"
#include "lba_lm.hpp"
#include "lba_pg_math.hpp"
#include "lba_plan.hpp"
#include "lba_tracker.hpp"

using namespace lba;

namespace {

constexpr int PG_NB = 32;              // rows of a panel
constexpr int PG_VB = 8;               // rows of a vertex
constexpr int PG_TILE = PG_NB * PG_NB;
constexpr int PG_MAX_V = 1 << 20;
constexpr int PG_MAX_E = 1 << 22;
constexpr int PG_MAX_DENSE = 2048;     // lba_posegraph_linearize: active free vertices of a dense H
constexpr size_t PG_MAX_BYTES = size_t(6) << 30;
constexpr int PG_JOB_DIAG = 1, PG_JOB_PAD = 2;

typedef double pg_d4 __attribute__((ext_vector_type(4)));   // v_mfma_f64_16x16x4 accumulator

struct PgDev {
    // the graph
    const lba_pg_edge* edges;   // the active edges, in edge order
    int ne, nv, NP, fix_scale;
    const int *voff, *vslot;    // per vertex: offset of its rows in the position-ordered vectors / its slot, or -1
    // block jobs
    const int *job_ptr, *job_flag, *job_tile, *job_off, *contrib;
    // the factorisation's lists
    const int *lvl_cols, *diag_tile, *rk_ptr, *rk_tile, *rk_col, *cr_ptr, *cr_tile, *cr_row, *pr_ptr, *pr_a, *pr_b;
    // work
    double *err, *J, *chi, *tiles, *dinv, *b, *hdiag, *y, *x, *dxnat, *out;
    int* fail;
};

template <bool JAC>
__global__ __launch_bounds__(64) void k_pg_edges(PgDev D, const double* __restrict__ S) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= D.ne) return;
    const lba_pg_edge E = D.edges[i];
    Sim3 C, S0, S1;
    C.q = qnormalize(Quat{E.q[0], E.q[1], E.q[2], E.q[3]});
    C.t[0] = E.t[0]; C.t[1] = E.t[1]; C.t[2] = E.t[2];
    C.s = E.s;
    const double* a = S + (size_t)E.v0 * 8;
    const double* b = S + (size_t)E.v1 * 8;
    S0.q = Quat{a[0], a[1], a[2], a[3]}; S0.t[0] = a[4]; S0.t[1] = a[5]; S0.t[2] = a[6]; S0.s = a[7];
    S1.q = Quat{b[0], b[1], b[2], b[3]}; S1.t[0] = b[4]; S1.t[1] = b[5]; S1.t[2] = b[6]; S1.s = b[7];
    double e[7];
    if (JAC) {
        double J0[49], J1[49];
        sim3_pg_edge(C, S0, S1, D.fix_scale != 0, e, J0, J1);
        double* o = D.J + (size_t)i * 98;
        for (int k = 0; k < 49; ++k) { o[k] = J0[k]; o[49 + k] = J1[k]; }
    } else {
        sim3_pg_edge(C, S0, S1, D.fix_scale != 0, e, nullptr, nullptr);
    }
    double c = 0.0;
    for (int k = 0; k < 7; ++k) {
        if (JAC) D.err[(size_t)i * 7 + k] = e[k];   // (a trial's errors are not kept: b of the next trial reads these)
        c += e[k] * e[k];
    }
    D.chi[i] = c;
}

// one wave per block job; thread (r, c) of the 8 x 8 block
__global__ __launch_bounds__(64) void k_pg_assemble(PgDev D, double lambda) {
    const int job = blockIdx.x, r = threadIdx.x >> 3, c = threadIdx.x & 7;
    if (job == 0 && threadIdx.x == 0) *D.fail = 0;
    const int flags = D.job_flag[job];
    const bool diag = flags & PG_JOB_DIAG, pad = flags & PG_JOB_PAD;
    const int r0 = (flags >> 8) & 31, c0 = (flags >> 16) & 31;
    const int p0 = D.job_ptr[job], p1 = D.job_ptr[job + 1];
    double v = 0.0;
    if (r < 7 && c < 7)
        for (int p = p0; p < p1; ++p) {
            const int code = D.contrib[p];
            const double* Jl = D.J + (size_t)(code >> 2) * 98 + ((code >> 1) & 1) * 49;
            const double* Jr = D.J + (size_t)(code >> 2) * 98 + (code & 1) * 49;
            double t = 0.0;
            for (int k = 0; k < 7; ++k) t += Jl[k * 7 + r] * Jr[k * 7 + c];
            v += t;
        }
    if (diag && r == c) {
        if (r < 7 && !pad) {
            D.hdiag[D.job_off[job] + r] = v;
            v += lambda;
        } else {
            v = 1.0;   // the inert dofs
        }
    }
    D.tiles[(size_t)D.job_tile[job] * PG_TILE + (r0 + r) * PG_NB + c0 + c] = v;
    if (diag && c == 7) {
        double bb = 0.0;
        if (r < 7 && !pad)
            for (int p = p0; p < p1; ++p) {
                const int code = D.contrib[p];
                const double* Js = D.J + (size_t)(code >> 2) * 98 + (code & 1) * 49;
                const double* e = D.err + (size_t)(code >> 2) * 7;
                double t = 0.0;
                for (int k = 0; k < 7; ++k) t += Js[k * 7 + r] * e[k];
                bb -= t;
            }
        D.b[D.job_off[job] + r] = bb;
    }
}

__device__ __forceinline__ void pg_load_tile(double (*X)[PG_NB + 1], const double* __restrict__ g, int tid) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = tid + 256 * q;
        X[idx >> 5][idx & 31] = g[idx];
    }
}

// acc (this wave's quadrant) += X[rows of rb] Y[rows of cb]^T, K = 32; lane (lr, kq) holds row kq + 4 q, column lr
__device__ __forceinline__ pg_d4 pg_mma_nt(const double (*X)[PG_NB + 1], const double (*Y)[PG_NB + 1], int rb, int cb, int lr,
                                           int kq, pg_d4 acc) {
#pragma unroll
    for (int k0 = 0; k0 < PG_NB; k0 += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[rb * 16 + lr][k0 + kq], Y[cb * 16 + lr][k0 + kq], acc, 0, 0, 0);
    return acc;
}

__global__ __launch_bounds__(256) void k_pg_column(PgDev D, int col0) {
    __shared__ double Xs[PG_NB][PG_NB + 1], Ys[PG_NB][PG_NB + 1], Ds[PG_NB][PG_NB + 1], Is[PG_NB][PG_NB + 1];
    __shared__ double vs[PG_NB];
    __shared__ int s_bad;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 15, kq = lane >> 4, rb = wave >> 1, cb = wave & 1;
    const int j = D.lvl_cols[col0 + blockIdx.x];
    if (tid == 0) s_bad = 0;
    // ---- the diagonal tile and the right hand side
    pg_d4 acc = {0.0, 0.0, 0.0, 0.0};
    double yb = tid < PG_NB ? D.b[j * PG_NB + tid] : 0.0;
    for (int p = D.rk_ptr[j]; p < D.rk_ptr[j + 1]; ++p) {
        pg_load_tile(Xs, D.tiles + (size_t)D.rk_tile[p] * PG_TILE, tid);
        if (tid < PG_NB) vs[tid] = D.y[D.rk_col[p] * PG_NB + tid];
        __syncthreads();
        acc = pg_mma_nt(Xs, Xs, rb, cb, lr, kq, acc);
        if (tid < PG_NB)
            for (int c = 0; c < PG_NB; ++c) yb -= Xs[tid][c] * vs[c];
        __syncthreads();
    }
    double* Dg = D.tiles + (size_t)D.diag_tile[j] * PG_TILE;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = 16 * rb + kq + 4 * q, col = 16 * cb + lr;
        Ds[row][col] = Dg[row * PG_NB + col] - acc[q];
    }
    __syncthreads();
    // ---- Cholesky of Ds (lower triangle), right-looking
    for (int k = 0; k < PG_NB; ++k) {
        const double piv = Ds[k][k];
        if (tid == 0 && !(piv > 0.0)) s_bad = 1;
        const double rt = sqrt(piv);
        __syncthreads();
        if (tid < PG_NB && tid >= k) Ds[tid][k] = tid == k ? rt : Ds[tid][k] / rt;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q, i = idx >> 5, c = idx & 31;
            if (c > k && i >= c) Ds[i][c] -= Ds[i][k] * Ds[c][k];
        }
        __syncthreads();
    }
    // ---- L_jj^-1 (thread c: its column c), zeros above the diagonal of both
    if (tid < PG_NB) {
        const int c = tid;
        for (int r = 0; r < c; ++r) { Is[r][c] = 0.0; Ds[r][c] = 0.0; }
        Is[c][c] = 1.0 / Ds[c][c];
        for (int r = c + 1; r < PG_NB; ++r) {
            double s = 0.0;
            for (int p = c; p < r; ++p) s += Ds[r][p] * Is[p][c];
            Is[r][c] = -s / Ds[r][r];
        }
        vs[tid] = yb;
    }
    __syncthreads();
    double* Ig = D.dinv + (size_t)j * PG_TILE;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = tid + 256 * q;
        Dg[idx] = Ds[idx >> 5][idx & 31];
        Ig[idx] = Is[idx >> 5][idx & 31];
    }
    if (tid < PG_NB) {
        double s = 0.0;
        for (int c = 0; c <= tid; ++c) s += Is[tid][c] * vs[c];
        D.y[j * PG_NB + tid] = s;
    }
    if (tid == 0 && s_bad) *D.fail = 1;   // (every writer of a launch writes the same value)
    // ---- the tiles below: L(i, j) = (A(i, j) - sum_k L(i, k) L(j, k)^T) L_jj^-T
    for (int t = D.cr_ptr[j]; t < D.cr_ptr[j + 1]; ++t) {
        acc = pg_d4{0.0, 0.0, 0.0, 0.0};
        for (int p = D.pr_ptr[t]; p < D.pr_ptr[t + 1]; ++p) {
            __syncthreads();
            pg_load_tile(Xs, D.tiles + (size_t)D.pr_a[p] * PG_TILE, tid);
            pg_load_tile(Ys, D.tiles + (size_t)D.pr_b[p] * PG_TILE, tid);
            __syncthreads();
            acc = pg_mma_nt(Xs, Ys, rb, cb, lr, kq, acc);
        }
        double* Tg = D.tiles + (size_t)D.cr_tile[t] * PG_TILE;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = 16 * rb + kq + 4 * q, col = 16 * cb + lr;
            Xs[row][col] = Tg[row * PG_NB + col] - acc[q];
        }
        __syncthreads();
        acc = pg_mma_nt(Xs, Is, rb, cb, lr, kq, pg_d4{0.0, 0.0, 0.0, 0.0});
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = 16 * rb + kq + 4 * q, col = 16 * cb + lr;
            Tg[row * PG_NB + col] = acc[q];
        }
    }
}

__global__ __launch_bounds__(64) void k_pg_back(PgDev D, int col0) {
    __shared__ double vs[PG_NB];
    const int t = threadIdx.x;
    const int j = D.lvl_cols[col0 + blockIdx.x];
    if (t < PG_NB) {
        double v = D.y[j * PG_NB + t];
        for (int p = D.cr_ptr[j]; p < D.cr_ptr[j + 1]; ++p) {
            const double* L = D.tiles + (size_t)D.cr_tile[p] * PG_TILE;
            const double* xi = D.x + D.cr_row[p] * PG_NB;
            for (int r = 0; r < PG_NB; ++r) v -= L[r * PG_NB + t] * xi[r];
        }
        vs[t] = v;
    }
    __syncthreads();
    if (t < PG_NB) {
        const double* Li = D.dinv + (size_t)j * PG_TILE;
        double s = 0.0;
        for (int r = t; r < PG_NB; ++r) s += Li[r * PG_NB + t] * vs[r];
        D.x[j * PG_NB + t] = s;
    }
}

__global__ __launch_bounds__(64) void k_pg_update(PgDev D, const double* __restrict__ S, double* __restrict__ T) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= D.nv) return;
    const double* a = S + (size_t)v * 8;
    double* o = T + (size_t)v * 8;
    const int off = D.voff[v];
    if (off < 0) {
        for (int k = 0; k < 8; ++k) o[k] = a[k];
        return;
    }
    double dx[7];
    for (int k = 0; k < 7; ++k) dx[k] = D.x[off + k];
    if (D.fix_scale) dx[6] = 0.0;   // oplusImpl (types_seven_dof_expmap.h:80-86)
    Sim3 X;
    X.q = Quat{a[0], a[1], a[2], a[3]}; X.t[0] = a[4]; X.t[1] = a[5]; X.t[2] = a[6]; X.s = a[7];
    const Sim3 N = sim3_mul(sim3_exp(dx), X);
    o[0] = N.q.x; o[1] = N.q.y; o[2] = N.q.z; o[3] = N.q.w;
    o[4] = N.t[0]; o[5] = N.t[1]; o[6] = N.t[2]; o[7] = N.s;
    double* d = D.dxnat + (size_t)D.vslot[v] * 7;
    for (int k = 0; k < 7; ++k) d[k] = dx[k];
}

// out = {sum of the edges' chi2, x.(lambda x + b) if with_x, the failure word}: strided partial sums, then a tree
__global__ __launch_bounds__(256) void k_pg_reduce(PgDev D, double lambda, int with_x) {
    __shared__ double sa[256], sb[256];
    const int tid = threadIdx.x;
    double a = 0.0, s = 0.0;
    for (int i = tid; i < D.ne; i += 256) a += D.chi[i];
    if (with_x)
        for (int i = tid; i < D.NP * PG_NB; i += 256) {
            const double xi = D.x[i];
            s += xi * (lambda * xi + D.b[i]);
        }
    sa[tid] = a; sb[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { sa[tid] += sa[tid + o]; sb[tid] += sb[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        D.out[0] = sa[0];
        D.out[1] = sb[0];
        D.out[2] = (double)*D.fail;
    }
}

// ---------------------------------------------------------------------------------------------- host: the plan
struct PgJob { int row_slot, col_slot, tile, r0, c0, flags, off; };

struct PgHost {
    int n_v = 0, n_e = 0, na = 0, NP = 0, nlevel = 0, fill_tiles = 0;
    std::vector<int> eact, slot, slot_v, voff;
    lba_plan::Plan pl;
    std::vector<int> lvl_ptr, lvl_cols, diag_tile, rk_ptr, rk_tile, rk_col, cr_ptr, cr_tile, cr_row, pr_ptr, pr_a, pr_b;
    std::vector<PgJob> jobs;
    std::vector<int> job_ptr, contrib;
};

int pg_check(const lba_pg_vertex* v, int n_v, const lba_pg_edge* e, int n_e) {
    if (!v || n_v < 1 || n_e < 0 || (n_e && !e)) return LBA_E_ARG;
    if (n_v > PG_MAX_V || n_e > PG_MAX_E) return LBA_E_LIMIT;
    for (int i = 0; i < n_v; ++i)
        if (!std::isfinite(v[i].s) || !(v[i].s > 0)) return LBA_E_ARG;
    for (int k = 0; k < n_e; ++k) {
        const lba_pg_edge& E = e[k];
        if (E.v0 < 0 || E.v0 >= n_v || E.v1 < 0 || E.v1 >= n_v || E.v0 == E.v1) return LBA_E_ARG;
        if (!std::isfinite(E.s) || !(E.s > 0)) return LBA_E_ARG;
    }
    return LBA_OK;
}

// activity, slots, the panel plan; with `lists` also the jobs and the factorisation's lists
int pg_plan(const lba_pg_vertex* v, int n_v, const lba_pg_edge* e, int n_e, bool lists, PgHost& G) {
    const int rc = pg_check(v, n_v, e, n_e);
    if (rc != LBA_OK) return rc;
    G.n_v = n_v; G.n_e = n_e;
    std::vector<char> touched(n_v, 0);
    for (int k = 0; k < n_e; ++k) {
        if (v[e[k].v0].fixed && v[e[k].v1].fixed) continue;
        G.eact.push_back(k);
        touched[e[k].v0] = 1; touched[e[k].v1] = 1;
    }
    if (G.eact.empty()) return LBA_E_EMPTY;
    G.slot.assign(n_v, -1);
    for (int i = 0; i < n_v; ++i)
        if (touched[i] && !v[i].fixed) { G.slot[i] = (int)G.slot_v.size(); G.slot_v.push_back(i); }
    G.na = (int)G.slot_v.size();   // (> 0: an active edge has a free vertex)
    const int NP = G.NP = (G.na + 3) / 4;
    std::vector<std::vector<int>> lower(NP);
    for (int k : G.eact) {
        const int s0 = G.slot[e[k].v0], s1 = G.slot[e[k].v1];
        if (s0 < 0 || s1 < 0) continue;
        const int P = std::max(s0, s1) / 4, Q = std::min(s0, s1) / 4;
        if (P != Q) lower[P].push_back(Q);
    }
    for (auto& l : lower) {
        std::sort(l.begin(), l.end());
        l.erase(std::unique(l.begin(), l.end()), l.end());
    }
    G.pl = lba_plan::make_plan(NP, NP, lower, 64, true, 2, 0);
    const lba_plan::Plan& pl = G.pl;
    // levels
    std::vector<int> level(NP, 0);
    int nlevel = 0;
    for (int j = 0; j < NP; ++j) {
        int l = 0;
        for (int q = pl.rowptr[j]; q < pl.rowptr[j + 1] - 1; ++q) l = std::max(l, level[pl.cols[q]] + 1);
        level[j] = l;
        nlevel = std::max(nlevel, l + 1);
    }
    G.nlevel = nlevel;
    // tiles of the pattern of the system (the others are fill-in)
    std::vector<char> in_s(pl.ntile(), 0);
    for (int P = 0; P < NP; ++P) {
        in_s[pl.tile_id(pl.ppos[P], pl.ppos[P])] = 1;
        for (int Q : lower[P]) {
            const int i = std::max(pl.ppos[P], pl.ppos[Q]), j = std::min(pl.ppos[P], pl.ppos[Q]);
            in_s[pl.tile_id(i, j)] = 1;
        }
    }
    G.fill_tiles = (int)std::count(in_s.begin(), in_s.end(), 0);
    if (!lists) return LBA_OK;
    G.lvl_ptr.assign(nlevel + 1, 0);
    for (int j = 0; j < NP; ++j) ++G.lvl_ptr[level[j] + 1];
    for (int l = 0; l < nlevel; ++l) G.lvl_ptr[l + 1] += G.lvl_ptr[l];
    G.lvl_cols.resize(NP);
    {
        std::vector<int> fill(G.lvl_ptr.begin(), G.lvl_ptr.end() - 1);
        for (int j = 0; j < NP; ++j) G.lvl_cols[fill[level[j]]++] = j;
    }
    G.diag_tile.resize(NP);
    G.rk_ptr.assign(1, 0);
    G.cr_ptr.assign(1, 0);
    G.pr_ptr.assign(1, 0);
    for (int j = 0; j < NP; ++j) {
        G.diag_tile[j] = pl.rowptr[j + 1] - 1;
        for (int q = pl.rowptr[j]; q < pl.rowptr[j + 1] - 1; ++q) {
            G.rk_tile.push_back(q);
            G.rk_col.push_back(pl.cols[q]);
        }
        G.rk_ptr.push_back((int)G.rk_tile.size());
        for (int i : pl.colrows[j]) {
            G.cr_tile.push_back(pl.tile_id(i, j));
            G.cr_row.push_back(i);
            for (int q = pl.rowptr[j]; q < pl.rowptr[j + 1] - 1; ++q) {
                const int tik = pl.tile_id(i, pl.cols[q]);
                if (tik >= 0) { G.pr_a.push_back(tik); G.pr_b.push_back(q); }
            }
            G.pr_ptr.push_back((int)G.pr_a.size());
        }
        G.cr_ptr.push_back((int)G.cr_tile.size());
    }
    // per vertex: where its rows are in the position-ordered vectors
    G.voff.assign(n_v, -1);
    auto off_of = [&](int s) { return pl.ppos[s / 4] * PG_NB + (s % 4) * PG_VB; };
    for (int s = 0; s < G.na; ++s) G.voff[G.slot_v[s]] = off_of(s);
    // block jobs: key (row slot, column slot), the row's panel not before the column's; gather lists in edge order
    std::map<std::pair<int, int>, std::vector<int>> terms;
    for (int s = 0; s < 4 * NP; ++s) terms[{s, s}];
    for (int a = 0; a < (int)G.eact.size(); ++a) {
        const lba_pg_edge& E = e[G.eact[a]];
        const int s[2] = {G.slot[E.v0], G.slot[E.v1]};
        for (int l = 0; l < 2; ++l)
            for (int r = 0; r < 2; ++r) {
                if (s[l] < 0 || s[r] < 0) continue;
                if (pl.ppos[s[l] / 4] < pl.ppos[s[r] / 4]) continue;   // the upper triangle of tiles is not stored
                terms[{s[l], s[r]}].push_back(a * 4 + l * 2 + r);
            }
    }
    G.job_ptr.assign(1, 0);
    for (const auto& kv : terms) {
        PgJob jb;
        jb.row_slot = kv.first.first; jb.col_slot = kv.first.second;
        jb.tile = pl.tile_id(pl.ppos[jb.row_slot / 4], pl.ppos[jb.col_slot / 4]);
        if (jb.tile < 0) return LBA_E_ARG;   // (never: the plan's pattern covers every coupled pair of panels)
        jb.r0 = (jb.row_slot % 4) * PG_VB; jb.c0 = (jb.col_slot % 4) * PG_VB;
        jb.flags = (jb.row_slot == jb.col_slot ? PG_JOB_DIAG : 0) | (jb.row_slot >= G.na ? PG_JOB_PAD : 0);
        jb.off = jb.row_slot == jb.col_slot ? off_of(jb.row_slot) : 0;
        G.jobs.push_back(jb);
        G.contrib.insert(G.contrib.end(), kv.second.begin(), kv.second.end());
        G.job_ptr.push_back((int)G.contrib.size());
    }
    return LBA_OK;
}

// ---------------------------------------------------------------------------------------------- host: the device
struct PgRun {
    lba_tracker* t = nullptr;
    PgDev D{};
    double *S = nullptr, *T = nullptr;   // current and trial states [n_v][8]
    std::vector<double> h_state;
    int njobs = 0, nlevel = 0;
    const PgHost* G = nullptr;
};

void pg_pack_state(const lba_pg_vertex* v, int n_v, std::vector<double>& o) {
    o.resize((size_t)n_v * 8);
    for (int i = 0; i < n_v; ++i) {
        const Quat q = qnormalize(Quat{v[i].q[0], v[i].q[1], v[i].q[2], v[i].q[3]});
        double* d = &o[(size_t)i * 8];
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
        d[4] = v[i].t[0]; d[5] = v[i].t[1]; d[6] = v[i].t[2]; d[7] = v[i].s;
    }
}

// lay the arena out, grow it, upload the graph and the lists (one copy); throws TrackerError (HIP, the size limit)
void pg_upload(lba_tracker* t, const lba_pg_vertex* v, const lba_pg_edge* e, int fix_scale, const PgHost& G, PgRun& R) {
    const int ne = (int)G.eact.size(), NP = G.NP, nt = G.pl.ntile();
    ArenaImage in;
    ArenaLayout& A = in.lay;
    std::vector<lba_pg_edge> ed(ne);
    for (int a = 0; a < ne; ++a) ed[a] = e[G.eact[a]];
    std::vector<int> jflag, jtile, joff;
    for (const PgJob& j : G.jobs) {
        jflag.push_back(j.flags | (j.r0 << 8) | (j.c0 << 16));
        jtile.push_back(j.tile);
        joff.push_back(j.off);
    }
    pg_pack_state(v, G.n_v, R.h_state);
    const Sec<lba_pg_edge> o_ed = in.put(ed);
    const Sec<double> o_S = in.put(R.h_state);
    const Sec<int> o_voff = in.put(G.voff), o_vslot = in.put(G.slot);
    const Sec<int> o_jptr = in.put(G.job_ptr), o_jflag = in.put(jflag), o_jtile = in.put(jtile), o_joff = in.put(joff);
    const Sec<int> o_con = in.put(G.contrib);
    const Sec<int> o_lvl = in.put(G.lvl_cols), o_dt = in.put(G.diag_tile), o_rkp = in.put(G.rk_ptr), o_rkt = in.put(G.rk_tile);
    const Sec<int> o_rkc = in.put(G.rk_col), o_crp = in.put(G.cr_ptr), o_crt = in.put(G.cr_tile), o_crr = in.put(G.cr_row);
    const Sec<int> o_prp = in.put(G.pr_ptr), o_pra = in.put(G.pr_a), o_prb = in.put(G.pr_b);
    const size_t up = A.total;
    const Sec<double> o_T = A.take<double>((size_t)G.n_v * 8);
    const Sec<double> o_err = A.take<double>((size_t)ne * 7), o_J = A.take<double>((size_t)ne * 98);
    const Sec<double> o_chi = A.take<double>((size_t)ne);
    const Sec<double> o_tiles = A.take<double>((size_t)nt * PG_TILE);
    const Sec<double> o_dinv = A.take<double>((size_t)NP * PG_TILE);
    const size_t vec = (size_t)NP * PG_NB;
    const Sec<double> o_b = A.take<double>(vec), o_hd = A.take<double>(vec), o_y = A.take<double>(vec), o_x = A.take<double>(vec);
    const Sec<double> o_dx = A.take<double>((size_t)G.na * 7);
    const Sec<double> o_out = A.take<double>(4);
    const Sec<int> o_fail = A.take<int>(1);
    if (A.total > PG_MAX_BYTES) throw TrackerError{LBA_E_LIMIT, "the pose graph's factor exceeds 6 GB of device memory"};
    TR_HIP(hipSetDevice(t->cfg.device));
    grow_bytes(t->d_arena, t->arena_cap, A.total, A.total + A.total / 2);
    char* d = t->d_arena;
    TR_HIP(hipMemcpyAsync(d, in.bytes.data(), up, hipMemcpyHostToDevice, t->stream));
    TR_HIP(hipStreamSynchronize(t->stream));   // (the image is pageable and goes out of scope)
    PgDev& D = R.D;
    D.edges = o_ed.at(d);
    D.ne = ne; D.nv = G.n_v; D.NP = NP; D.fix_scale = fix_scale != 0;
    D.voff = o_voff.at(d); D.vslot = o_vslot.at(d);
    D.job_ptr = o_jptr.at(d); D.job_flag = o_jflag.at(d); D.job_tile = o_jtile.at(d); D.job_off = o_joff.at(d);
    D.contrib = o_con.at(d);
    D.lvl_cols = o_lvl.at(d); D.diag_tile = o_dt.at(d); D.rk_ptr = o_rkp.at(d); D.rk_tile = o_rkt.at(d); D.rk_col = o_rkc.at(d);
    D.cr_ptr = o_crp.at(d); D.cr_tile = o_crt.at(d); D.cr_row = o_crr.at(d);
    D.pr_ptr = o_prp.at(d); D.pr_a = o_pra.at(d); D.pr_b = o_prb.at(d);
    D.err = o_err.at(d); D.J = o_J.at(d); D.chi = o_chi.at(d); D.tiles = o_tiles.at(d); D.dinv = o_dinv.at(d);
    D.b = o_b.at(d); D.hdiag = o_hd.at(d); D.y = o_y.at(d); D.x = o_x.at(d); D.dxnat = o_dx.at(d); D.out = o_out.at(d);
    D.fail = o_fail.at(d);
    R.t = t; R.S = o_S.at(d); R.T = o_T.at(d);
    R.njobs = (int)G.jobs.size(); R.nlevel = G.nlevel; R.G = &G;
}

void pg_launch_check() { TR_HIP(hipGetLastError()); }

void pg_edges(const PgRun& R, const double* S, bool jac) {
    const dim3 g((unsigned)((R.D.ne + 63) / 64)), b(64);
    if (jac) hipLaunchKernelGGL(k_pg_edges<true>, g, b, 0, R.t->stream, R.D, S);
    else hipLaunchKernelGGL(k_pg_edges<false>, g, b, 0, R.t->stream, R.D, S);
    pg_launch_check();
}

void pg_assemble(const PgRun& R, double lambda) {
    hipStream_t s = R.t->stream;
    TR_HIP(hipMemsetAsync(R.D.tiles, 0, (size_t)R.G->pl.ntile() * PG_TILE * sizeof(double), s));
    hipLaunchKernelGGL(k_pg_assemble, dim3((unsigned)R.njobs), dim3(64), 0, s, R.D, lambda);
    pg_launch_check();
}

// (H + lambda I) x = b from the edges' Jacobians of the last k_pg_edges<true>
void pg_solve(const PgRun& R, double lambda) {
    hipStream_t s = R.t->stream;
    pg_assemble(R, lambda);
    const PgHost& G = *R.G;
    for (int l = 0; l < G.nlevel; ++l) {
        hipLaunchKernelGGL(k_pg_column, dim3((unsigned)(G.lvl_ptr[l + 1] - G.lvl_ptr[l])), dim3(256), 0, s, R.D, G.lvl_ptr[l]);
        pg_launch_check();
    }
    for (int l = G.nlevel - 1; l >= 0; --l) {
        hipLaunchKernelGGL(k_pg_back, dim3((unsigned)(G.lvl_ptr[l + 1] - G.lvl_ptr[l])), dim3(64), 0, s, R.D, G.lvl_ptr[l]);
        pg_launch_check();
    }
}

// the trial state S (+) x into T, its errors; out = {chi2 of T, x.(lambda x + b), failure}
void pg_trial(const PgRun& R, double lambda, double* out3) {
    hipStream_t s = R.t->stream;
    hipLaunchKernelGGL(k_pg_update, dim3((unsigned)((R.D.nv + 63) / 64)), dim3(64), 0, s, R.D, (const double*)R.S, R.T);
    pg_launch_check();
    pg_edges(R, R.T, false);
    hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(256), 0, s, R.D, lambda, 1);
    pg_launch_check();
    TR_HIP(hipMemcpyAsync(out3, R.D.out, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    TR_HIP(hipStreamSynchronize(s));
}

double pg_ms(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

void pg_unpack(const double* st, lba_pg_vertex& o) {
    std::memcpy(o.q, st, 4 * sizeof(double));
    std::memcpy(o.t, st + 4, 3 * sizeof(double));
    o.s = st[7];
}

}  // namespace

extern "C" int lba_posegraph_plan_info(const lba_pg_vertex* v, int32_t n_v, const lba_pg_edge* e, int32_t n_e, int32_t info[8]) {
    if (!info) return LBA_E_ARG;
    PgHost G;
    const int rc = pg_plan(v, n_v, e, n_e, false, G);
    if (rc != LBA_OK) return rc;
    info[0] = G.na; info[1] = G.NP; info[2] = G.pl.ntile(); info[3] = G.fill_tiles;
    info[4] = G.nlevel; info[5] = G.pl.chain; info[6] = G.pl.tail; info[7] = G.pl.levels;
    return G.na;
}

extern "C" int lba_posegraph_profile(lba_tracker* t, double ms[3]) {
    if (!t || !ms) return LBA_E_ARG;
    for (int i = 0; i < 3; ++i) ms[i] = t->pg_ms[i];
    return LBA_OK;
}

extern "C" int lba_posegraph_linearize(lba_tracker* t, const lba_pg_vertex* v, int32_t n_v, const lba_pg_edge* e, int32_t n_e,
                                       int32_t fix_scale, double* errors, double* H, double* b) {
    if (!t) return LBA_E_ARG;
    PgHost G;
    const int rc = pg_plan(v, n_v, e, n_e, true, G);
    if (rc != LBA_OK) return rc;
    if (H && G.na > PG_MAX_DENSE)
        return tracker_fail(t, {LBA_E_LIMIT, "lba_posegraph_linearize: more than 2048 active free vertices for a dense H"});
    const int ne = (int)G.eact.size(), nt = G.pl.ntile();
    std::vector<double> h_err((size_t)ne * 7), h_tiles((size_t)nt * PG_TILE), h_b((size_t)G.NP * PG_NB);
    try {
        PgRun R;
        pg_upload(t, v, e, fix_scale, G, R);
        pg_edges(R, R.S, true);
        pg_assemble(R, 0.0);
        hipStream_t s = t->stream;
        TR_HIP(hipMemcpyAsync(h_err.data(), R.D.err, h_err.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        TR_HIP(hipMemcpyAsync(h_tiles.data(), R.D.tiles, h_tiles.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        TR_HIP(hipMemcpyAsync(h_b.data(), R.D.b, h_b.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        TR_HIP(hipStreamSynchronize(s));
    } catch (const TrackerError& err) {
        return tracker_fail(t, err);
    }
    if (errors) {
        std::memset(errors, 0, (size_t)n_e * 7 * sizeof(double));
        for (int a = 0; a < ne; ++a) std::memcpy(errors + (size_t)G.eact[a] * 7, &h_err[(size_t)a * 7], 7 * sizeof(double));
    }
    const size_t n = (size_t)G.na * 7;
    if (H) {
        std::memset(H, 0, n * n * sizeof(double));
        for (const PgJob& j : G.jobs) {
            if (j.flags & PG_JOB_PAD) continue;
            const double* T = &h_tiles[(size_t)j.tile * PG_TILE];
            for (int r = 0; r < 7; ++r)
                for (int c = 0; c < 7; ++c) {
                    const double x = T[(j.r0 + r) * PG_NB + j.c0 + c];
                    H[((size_t)j.row_slot * 7 + r) * n + (size_t)j.col_slot * 7 + c] = x;
                    H[((size_t)j.col_slot * 7 + c) * n + (size_t)j.row_slot * 7 + r] = x;
                }
        }
    }
    if (b)
        for (int s = 0; s < G.na; ++s) std::memcpy(b + (size_t)s * 7, &h_b[G.voff[G.slot_v[s]]], 7 * sizeof(double));
    return G.na;
}

extern "C" int lba_posegraph_step(lba_tracker* t, const lba_pg_vertex* v, int32_t n_v, const lba_pg_edge* e, int32_t n_e,
                                  int32_t fix_scale, double lambda, double* dx, lba_pg_vertex* trial, double* chi2_trial) {
    if (!t || !std::isfinite(lambda)) return LBA_E_ARG;
    PgHost G;
    const int rc = pg_plan(v, n_v, e, n_e, true, G);
    if (rc != LBA_OK) return rc;
    double out3[3] = {0, 0, 0};
    std::vector<double> h_dx((size_t)G.na * 7), h_T((size_t)n_v * 8);
    try {
        PgRun R;
        pg_upload(t, v, e, fix_scale, G, R);
        pg_edges(R, R.S, true);
        pg_solve(R, lambda);
        pg_trial(R, lambda, out3);
        if (out3[2] == 0.0) {
            hipStream_t s = t->stream;
            TR_HIP(hipMemcpyAsync(h_dx.data(), R.D.dxnat, h_dx.size() * sizeof(double), hipMemcpyDeviceToHost, s));
            TR_HIP(hipMemcpyAsync(h_T.data(), R.T, h_T.size() * sizeof(double), hipMemcpyDeviceToHost, s));
            TR_HIP(hipStreamSynchronize(s));
        }
    } catch (const TrackerError& err) {
        return tracker_fail(t, err);
    }
    if (out3[2] != 0.0) return LBA_E_SOLVE;
    if (dx) std::memcpy(dx, h_dx.data(), h_dx.size() * sizeof(double));
    if (trial)
        for (int i = 0; i < n_v; ++i) {
            trial[i] = v[i];
            if (G.slot[i] >= 0) pg_unpack(&h_T[(size_t)i * 8], trial[i]);
        }
    if (chi2_trial) *chi2_trial = out3[0];
    return G.na;
}

extern "C" int lba_posegraph_optimize(lba_tracker* t, lba_pg_vertex* v, int32_t n_v, const lba_pg_edge* e, int32_t n_e,
                                      int32_t fix_scale, int32_t iterations, double lambda_init, lba_pg_stats* out) {
    if (!t || iterations < 0 || !std::isfinite(lambda_init)) return LBA_E_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    PgHost G;
    const int rc = pg_plan(v, n_v, e, n_e, true, G);
    if (rc != LBA_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    lba_pg_stats st;
    std::memset(&st, 0, sizeof(st));
    st.panels = G.NP; st.tiles = G.pl.ntile(); st.fill_tiles = G.fill_tiles; st.levels = G.nlevel; st.chain = G.pl.chain;
    st.launches_per_solve = 1 + 2 * G.nlevel;
    std::vector<double> h_S((size_t)n_v * 8);
    LmCtl lm{0.0, 2.0, 0};
    int iters = 0;
    try {
        PgRun R;
        pg_upload(t, v, e, fix_scale, G, R);
        const auto t2 = std::chrono::steady_clock::now();
        hipStream_t s = t->stream;
        const int max_trials = t->cfg.max_trials;
        double out3[3];
        for (int k = 0; k < iterations; ++k) {
            // computeActiveErrors + activeRobustChi2 + buildSystem at the estimate
            pg_edges(R, R.S, true);
            hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(256), 0, s, R.D, 0.0, 0);
            pg_launch_check();
            TR_HIP(hipMemcpyAsync(out3, R.D.out, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
            TR_HIP(hipStreamSynchronize(s));
            double currentChi = out3[0];
            const double iniChi = currentChi;
            if (k == 0) {
                st.chi2_initial = currentChi;
                double lambda = lambda_init;
                if (!(lambda_init > 0)) {   // computeLambdaInit: tau max|H_ii|
                    pg_assemble(R, 0.0);
                    std::vector<double> hd((size_t)G.NP * PG_NB);
                    TR_HIP(hipMemcpyAsync(hd.data(), R.D.hdiag, hd.size() * sizeof(double), hipMemcpyDeviceToHost, s));
                    TR_HIP(hipStreamSynchronize(s));
                    double m = 0.0;
                    for (int sl = 0; sl < G.na; ++sl)
                        for (int d = 0; d < 7; ++d) m = std::max(m, std::fabs(hd[G.voff[G.slot_v[sl]] + d]));
                    lambda = t->cfg.tau * m;
                }
                lm = LmCtl{lambda, 2.0, 0};
            }
            double rho = 0.0;
            int qmax = 0;
            do {
                pg_solve(R, lm.lambda);
                pg_trial(R, lm.lambda, out3);
                const bool ok = out3[2] == 0.0;
                const double tempChi = ok ? out3[0] : DBL_MAX;
                double scale = 1e-3;
                if (ok) scale += out3[1];
                else ++st.solve_failures;
                ++st.trials;
                bool accept;
                rho = lm_trial(lm, currentChi, tempChi, scale, accept);
                if (accept) std::swap(R.S, R.T);
                qmax++;
            } while (rho < 0 && qmax < max_trials);
            ++iters;
            st.chi2_final = currentChi;
            st.result = qmax == max_trials ? 1 : 0;
            if (lm_stop(lm, iniChi, currentChi, rho, qmax, max_trials) && t->cfg.early_stop) break;
        }
        if (iterations == 0) {
            pg_edges(R, R.S, false);
            hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(256), 0, s, R.D, 0.0, 0);
            pg_launch_check();
            TR_HIP(hipMemcpyAsync(out3, R.D.out, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
            TR_HIP(hipStreamSynchronize(s));
            st.chi2_initial = st.chi2_final = out3[0];
        }
        TR_HIP(hipMemcpyAsync(h_S.data(), R.S, h_S.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        TR_HIP(hipStreamSynchronize(s));
        const auto t3 = std::chrono::steady_clock::now();
        t->pg_ms[0] = pg_ms(t0, t1); t->pg_ms[1] = pg_ms(t1, t2); t->pg_ms[2] = pg_ms(t2, t3);
    } catch (const TrackerError& err) {
        return tracker_fail(t, err);
    }
    for (int i = 0; i < n_v; ++i)
        if (G.slot[i] >= 0) pg_unpack(&h_S[(size_t)i * 8], v[i]);
    st.iterations = iters;
    st.lambda_final = lm.lambda;
    if (out) *out = st;
    return iters;
}
