// lba_lm.hpp — what the tracker's four optimisers share (k_track, k_vel_hyp, k_sim3's lm_round, the host loop of
// lba_posegraph_optimize): g2o's Levenberg controller and the small register Cholesky.  DESIGN.md §7 item 8.
//
// The controller is OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-194) plus the stop
// rule of SparseOptimizer::optimize.  (lm_round restates lm_trial and lm_stop in place, for a reason given there: a
// change to the rule goes there too.)  A caller keeps what is its own: how it gets tempChi and scale, what accepting a
// trial does to its state, its lambda at the first iteration, its statistics and its barriers.  Its loop reads
//
//     LmCtl c;
//     for (k < iterations) {
//         currentChi = iniChi = chi2 and the system at the state;
//         if (k == 0) c = LmCtl{tau max|H_ii| or the caller's lambda, 2.0, 0};
//         do { solve, trial state, tempChi, scale;
//              rho = lm_trial(c, currentChi, tempChi, scale, accept);  if (accept) the trial state becomes current;
//              qmax++;
//         } while (rho < 0 && qmax < max_trials);
//         if (lm_stop(c, iniChi, currentChi, rho, qmax, max_trials) && early_stop) break;
//     }
//
// No fp-contract pragma here: the device callers compile with contraction, the host caller without, and each keeps
// its bits.  (The main solver's lm_decide, lba_kernels.hip, runs with contraction off on both sides and is separate
// for that reason.)
#pragma once

#include "lba_math.hpp"

namespace lba {

struct LmCtl {
    double lambda, ni;
    int nbad;   // consecutive iterations whose gain stayed below 1e-3 of the iteration's first chi2
};

// One trial of an iteration: rho = (currentChi - tempChi) / scale.  A trial with rho > 0 and a finite tempChi is
// accepted: lambda shrinks by 1 - (2 rho - 1)^3 held to [1/3, 2/3], ni goes back to 2 and tempChi becomes currentChi.
// Any other (a failed solve comes as tempChi = DBL_MAX, a NaN fails both tests) is refused: lambda *= ni, ni *= 2.
LBA_HD double lm_trial(LmCtl& c, double& currentChi, double tempChi, double scale, bool& accept) {
    const double rho = (currentChi - tempChi) / scale;
    accept = rho > 0 && isfinite(tempChi);
    if (accept) {
        const double t = 2 * rho - 1;
        double alpha = 1. - t * t * t;
        alpha = fmin(alpha, 2. / 3.);
        c.lambda *= fmax(1. / 3., alpha);
        c.ni = 2;
        currentChi = tempChi;
    } else {
        c.lambda *= c.ni;
        c.ni *= 2;
    }
    return rho;
}

// After an iteration's trials (qmax of them, the last with gain ratio rho): stop if the trials ran out, if rho is
// exactly 0, or at the third iteration in a row that gained less than 1e-3 of its first chi2.
LBA_HD bool lm_stop(LmCtl& c, double iniChi, double currentChi, double rho, int qmax, int max_trials) {
    bool stop = qmax == max_trials || rho == 0;
    if (!stop) {
        if ((iniChi - currentChi) * 1e3 < iniChi) c.nbad++;
        else c.nbad = 0;
        stop = c.nbad >= 3;
    }
    return stop;
}

// (H + lambda I) x = b, H the packed upper triangle of an N x N matrix: unpivoted Cholesky, fully unrolled so that it
// lives in registers and is the same on every lane of a wave; 1 if every pivot is positive, else x is not to be used.
template <int N>
LBA_HD int chol_solve(const double* H, double lambda, const double* b, double* x) {
    double L[N][N];
    int ok = 1;
#pragma unroll
    for (int i = 0, q = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j, ++q) L[j][i] = H[q] + (i == j ? lambda : 0.0);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double d = L[k][k];
#pragma unroll
        for (int p = 0; p < k; ++p) d -= L[k][p] * L[k][p];
        ok &= d > 0.0 ? 1 : 0;   // (a NaN pivot fails too; what follows it is never used)
        const double r = sqrt(d);
        L[k][k] = r;
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            double s = L[i][k];
#pragma unroll
            for (int p = 0; p < k; ++p) s -= L[i][p] * L[k][p];
            L[i][k] = s / r;
        }
    }
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = b[i];
#pragma unroll
        for (int p = 0; p < i; ++p) s -= L[i][p] * y[p];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int p = i + 1; p < N; ++p) s -= L[p][i] * x[p];
        x[i] = s / L[i][i];
    }
    return ok;
}

}  // namespace lba
