// Host build of what the tracker's optimisers share (amc-slam_amd/csrc/lba_lm.hpp: lm_trial, lm_stop, chol_solve<N>),
// for tests/test_lm_host.py.  LmCtl crosses as the struct itself (double, double, int).
#include "../../amc-slam_amd/csrc/lba_lm.hpp"

using namespace lba;

extern "C" double lm_trial_c(LmCtl* c, double* currentChi, double tempChi, double scale, int* accept) {
    bool a = false;
    const double rho = lm_trial(*c, *currentChi, tempChi, scale, a);
    *accept = a ? 1 : 0;
    return rho;
}

extern "C" int lm_stop_c(LmCtl* c, double iniChi, double currentChi, double rho, int qmax, int max_trials) {
    return lm_stop(*c, iniChi, currentChi, rho, qmax, max_trials) ? 1 : 0;
}

// H: the packed upper triangle (21 or 28 doubles)
extern "C" int chol_solve6(const double* H, double lambda, const double* b, double* x) { return chol_solve<6>(H, lambda, b, x); }
extern "C" int chol_solve7(const double* H, double lambda, const double* b, double* x) { return chol_solve<7>(H, lambda, b, x); }
