// Host build of the pose graph's maths (lba_pg_math.hpp: sim3_log, sim3_Ad, sim3_left_jac, sim3_pg_edge), put together
// as k_pg_edges does, for tests/test_posegraph_math_host.py.
#include "../../amc-slam_amd/csrc/lba_pg_math.hpp"

using namespace lba;

namespace {
Sim3 load(const double* s) {   // q[4] (x, y, z, w), t[3], s
    Sim3 S;
    S.q = qnormalize(Quat{s[0], s[1], s[2], s[3]});
    S.t[0] = s[4]; S.t[1] = s[5]; S.t[2] = s[6];
    S.s = s[7];
    return S;
}
}  // namespace

extern "C" void pg_log(const double* S, double* e) { sim3_log(load(S), e); }

// e = log(Sim3(update))
extern "C" void pg_log_exp(const double* update, double* e) { sim3_log(sim3_exp(update), e); }

extern "C" void pg_Ad(const double* S, double* A) { sim3_Ad(load(S), A); }

extern "C" void pg_left_jac(const double* e, double* J) { sim3_left_jac(e, J); }

// e[7] and J0, J1 (7 x 7 row-major) of one edge
extern "C" void pg_edge(const double* C, const double* S0, const double* S1, int fix_scale, double* e, double* J0, double* J1) {
    sim3_pg_edge(load(C), load(S0), load(S1), fix_scale != 0, e, J0, J1);
}
