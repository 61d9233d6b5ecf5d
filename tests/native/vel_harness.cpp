// Host build of the product's EdgeVelReproj maths (lba_math.hpp: vel_motion, vel_reproj_error, vel_reproj_jac), put
// together as k_vel_hyp does, for tests/test_vel_math_host.py.
#include "../../amc-slam_amd/csrc/lba_math.hpp"

using namespace lba;

// T = (q[4] (x, y, z, w), t[3]), cam = {Tbc q[4], t[3], fx, fy, cx, cy}: e[2], J[12] (2 x 6, row-major)
extern "C" void vel_edge(const double* q, const double* t, const double* cam, const double* v, double dt, const double* z,
                         const double* Xw, double* e, double* J) {
    SE3 T;
    T.q = qnormalize(Quat{q[0], q[1], q[2], q[3]});
    T.t[0] = t[0]; T.t[1] = t[1]; T.t[2] = t[2];
    const SE3 Ti = se3_inv(T);
    double Xb[3], Xc[3], Rp[9], tp[3];
    qrot(Ti.q, Xw, Xb);
    Xb[0] += Ti.t[0]; Xb[1] += Ti.t[1]; Xb[2] += Ti.t[2];
    Cam c;
    for (int i = 0; i < 4; ++i) c.q[i] = cam[i];
    for (int i = 0; i < 3; ++i) c.t[i] = cam[4 + i];
    c.fx = cam[7]; c.fy = cam[8]; c.cx = cam[9]; c.cy = cam[10];
    CamD cd;
    cam_derive(c, &cd);
    vel_motion(v, dt, Rp, tp);
    vel_reproj_error(Rp, tp, cd, Xb, z, Xc, e);
    vel_reproj_jac(v, dt, Rp, cd, Xb, Xc, J);
}
