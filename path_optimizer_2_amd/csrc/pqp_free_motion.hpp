// pqp_free_motion.hpp - the free model of a tracked state, shared by predict_agents_kernel (pqp_predict_kernels.inc, pqp_agents.hip) and
// stitch_trajectory_kernel (pqp_stitch_kernels.inc, pqp_select.hip), each .inc including it for itself: the speed under a constant
// acceleration that ends at a stop or at a cap, and the pose under constant turn rate and acceleration in closed form.  include/pqp.h
// states every operation below once, under pqp_predict_agents.  Device code only.  Every function is forced inline and keeps fp
// contraction off: a fused multiply-add here breaks bit equality with the definition.
// Both kernels take ctra_functions from here.  free_speed and free_pose are stitch_trajectory_kernel's alone: predict_slot keeps the
// same two texts in its step loop, because calling them from there moved its register allocation (189 -> 191 VGPRs), and that kernel's
// code is pinned instruction for instruction.  A change to the model is made in both places; tests/predict_util.py restates it once and
// both kernels are held to that.
#pragma once
#include "pqp_driven_path.hpp"

namespace pqp {

constexpr double kPredictSmallAngle = 0x1p-6;           // below it the four CTRA functions are their Taylor polynomials

// sinc, cosc, f1, f2 of include/pqp.h at one angle: sin th / th, 2 sin^2(th / 2) / th, (th sin th - 2 sin^2(th / 2)) / th^2 and
// (sin th - th cos th) / th^2, or their Taylor polynomials through th^5 below kPredictSmallAngle
__device__ __forceinline__ void ctra_functions(double th, double& sinc, double& cosc, double& f1, double& f2) {
#pragma clang fp contract(off)
    const double t2 = th * th;
    if (fabs(th) < kPredictSmallAngle) {
        sinc = 1.0 - t2 * (1.0 / 6.0 - t2 * (1.0 / 120.0));
        cosc = th * (0.5 - t2 * (1.0 / 24.0 - t2 * (1.0 / 720.0)));
        f1 = 0.5 - t2 * (1.0 / 8.0 - t2 * (1.0 / 144.0));
        f2 = th * (1.0 / 3.0 - t2 * (1.0 / 30.0 - t2 * (1.0 / 840.0)));
    } else {
        double sn, cs;
        sincos(th, &sn, &cs);
        const double sh = sin(0.5 * th);
        const double hv = 2.0 * (sh * sh);
        sinc = sn / th;
        cosc = hv / th;
        f1 = (th * sn - hv) / t2;
        f2 = (sn - th * cs) / t2;
    }
}

// the speed along the motion at time tau: acc acts for te seconds, then the speed is ve.  stops / capped are set - never cleared - when
// the stop or the cap is reached at tau, so a caller may carry them over its steps
__device__ __forceinline__ void free_speed(double v, double acc, double v_cap, double tau, double& te, double& ve, bool& stops, bool& capped) {
#pragma clang fp contract(off)
    if (acc < 0.0) {
        const double ts = v / (-acc);
        const bool done = tau >= ts;
        te = fmin(tau, ts);
        ve = done ? 0.0 : v + acc * te;
        stops = stops || done;
    } else if (acc > 0.0) {
        if (v >= v_cap) {
            te = 0.0; ve = v; capped = true;
        } else {
            const double tcap = (v_cap - v) / acc;
            const bool done = tau >= tcap;
            te = fmin(tau, tcap);
            ve = done ? v_cap : v + acc * te;
            capped = capped || done;
        }
    } else if (v == 0.0) {
        te = 0.0; ve = 0.0; stops = true;                               // stands from the start
    } else {
        te = tau; ve = v;
    }
}

// the pose after te seconds of (v, acc, om) from (x0, y0, h0) and tc seconds at ve behind them; sh0, ch0 = sincos(h0), which a caller
// with many steps takes once
__device__ __forceinline__ void free_pose(double x0, double y0, double h0, double sh0, double ch0, double v, double acc, double om, double te,
                                          double ve, double tc, double& px, double& py, double& ph) {
#pragma clang fp contract(off)
    const double th = om * te;
    double sinc, cosc, f1, f2;
    ctra_functions(th, sinc, cosc, f1, f2);
    const double vt = v * te, at2 = acc * (te * te);
    const double p = vt * sinc + at2 * f1, q = vt * cosc + at2 * f2;
    const double h1 = h0 + th;
    const double th2 = ve > 0.0 ? om * tc : 0.0;
    double sinc2, cosc2, g1, g2;
    ctra_functions(th2, sinc2, cosc2, g1, g2);
    const double vt2 = ve * tc;
    const double p2 = vt2 * sinc2, q2 = vt2 * cosc2;
    double sh1, ch1;
    sincos(h1, &sh1, &ch1);
    px = (x0 + (p * ch0 - q * sh0)) + (p2 * ch1 - q2 * sh1);
    py = (y0 + (p * sh0 + q * ch0)) + (p2 * sh1 + q2 * ch1);
    ph = constrain_angle(h1 + th2);
}

}  // namespace pqp
