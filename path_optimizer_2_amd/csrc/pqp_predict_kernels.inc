// pqp_predict_kernels.inc — instantiated by pqp_agents.hip; includes pqp_driven_path.hpp, pqp_free_motion.hpp (the four CTRA functions) and pqp_line_device.hpp.  Tracked agents to predicted rows (pqp_predict_agents):
// a pose, a speed, an acceleration, a yaw rate and a size per track become the [step][PQP_AGENT_STRIDE] rows pqp_agents_check,
// pqp_speed_search and the fine check behind pqp_sample_plan read, on the layers' times (r = 1) or on r sub-steps per layer, under
// pqp_sample_plan's time expression.  The reference has no counterpart: it plans against a static map.  include/pqp.h states the
// definition operation by operation.
//
// predict_agents_kernel: one wavefront per (scene, agent), four per workgroup, no LDS, no scratch, no atomics.
//   1  the track row, the slot's count and the lane's view are read wave-uniform; an absent or bad track fills its rows and is done
//   2  a track with a lane is anchored once: spline_projection_wave (pqp_line_device.hpp, the wavefront's 64 lanes share its coarse scan),
//      then the lane's point and heading at s0 and the offset l0 as project_points_kernel takes them.  The lane's table stays where it
//      lies (HBM through L2), so there is no knot cap
//   3  tiles of 64 steps, one step per lane: the lane forms its time, the distance driven under the capped constant acceleration, and
//      its pose - the closed CTRA form, or pqp_offsets_to_points' expression at (s0 + dir D, l0) - and writes its row of six doubles;
//      a wavefront's 64 rows are one contiguous 3 KB.  The flags are ballots carried over the tiles; lane 0 writes them and the anchor.
// A (scene, agent)'s result depends on its track, its lane and the parameters alone.

#include "pqp_driven_path.hpp"
#include "pqp_free_motion.hpp"
#include "pqp_line_device.hpp"

namespace pqp {

constexpr int kPredictThreads = 256;
constexpr long long kPredictMaxBlocks = 1ll << 22;      // beyond that many workgroups a wavefront takes several (scene, agent) slots in turn
// a lane of 2^20 m and more is not projected on, as pqp_project_points refuses it: the coarse scan has floor(length) + 1 steps
constexpr double kPredictMaxLength = 1048576.0;

struct PredictArgs {
    int n_scenes, a_max, m, r, n_lanes, lane_m;
    double t0, dt, v_cap, grow, l_max;
    const double* tracks;            // [n_scenes][a_max][PQP_TRACK_STRIDE]
    const int32_t* a_of;             // [n_scenes] or nullptr: all a_max
    const int32_t* lane_of;          // [n_scenes][a_max] or nullptr: the free model
    const double* lane_spl;          // [n_lanes][9][lane_m]
    const double* lane_ext;          // [n_lanes][4]
    const double* lane_len;          // [n_lanes]
    double* agents;                  // [n_scenes][a_max][M][PQP_AGENT_STRIDE], M = (m - 1) r + 1
    double* anchor;                  // [n_scenes][a_max][PQP_ANCHOR_STRIDE] or nullptr
    int32_t* flags;                  // [n_scenes][a_max]
};

// one (scene, agent) slot, by a whole wavefront
__device__ __forceinline__ void predict_slot(const PredictArgs& a, long long item, int lane) {
#pragma clang fp contract(off)
    const int scene = (int)(item / a.a_max), ag = (int)(item - (long long)scene * a.a_max);
    const int M = (a.m - 1) * a.r + 1;
    const double* __restrict__ tr = a.tracks + (size_t)item * PQP_TRACK_STRIDE;
    double* __restrict__ rows = a.agents + (size_t)item * M * PQP_AGENT_STRIDE;
    double* anchor = a.anchor ? a.anchor + (size_t)item * PQP_ANCHOR_STRIDE : nullptr;

    // ---- 1: absent, bad -----------------------------------------------------------------------------------------------------------------
    bool absent = ag >= clamped_count(a.a_of, scene, a.a_max);
    double x0 = 0.0, y0 = 0.0, h0 = 0.0, v = 0.0, acc = 0.0, om = 0.0, hl = -1.0, hw = -1.0, radius = 0.0;
    if (!absent) {
        hl = tr[6]; hw = tr[7];
        absent = hl < 0.0 || hw < 0.0;
    }
    bool bad = false;
    if (!absent) {
        x0 = tr[0]; y0 = tr[1]; h0 = tr[2]; v = tr[3]; acc = tr[4]; om = tr[5]; radius = tr[8];
        bad = !(isfinite(x0) && isfinite(y0) && isfinite(h0) && isfinite(v) && isfinite(acc) && isfinite(om) && isfinite(hl) && isfinite(hw) &&
                isfinite(radius)) || v < 0.0 || radius < 0.0;
    }
    if (absent || bad) {
        const double pose = bad ? NAN : 0.0, sl = bad ? hl : -1.0, sw = bad ? hw : -1.0, sr = bad ? radius : 0.0;
        for (int f = lane; f < M; f += 64) {
            double* o = rows + (size_t)f * PQP_AGENT_STRIDE;
            o[0] = pose; o[1] = pose; o[2] = pose; o[3] = sl; o[4] = sw; o[5] = sr;
        }
        if (lane == 0) {
            a.flags[item] = bad ? PQP_PREDICT_BAD : PQP_PREDICT_ABSENT;
            if (anchor) { anchor[0] = 0.0; anchor[1] = 0.0; anchor[2] = 0.0; anchor[3] = 0.0; }
        }
        return;
    }

    // ---- 2: the lane's anchor ------------------------------------------------------------------------------------------------------------
    int flags = 0;
    const int want = a.lane_of ? a.lane_of[item] : -1;
    if (want >= a.n_lanes) flags |= PQP_PREDICT_LANE_FAR;
    const bool has_lane = want >= 0 && want < a.n_lanes;
    const int n = a.lane_m;
    const double* tab = a.lane_spl + (size_t)(has_lane ? want : 0) * 9 * n;
    SplineView sx{tab, tab + n, tab + 2 * n, tab + 3 * n, tab + 4 * n, 0.0, 0.0, n};
    SplineView sy{tab, tab + 5 * n, tab + 6 * n, tab + 7 * n, tab + 8 * n, 0.0, 0.0, n};
    double s0 = 0.0, l0 = 0.0, dir = 0.0, dh = 0.0, length = 0.0;
    bool on_lane = false;
    if (has_lane) {
        const double* ext = a.lane_ext + (size_t)want * 4;
        sx.b0 = ext[0]; sx.c0 = ext[1]; sy.b0 = ext[2]; sy.c0 = ext[3];
        length = a.lane_len[want];
        if (length > 0.0 && length < kPredictMaxLength) {
            s0 = spline_projection_wave(sx, sy, x0, y0, length);
            double xp, dx, ddx, yp, dy, ddy;
            spline_eval3(sx, s0, xp, dx, ddx); spline_eval3(sy, s0, yp, dy, ddy);
            const double hp = atan2(dy, dx);                                   // getHeading
            const double ch = cos(hp), sh = sin(hp);
            const double ex = x0 - xp, ey = y0 - yp;                           // global2Local((x_p, y_p, heading_p), point)
            l0 = -ex * sh + ey * ch;
            dh = constrain_angle(h0 - hp);
            on_lane = isfinite(l0) && fabs(l0) <= a.l_max;
            if (on_lane) dir = cos(h0 - hp) >= 0.0 ? 1.0 : -1.0;
        }
        flags |= on_lane ? PQP_PREDICT_ON_LANE : PQP_PREDICT_LANE_FAR;
    }

    // ---- 3: the steps --------------------------------------------------------------------------------------------------------------------
    const int r = a.r;
    const double dt = a.dt, rr = (double)r, v_cap = a.v_cap;
    double sh0 = 0.0, ch0 = 1.0;
    if (!on_lane) sincos(h0, &sh0, &ch0);
    bool stops = false, capped = false, off = false;
    for (int f0 = 0; f0 < M; f0 += 64) {
        const int f = f0 + lane;
        if (f < M) {
            const int k = f / r, i = f - k * r;
            const double tau = a.t0 + ((double)k * dt + ((double)i * dt) / rr);
            // the speed along the motion: acc acts for te seconds, then the speed is ve
            double te, ve;
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
            const double tc = tau - te;
            double px, py, ph;
            if (on_lane) {
                const double D = (v + (0.5 * acc) * te) * te + ve * tc;
                const double sf = s0 + dir * D;
                double fx, dx, ddx, fy, dy, ddy;
                spline_eval3(sx, sf, fx, dx, ddx);
                spline_eval3(sy, sf, fy, dy, ddy);
                const double way = atan2(dy, dx);
                px = fx + l0 * cos(way + kPi2);
                py = fy + l0 * sin(way + kPi2);
                ph = dir < 0.0 ? constrain_angle(way + kPi) : way;
                off = off || sf < 0.0 || sf > length;
            } else {
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
            double* o = rows + (size_t)f * PQP_AGENT_STRIDE;
            o[0] = px; o[1] = py; o[2] = ph; o[3] = hl; o[4] = hw; o[5] = radius + a.grow * tau;
        }
    }
    if (__ballot(stops)) flags |= PQP_PREDICT_STOPS;
    if (__ballot(capped)) flags |= PQP_PREDICT_CAPPED;
    if (__ballot(off)) flags |= PQP_PREDICT_OFF_LANE;
    if (lane == 0) {
        a.flags[item] = flags;
        if (anchor) { anchor[0] = s0; anchor[1] = l0; anchor[2] = dir; anchor[3] = dh; }
    }
}

__global__ void __launch_bounds__(kPredictThreads) predict_agents_kernel(const PredictArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long total = (long long)a.n_scenes * a.a_max, step = (long long)gridDim.x * (kPredictThreads / 64);
    for (long long item = (long long)blockIdx.x * (kPredictThreads / 64) + wave; item < total; item += step) predict_slot(a, item, lane);
}

}  // namespace pqp
