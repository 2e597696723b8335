// pqp_agent_frames.hpp - the agent frame row and what its readers share: agents_check_kernel (pqp_agents.hip), st_occupancy_kernel
// (pqp_speed.hip) and overlay_kernel (pqp_maps.hip).  A row is PQP_AGENT_FRAME_STRIDE doubles, written by agent_frames_kernel
// (pqp_agents_kernels.inc; launch_agent_frames of pqp_internal.hpp runs it for all three):
//   x, y, cos(heading), sin(heading), hl, hw, radius, reach
// reach = the circumradius of the rounded rectangle, whose sign and NaN also say "absent" and "bad".  include/pqp.h states every
// operation below once; this is the one place the kernels state them.  Device code only.  Every function is forced inline, and those
// that compute keep fp contraction off: a fused multiply-add here breaks bit equality with the definition.
#pragma once
#include "pqp_driven_path.hpp"

namespace pqp {

// the workgroup of the kernels that walk frame rows a wavefront per item: agent_frames_kernel, agents_check_kernel, st_occupancy_kernel
constexpr int kAgentsThreads = 256;

// d of include/pqp.h: the distance of the point (px, py) to the rounded rectangle of one frame row, negative inside it.  The one text of
// it: agent_clear below takes it for the car's circles, overlay_kernel (pqp_overlay_kernels.inc) for a cell's centre
__device__ __forceinline__ double agent_point_distance(double px, double py, double ax, double ay, double c, double sn, double hl, double hw,
                                                       double radius) {
#pragma clang fp contract(off)
    const double dx = px - ax, dy = py - ay;
    const double u = dx * c + dy * sn, w = dy * c - dx * sn;
    const double ex = fabs(u) - hl, ey = fabs(w) - hw;
    const double ox = fmax(ex, 0.0), oy = fmax(ey, 0.0);
    return sqrt(ox * ox + oy * oy) + fmin(fmax(ex, ey), 0.0) - radius;
}

// clear(k, a) of include/pqp.h: the six circles at (gx, gy) with radii cr against the rounded rectangle of one frame row; the test of
// agents_check_kernel and of st_occupancy_kernel (pqp_search_kernels.inc)
__device__ __forceinline__ double agent_clear(const double (&gx)[6], const double (&gy)[6], const double* cr, double ax, double ay, double c,
                                              double sn, double hl, double hw, double radius) {
#pragma clang fp contract(off)
    double c_ka = INFINITY;
#pragma unroll
    for (int j = 0; j < 6; ++j) c_ka = fmin(c_ka, agent_point_distance(gx[j], gy[j], ax, ay, c, sn, hl, hw, radius) - cr[j]);
    return c_ka;
}

// a frame row's reach, as agent_frames_kernel wrote it: negative - the agent is absent; NaN - its row is bad; else the circumradius
__device__ __forceinline__ bool agent_absent(double reach) { return reach < 0.0; }
__device__ __forceinline__ bool agent_bad(double reach) { return !(reach == reach); }

// the slack of the broad phase: 2^-10 m and 2^-30 of the coordinates' size, against a rounding of the exact test near 2^-50 of it
constexpr double kAgentsSlack = 0x1p-10, kAgentsSlackRel = 0x1p-30;

// the broad phase: the bounding circle's centre (bx, by) is so far from the agent's (ax, ay) that clear(k, a) >= margin + the slack.
// Leaving such an agent out changes no hit.
__device__ __forceinline__ bool agent_out_of_reach(double rb, double reach, double margin, double bx, double by, double ax, double ay) {
#pragma clang fp contract(off)
    const double ux = bx - ax, uy = by - ay;
    const double far = rb + reach + margin + kAgentsSlack + kAgentsSlackRel * (fabs(bx) + fabs(by) + fabs(ax) + fabs(ay));
    return ux * ux + uy * uy > far * far;
}

// the frames of path b's scene, and in *A how many of its a_max agents count; of an argument struct with scene_of, a_of and frames
template <class Args>
__device__ __forceinline__ const double* scene_frames(const Args& a, long long b, int* A) {
    const int scene = a.scene_of ? min(max(a.scene_of[b], 0), a.n_scenes - 1) : 0;
    *A = clamped_count(a.a_of, scene, a.a_max);
    return a.frames + (size_t)scene * a.a_max * a.m * PQP_AGENT_FRAME_STRIDE;
}

}  // namespace pqp
