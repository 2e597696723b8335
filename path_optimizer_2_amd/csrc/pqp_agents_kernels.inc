// pqp_agents_kernels.inc — instantiated by pqp_agents.hip; includes pqp_car_circles.hpp and pqp_agent_frames.hpp.  Sampled trajectories against predicted moving agents
// (pqp_agents_check): every sample of every trajectory against every agent of the path's scene at the same time step, the six-circle
// footprint (pqp_car_circles, placed by local_to_global) against a rounded oriented rectangle.  The reference has
// no counterpart: it plans one path against a static map.  include/pqp.h states the definition operation by operation.
//
// agent_frames_kernel: one lane per (scene, agent, step).  The agent's sincos is taken here, once, so the batch x agents x steps tests
//   never take it again; reach = the circumradius of the rounded rectangle, whose sign and NaN also say "absent" and "bad".
// agents_check_kernel<CLEARANCE>: one wavefront per path, four per workgroup, one sample per lane in tiles of 64, no LDS, no atomics.
//   The loop over agents is wave-uniform; lane k reads frame row [a][k], so a wavefront's 64 rows are one contiguous 4 KB, and a scene's
//   table is read by every path of the scene: it stays in L2.  first_hit is a ballot and a count of trailing zeros, hit_agent is read from
//   the hit lane.  Without a clearance to write (CLEARANCE = false) a lane leaves out the agents it cannot come within the margin of
//   (agent_out_of_reach, whose slack is orders above the rounding of the exact test) and the agents behind its first hit, and the
//   wavefront stops behind the tile of its first hit: none of that changes an output.
// agent_frames_kernel also writes the frames of st_occupancy_kernel (pqp_search_kernels.inc) and of overlay_kernel (pqp_overlay_kernels.inc):
// their units call launch_agent_frames (pqp_internal.hpp, defined in pqp_agents.hip), so the kernel exists in this unit alone.  What the
// three share about a frame row - agent_clear, the reading of its reach, the broad phase, the scene's lookup - is pqp_agent_frames.hpp.

#include "pqp_car_circles.hpp"
#include "pqp_agent_frames.hpp"

namespace pqp {

struct AgentsArgs {
    int batch, m, stride, n_scenes, a_max;
    const double* traj;              // [batch][m][stride]  x, y, heading at offsets 0, 1, 2
    const int32_t* m_of;             // [batch] or nullptr: all m
    const int32_t* a_of;             // [n_scenes] or nullptr: all a_max
    const int32_t* scene_of;         // [batch] or nullptr: scene 0
    double margin;
    CarCircles car;
    double* frames;                  // [n_scenes][a_max][m][PQP_AGENT_FRAME_STRIDE]
    int32_t* first_hit;              // [batch]
    int32_t* hit_agent;              // [batch]
    double* clearance;               // [batch][m] or nullptr
};

struct AgentFramesArgs {
    long long rows;                  // n_scenes * a_max * m
    const double* agents;            // [rows][PQP_AGENT_STRIDE]
    double* frames;                  // [rows][PQP_AGENT_FRAME_STRIDE]
};

__global__ void __launch_bounds__(kAgentsThreads) agent_frames_kernel(const AgentFramesArgs a) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kAgentsThreads + threadIdx.x;
    if (i >= a.rows) return;
    const double* __restrict__ r = a.agents + (size_t)i * PQP_AGENT_STRIDE;
    double* __restrict__ o = a.frames + (size_t)i * PQP_AGENT_FRAME_STRIDE;
    double f[PQP_AGENT_FRAME_STRIDE] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0};
    const double hl = r[3], hw = r[4];
    if (!(hl < 0.0 || hw < 0.0)) {                                                        // present: the rest of the row is read
        const double x = r[0], y = r[1], heading = r[2], radius = r[5];
        if (isfinite(x) && isfinite(y) && isfinite(heading) && isfinite(hl) && isfinite(hw) && isfinite(radius) && radius >= 0.0) {
            double sh, ch;
            sincos(heading, &sh, &ch);
            f[0] = x; f[1] = y; f[2] = ch; f[3] = sh; f[4] = hl; f[5] = hw; f[6] = radius;
            f[7] = sqrt(hl * hl + hw * hw) + radius;
        } else {
            f[7] = NAN;                                                                   // bad
        }
    }
#pragma unroll
    for (int q = 0; q < PQP_AGENT_FRAME_STRIDE; ++q) o[q] = f[q];
}

template <bool CLEARANCE>
__global__ void __launch_bounds__(kAgentsThreads) agents_check_kernel(const AgentsArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kAgentsThreads / 64) + (threadIdx.x >> 6)));
    if (b >= a.batch) return;
    const int count = clamped_count(a.m_of, b, a.m);
    // (in front of the scene lookup: the traj pointer is then fetched with the frames pointer, one round of argument loads fewer before
    // the first tile - 0.2 us of a 17 us call, profiles/r19a_path_kernels_speed.txt)
    const double* __restrict__ traj = a.traj + (size_t)b * a.m * a.stride;
    int A;
    const double* __restrict__ frames = scene_frames(a, b, &A);
    const double margin = a.margin;
    int first = count, who = -1;                                                          // wave-uniform
    const int k_end = CLEARANCE ? a.m : count;
    for (int k0 = 0; k0 < k_end; k0 += 64) {
        const int k = k0 + lane;
        const bool checked = k < count;
        double clear = INFINITY;
        int hit_a = -1;
        bool hit = false;
        if (checked) {
            const double* s = traj + (size_t)k * a.stride;
            const double x = s[0], y = s[1], heading = s[2];
            if (isfinite(x) && isfinite(y) && isfinite(heading)) {
                double sh, ch;
                sincos(heading, &sh, &ch);
                double gx[6], gy[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const Point2 g = local_to_global(a.car.cx[j], a.car.cy[j], sh, ch, x, y);
                    gx[j] = g.x; gy[j] = g.y;
                }
                const Point2 bp = local_to_global(a.car.cx[6], a.car.cy[6], sh, ch, x, y);
                const double* f = frames + (size_t)k * PQP_AGENT_FRAME_STRIDE;
                for (int ag = 0; ag < A; ++ag, f += (size_t)a.m * PQP_AGENT_FRAME_STRIDE) {
                    if (!CLEARANCE && hit) break;                                         // the lowest hitting agent is found
                    const double ax = f[0], ay = f[1], reach = f[7];
                    if (agent_absent(reach)) continue;
                    double c_ka = -INFINITY;                                              // what a bad agent gives
                    if (!agent_bad(reach)) {
                        if (!CLEARANCE && agent_out_of_reach(a.car.rb, reach, margin, bp.x, bp.y, ax, ay)) continue;        // no hit
                        c_ka = agent_clear(gx, gy, a.car.cr, ax, ay, f[2], f[3], f[4], f[5], f[6]);
                    }
                    clear = fmin(clear, c_ka);
                    if (c_ka < margin && !hit) { hit = true; hit_a = ag; }
                }
            } else {
                clear = -INFINITY;                                                        // the ego sample itself: hit_agent -1
                hit = true;
            }
        }
        if (CLEARANCE && k < a.m) a.clearance[(size_t)b * a.m + k] = checked ? clear : 0.0;
        const uint64_t hits = __ballot(hit);
        if (hits && first == count) {
            const int at = __builtin_ctzll(hits);
            first = k0 + at;
            who = __builtin_amdgcn_readlane(hit_a, at);
            if (!CLEARANCE) break;
        }
    }
    if (lane == 0) { a.first_hit[b] = first; a.hit_agent[b] = who; }
}

}  // namespace pqp
