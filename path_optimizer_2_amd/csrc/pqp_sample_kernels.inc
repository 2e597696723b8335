// pqp_sample_kernels.inc — instantiated by pqp_speed.hip; includes pqp_driven_path.hpp.  Time-stamped trajectories on a fixed time step
// (pqp_sample_trajectory): where the car is at t0 + k dt, from the waypoints in `paths` and their s, v, a, t in `profile`.  The kinematics
// inside a segment are the speed profile's own - constant acceleration along the chord - so a sample is the closed form of them; the
// reference has no counterpart (nothing fills State::v there).  include/pqp.h states the definition operation by operation.
//
// sample_trajectory_kernel: one wavefront per path, four per workgroup, no LDS, no atomics.
//   1  tiles of 64 waypoints ascending: every value below the driven count is judged (row_not_finite of pqp_driven_path.hpp and this
//      kernel's own terms on t and t0; a ballot decides for the path), and the maximum of the t column gives the arrival time T_{c-1}
//   2  tiles of 64 samples ascending, one sample per lane.  tau and T both ascend, so the t column is walked forward (walk_tile of
//      pqp_driven_path.hpp) by a wave-uniform cursor: a tile of it is taken while its last T is <= the sample tile's last tau, and the
//      next sample tile starts at the tile the previous one ended in.  Then a lane gathers its segment's two rows - read a moment ago
//      by step 1, so they come from this CU's cache or L2 - places itself on the chord (chord_pose) and writes its row of eight doubles.
// A sample's operations depend on its path's driven rows, t0, dt and k alone.

#include "pqp_driven_path.hpp"

namespace pqp {

constexpr int kSampleThreads = 256;

struct SampleArgs {
    int batch, n, stride, m;
    const double* paths;             // [batch][n][stride]  x, y, heading at 0, 1, 2 and k at 5
    const int32_t* n_of;             // [batch] or nullptr: all have n
    const int32_t* stop_before;      // [batch] or nullptr
    const double* profile;           // [batch][n][PQP_SPEED_STRIDE]
    const double* t0;                // [batch] or nullptr: all 0
    pqp_sample_params prm;
    double* traj;                    // [batch][m][PQP_TRAJ_STRIDE]
    int32_t* m_of;                   // [batch]
    int32_t* flags;                  // [batch]
};

__global__ void __launch_bounds__(kSampleThreads) sample_trajectory_kernel(const SampleArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kSampleThreads / 64) + (threadIdx.x >> 6)));
    if (b >= a.batch) return;
    const int c = driven_count(clamped_count(a.n_of, b, a.n), a.stop_before, b);
    const long long cells = (long long)a.m * PQP_TRAJ_STRIDE;
    double* traj = a.traj + (size_t)b * a.m * PQP_TRAJ_STRIDE;
    if (c == 0) {                                                                         // nothing is read, t0 neither
        for (long long e = lane; e < cells; e += 64) traj[e] = 0.0;
        if (lane == 0) { a.m_of[b] = 0; a.flags[b] = PQP_TRAJ_EMPTY; }
        return;
    }
    const double* __restrict__ p = a.paths + (size_t)b * a.n * a.stride;
    const double* __restrict__ prof = a.profile + (size_t)b * a.n * PQP_SPEED_STRIDE;
    const double t0 = a.t0 ? a.t0[b] : 0.0, dt = a.prm.dt;
    const int tiles = (c + 63) / 64;

    // ---- 1: what is read must be numbers; the arrival time ---------------------------------------------------------------------------------
    bool bad = !(t0 >= 0.0 && t0 < INFINITY);
    double t_arrive = -INFINITY;
    for (int w = 0; w < tiles; ++w) {
        const int j = w * 64 + lane;
        double t = -INFINITY;
        if (j < c) {
            const double* r = p + (size_t)j * a.stride;
            const double* o = prof + (size_t)j * PQP_SPEED_STRIDE;
            t = o[3];
            bad = bad || row_not_finite(r, o) || !(t >= 0.0);
        }
        t_arrive = fmax(t_arrive, wave_max(t));
    }
    if (__ballot(bad)) {
        for (long long e = lane; e < cells; e += 64) traj[e] = NAN;
        if (lane == 0) { a.m_of[b] = 0; a.flags[b] = PQP_TRAJ_NOT_FINITE; }
        return;
    }
    const double* last = p + (size_t)(c - 1) * a.stride;
    const double* last_o = prof + (size_t)(c - 1) * PQP_SPEED_STRIDE;
    const double v_last = last_o[1];

    // ---- 2: the samples --------------------------------------------------------------------------------------------------------------------
    int wt = 0;                                  // the waypoint tile the walk stands in: every T before it is <= this sample tile's first tau
    double carry = -INFINITY;                    // the running maximum in front of that tile
    int on_path = 0;
    bool stands = false;
    for (int k0 = 0; k0 < a.m; k0 += 64) {
        const int k = k0 + lane;
        const bool valid = k < a.m;
        const double tau = t0 + (double)k * dt;
        const double tau_hi = uniform(__shfl(tau, min(63, a.m - 1 - k0)));               // tau ascends: the tile's last sample
        int cnt = min(wt * 64, c);
        int w = wt;
        double cw = carry;
        while (w * 64 < c) {
            double T_end;
            cnt += walk_tile(prof, 3, c, w, cw, tau, lane, &T_end);                       // #{ j in this tile : T_j <= tau }
            if (!(T_end <= tau_hi)) break;
            ++w; cw = T_end;
            wt = w; carry = cw;
        }
        const bool on = valid && tau <= t_arrive;
        on_path += __popcll(__ballot(on));
        const int i = max(cnt - 1, 0);           // (cnt = 0 only where the t column does not start at 0 and tau lies in front of it)
        double row[PQP_TRAJ_STRIDE] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (on && i < c - 1) {
            const double* o0 = prof + (size_t)i * PQP_SPEED_STRIDE;
            const double s0 = o0[0], v0 = o0[1], a0 = o0[2], ti = o0[3], t_next = o0[PQP_SPEED_STRIDE + 3];
            stands = stands || fmax(ti, t_next) == INFINITY;                          // T_{i+1}: T_i <= tau is finite here
            const double u = tau - ti;
            double e;
            const PathPose at = chord_pose(p + (size_t)i * a.stride, a.stride, (v0 + (0.5 * a0) * u) * u, &e);
            row[0] = at.x; row[1] = at.y; row[2] = at.heading; row[3] = at.k;
            row[4] = s0 + e;
            row[5] = fmax(v0 + a0 * u, 0.0);
            row[6] = a0;
            row[7] = tau;
        } else if (on || (valid && a.prm.hold_last)) {                                    // the last driven waypoint itself; behind it: at rest
            const PathPose at = waypoint_pose(last);
            row[0] = at.x; row[1] = at.y; row[2] = at.heading; row[3] = at.k; row[4] = last_o[0];
            row[5] = on ? v_last : 0.0;
            row[7] = tau;
        }
        if (valid) {
            double* o = traj + (size_t)k * PQP_TRAJ_STRIDE;
#pragma unroll
            for (int q = 0; q < PQP_TRAJ_STRIDE; ++q) o[q] = row[q];
        }
    }
    const double tau_last = t0 + (double)(a.m - 1) * dt;
    const int fl = (tau_last < t_arrive ? PQP_TRAJ_HORIZON_SHORT : 0) | (__ballot(stands) ? PQP_TRAJ_STANDS : 0) |
                   ((on_path < a.m && v_last > 0.0) ? PQP_TRAJ_ENDS_MOVING : 0);
    if (lane == 0) { a.m_of[b] = on_path; a.flags[b] = fl; }
}

}  // namespace pqp
