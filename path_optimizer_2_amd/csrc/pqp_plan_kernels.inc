// pqp_plan_kernels.inc — instantiated by pqp_speed.hip behind pqp_search_kernels.inc, whose st_count and st_pose it uses;
// includes nothing of its own.  Speed plans on a fine time step (pqp_sample_plan): the m rows a second apart that pqp_speed_search
// or pqp_speed_refine wrote, put on r sub-steps per layer under the plan's own kinematics -
// constant acceleration for a refined path, a straight line in the path-time plane for a searched staircase - and placed on the path by
// the walk the search and the refine share.  The rows are pqp_agents_check's input.  The reference has no counterpart.  include/pqp.h
// states the definition operation by operation.
//
// plan_sample_kernel: one wavefront per path, four per workgroup, no LDS, no atomics.
//   1  tiles of 64 waypoints, then tiles of 64 layers: every value read below the driven count (row_not_finite of pqp_driven_path.hpp) and
//      below the planned layers (s, v, a of a plan row) is judged; a ballot decides for the path
//   2  tiles of 64 fine samples ascending, one sample per lane: the lane reads its layer's s, v, a and the next layer's s, forms its
//      station, finds its segment (st_count) and places the pose (st_pose) as refine_finish_kernel does per layer, and writes its row of
//      eight doubles.  defect and excess are wave_max reductions carried over the tiles; lane 0 writes the path's scalars.
// A path's result depends on its own rows, dt, r and the kinematics chosen for it alone.

namespace pqp {

constexpr int kPlanThreads = 256;

struct PlanArgs {
    int batch, n, stride, m, r, linear;
    double dt;
    const double* paths;             // [batch][n][stride]  x, y, heading at 0, 1, 2 and k at 5
    const int32_t* n_of;             // [batch] or nullptr
    const int32_t* stop_before;      // [batch] or nullptr
    const double* profile;           // [batch][n][PQP_SPEED_STRIDE]
    const double* plan;              // [batch][m][PQP_TRAJ_STRIDE]  s, v, a at 4, 5, 6
    const int32_t* count_of;         // [batch] or nullptr: all have m layers
    const int32_t* refine_flags;     // [batch] or nullptr: every path by `linear`
    double* fine;                    // [batch][(m - 1) r + 1][PQP_TRAJ_STRIDE]
    int32_t* m_of;                   // [batch]
    double* defect;                  // [batch] or nullptr
    double* excess;                  // [batch] or nullptr
    int32_t* flags;                  // [batch]
};

__global__ void __launch_bounds__(kPlanThreads) plan_sample_kernel(const PlanArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kPlanThreads / 64) + (threadIdx.x >> 6)));
    if (b >= a.batch) return;
    const int c = driven_count(clamped_count(a.n_of, b, a.n), a.stop_before, b);
    const int L = clamped_count(a.count_of, b, a.m);
    const int r = a.r;
    const long long M = (long long)(a.m - 1) * r + 1;
    double* __restrict__ fine = a.fine + (size_t)b * M * PQP_TRAJ_STRIDE;
    const double* __restrict__ p = a.paths + (size_t)b * a.n * a.stride;
    const double* __restrict__ prof = a.profile + (size_t)b * a.n * PQP_SPEED_STRIDE;
    const double* __restrict__ plan = a.plan + (size_t)b * a.m * PQP_TRAJ_STRIDE;

    // ---- 1: what is read must be numbers ---------------------------------------------------------------------------------------------------
    bool bad = false;
    if (c > 0 && L > 0) {
        for (int w = 0; w * 64 < c; ++w) {
            const int i = w * 64 + lane;
            if (i < c) bad = bad || row_not_finite(p + (size_t)i * a.stride, prof + (size_t)i * PQP_SPEED_STRIDE);
        }
        for (int w = 0; w * 64 < L; ++w) {
            const int k = w * 64 + lane;
            if (k < L) {
                const double* row = plan + (size_t)k * PQP_TRAJ_STRIDE;
                bad = bad || !isfinite(row[4]) || !isfinite(row[5]) || !isfinite(row[6]);
            }
        }
        bad = __ballot(bad) != 0;
    }
    if (c == 0 || L == 0 || bad) {
        const double fill = bad ? NAN : 0.0;
        for (long long e = lane; e < M * PQP_TRAJ_STRIDE; e += 64) fine[e] = fill;
        if (lane == 0) {
            a.m_of[b] = 0;
            if (a.defect) a.defect[b] = NAN;
            if (a.excess) a.excess[b] = NAN;
            a.flags[b] = bad ? PQP_PLAN_NOT_FINITE : PQP_PLAN_EMPTY;
        }
        return;
    }

    // ---- 2: the samples --------------------------------------------------------------------------------------------------------------------
    const bool line = a.refine_flags ? (a.refine_flags[b] & PQP_REFINE_REFINED) == 0 : a.linear != 0;
    const double dt = a.dt, rr = (double)r;
    const long long on_plan = (long long)(L - 1) * r + 1;
    double off = 0.0, over = -INFINITY;
    bool backward = false;
    for (long long f0 = 0; f0 < M; f0 += 64) {
        const long long f = f0 + lane;
        const bool on = f < on_plan;
        double row[PQP_TRAJ_STRIDE] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double s = -INFINITY, gap = 0.0;
        if (on) {
            const int k = (int)(f / r), i = (int)(f - (long long)k * r);
            const double* here = plan + (size_t)k * PQP_TRAJ_STRIDE;
            const double sk = here[4], vk = here[5], ak = here[6];
            if (k < L - 1) {
                const double sn = here[PQP_TRAJ_STRIDE + 4];
                const double u = ((double)i * dt) / rr;
                double at;
                if (line) {
                    at = sk + ((sn - sk) * (double)i) / rr;
                    row[5] = (sn - sk) / dt;
                } else {
                    at = sk + (vk + (0.5 * ak) * u) * u;
                    row[5] = fmax(vk + ak * u, 0.0);
                    row[6] = ak;
                    if (i == 0) gap = fabs((sk + (vk + (0.5 * ak) * dt) * dt) - sn);
                }
                s = fmin(fmax(at, sk), fmax(sn, sk));
                row[7] = (double)k * dt + u;
                backward = backward || sn < sk;
            } else {                                         // the last planned layer: the row itself
                s = sk;
                row[5] = fmax(vk, 0.0);
                row[6] = ak;
                row[7] = (double)k * dt;
            }
            row[4] = s;
        }
        const int cnt = st_count(prof, c, s, lane);
        double above = -INFINITY;
        if (on) {
            double w;
            const PathPose o = st_pose(p, prof, a.stride, c, cnt, s, &w);
            row[0] = o.x; row[1] = o.y; row[2] = o.heading; row[3] = o.k;
            above = row[5] - sqrt(fmax(w, 0.0));
        }
        if (f < M) {
            double* o = fine + (size_t)f * PQP_TRAJ_STRIDE;
#pragma unroll
            for (int q = 0; q < PQP_TRAJ_STRIDE; ++q) o[q] = row[q];
        }
        off = fmax(off, wave_max(gap));
        over = fmax(over, wave_max(above));
    }
    const bool any_backward = __ballot(backward) != 0;
    if (lane == 0) {
        a.m_of[b] = (int32_t)on_plan;
        if (a.defect) a.defect[b] = off;
        if (a.excess) a.excess[b] = over;
        a.flags[b] = any_backward ? PQP_PLAN_BACKWARD : 0;
    }
}

}  // namespace pqp
