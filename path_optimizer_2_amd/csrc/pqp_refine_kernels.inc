// pqp_refine_kernels.inc — instantiated by pqp_speed.hip behind pqp_search_kernels.inc, whose st_count, st_pose and st_judge it
// uses; includes pqp_banded_qp.hpp (kRMax, the core's row length).  The jerk-limited speed QP behind the path-time search
// (pqp_speed_refine): the corridor around the searched plan from the search's own occupancy bits, the assembly of the QP for the generic
// banded core (pqp_banded_qp.hpp, launched from pqp_smoothers.hip between the second and the third kernel here), and the placement of the
// refined stations back on the path.  The reference has no counterpart.  include/pqp.h states the definition operation by operation.
//
// One wavefront per path in the first and the third kernel, no atomics; a path's result depends on its own rows alone.
// st_corridor_kernel: decides whether the path is refined at all (flags = PQP_REFINE_KEPT otherwise, which the two kernels behind read),
//   places the stations' envelope venv_j a tile of 64 at a time as st_occupancy_kernel's step 2 does (st_count / st_pose) into LDS, then a
//   lane per layer finds the free run around j_k by bit scans over the OR of the three layers' words and takes the run's largest venv.
// refine_assemble_kernel: a lane per (path, layer), after post_assemble_kernel; a kept path gets the all-dummy QP (unit diagonal, zero
//   rows, bounds +-1e30), which the core solves at x = 0 beside the real ones.
// refine_finish_kernel: a lane per layer clamps s_k into its corridor, places it with the same walk, writes the row and the excess over the
//   envelope at the placed pose; a kept path gets search_traj's rows.

#include "pqp_banded_qp.hpp"

namespace pqp {

constexpr int kRefineThreads = 64;

struct RefineArgs {
    int batch, n, stride, m, stations, window;
    double dt, ds, w_ref, w_accel, w_jerk, a_max, d_max;
    const double* paths;             // [batch][n][stride]
    const int32_t* n_of;             // [batch] or nullptr
    const int32_t* stop_before;      // [batch] or nullptr
    const double* profile;           // [batch][n][PQP_SPEED_STRIDE]
    const double* v_start;           // [batch]
    const int32_t* blocked;          // [batch][m][W]
    const int32_t* steps;            // [batch][m][2]
    const int32_t* reached;          // [batch]
    const double* search_traj;       // [batch][m][PQP_TRAJ_STRIDE]
    double* corridor;                // [batch][m][3]  lo, hi, vcap: the handle's
    double *pband, *q, *aval, *lo, *up;      // the QPs, as BandedQpArgs takes them
    const double* x;                 // [batch][3 m]   the core's solution
    double* traj;                    // [batch][m][PQP_TRAJ_STRIDE]
    double* bounds;                  // [batch][m][3] or nullptr
    double* cost;                    // [batch]
    double* excess;                  // [batch] or nullptr
    int32_t* status;                 // [batch]  the core's, then the call's
    int32_t* iters;                  // [batch]
    int32_t* flags;                  // [batch]  st_corridor_kernel's decision, then the call's
};

// what st_judge reads of a search's arguments
__device__ __forceinline__ SearchArgs refine_as_search(const RefineArgs& a) {
    SearchArgs s;
    s.n = a.n; s.stride = a.stride; s.paths = a.paths; s.profile = a.profile; s.v_start = a.v_start;
    return s;
}

// the OR of layer k and its two neighbours, word w
__device__ __forceinline__ uint32_t rf_occ(const int32_t* __restrict__ blk, int W, int m, int k, int w) {
    return (uint32_t)(blk[(size_t)k * W + w] | blk[(size_t)max(k - 1, 0) * W + w] | blk[(size_t)min(k + 1, m - 1) * W + w]);
}

__global__ void __launch_bounds__(kRefineThreads) st_corridor_kernel(const RefineArgs a) {
#pragma clang fp contract(off)
    __shared__ double venv[PQP_SEARCH_MAX_STATES];
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    const int S = a.stations, W = (S + 31) / 32, m = a.m;
    const int c = driven_count(clamped_count(a.n_of, b, a.n), a.stop_before, b);
    double m_last = -INFINITY;
    bool keep = m < 2 || a.reached[b] != m || c == 0;
    if (!keep) keep = st_judge(refine_as_search(a), b, c, lane, &m_last);
    int J = 0;                                               // #{ j < S : sigma_j <= M_{c-1} }, as st_search_kernel counts it
    if (!keep) {
        for (int lo = 0, hi = S; ; ) {
            if (lo == hi) { J = lo; break; }
            const int mid = (lo + hi) >> 1;
            if ((double)mid * a.ds <= m_last) lo = mid + 1; else hi = mid;
        }
        keep = J == 0;
    }
    if (keep) {
        if (lane == 0) a.flags[b] = PQP_REFINE_KEPT;
        return;
    }
    const double* __restrict__ p = a.paths + (size_t)b * a.n * a.stride;
    const double* __restrict__ prof = a.profile + (size_t)b * a.n * PQP_SPEED_STRIDE;
    for (int j0 = 0; j0 < J; j0 += 64) {
        const int j = j0 + lane;
        const bool on = j < J;
        const double sigma = (double)j * a.ds;
        const int cnt = st_count(prof, c, on ? sigma : -INFINITY, lane);
        if (on) {
            double w;
            (void)st_pose(p, prof, a.stride, c, cnt, sigma, &w);
            venv[j] = sqrt(fmax(w, 0.0));
        }
    }
    __syncthreads();
    const int32_t* __restrict__ blk = a.blocked + (size_t)b * m * W;
    const int32_t* __restrict__ steps = a.steps + (size_t)b * m * 2;
    double* __restrict__ cor = a.corridor + (size_t)b * m * 3;
    const int window = min(a.window, S);
    bool strange = false;                                    // a station outside the path, or one that is not free: no search wrote this
    for (int k0 = 0; k0 < m; k0 += 64) {
        const int k = k0 + lane;
        if (k < m) {
            const int jk = steps[2 * k];
            if (jk < 0 || jk >= J || ((rf_occ(blk, W, m, k, jk >> 5) >> (jk & 31)) & 1u)) { strange = true; continue; }
            const int low = max(jk - window, 0), high = min(jk + window, J - 1);
            int jlo = low, jhi = high;
            for (int w = jk >> 5; w >= (low >> 5); --w) {                                 // the highest occupied station of low .. jk
                uint32_t bits = rf_occ(blk, W, m, k, w);
                if (w == (jk >> 5)) bits &= 0xffffffffu >> (31 - (jk & 31));
                if (w == (low >> 5)) bits &= 0xffffffffu << (low & 31);
                if (bits) { jlo = 32 * w + (31 - __clz((int)bits)) + 1; break; }
            }
            for (int w = jk >> 5; w <= (high >> 5); ++w) {                                // the lowest occupied station of jk .. high
                uint32_t bits = rf_occ(blk, W, m, k, w);
                if (w == (jk >> 5)) bits &= 0xffffffffu << (jk & 31);
                if (w == (high >> 5)) bits &= 0xffffffffu >> (31 - (high & 31));
                if (bits) { jhi = 32 * w + (__ffs((int)bits) - 1) - 1; break; }
            }
            double vcap = venv[jlo];
            for (int j = jlo + 1; j <= jhi; ++j) vcap = fmax(vcap, venv[j]);
            cor[3 * k] = k == 0 ? 0.0 : (double)jlo * a.ds;
            cor[3 * k + 1] = k == 0 ? 0.0 : (double)jhi * a.ds;
            cor[3 * k + 2] = vcap;
        }
    }
    const bool any = __ballot(strange) != 0;
    if (lane == 0) a.flags[b] = any ? PQP_REFINE_KEPT : 0;
}

// (s, v, a)_k -> 3k + {0, 1, 2}.  rows k, m + k, 2m + k: the boxes of s_k, v_k, a_k;  3m + k: s_{k+1} - s_k - dt v_k - (dt^2 / 2) a_k = 0;
// 4m - 1 + k: v_{k+1} - v_k - dt a_k = 0, their entries in ascending column order (sm_upload_structure's slots)
__global__ void refine_assemble_kernel(const RefineArgs a) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = a.m;
    if (idx >= (long long)a.batch * m) return;
    const long long b = idx / m;
    const int k = (int)(idx - b * m);
    const int nv = 3 * m, nc = 5 * m - 2;
    const bool dummy = (a.flags[b] & PQP_REFINE_KEPT) != 0;
    double* pb = a.pband + (size_t)b * 4 * nv;
    double* qq = a.q + (size_t)b * nv;
    double* av = a.aval + (size_t)b * nc * kRMax;
    double* l = a.lo + (size_t)b * nc;
    double* u = a.up + (size_t)b * nc;
    const bool last = k == m - 1;
    const double jerk = a.w_jerk / (a.dt * a.dt);
#pragma unroll
    for (int d = 1; d < 4; ++d) pb[(size_t)d * nv + 3 * k] = pb[(size_t)d * nv + 3 * k + 1] = pb[(size_t)d * nv + 3 * k + 2] = 0.0;
    double* r0 = av + (size_t)k * kRMax;
    double* r1 = av + (size_t)(m + k) * kRMax;
    double* r2 = av + (size_t)(2 * m + k) * kRMax;
    double* r3 = av + (size_t)(3 * m + k) * kRMax;           // (k < m - 1 only)
    double* r4 = av + (size_t)(4 * m - 1 + k) * kRMax;
    r0[1] = r0[2] = r0[3] = r1[1] = r1[2] = r1[3] = r2[1] = r2[2] = r2[3] = 0.0;
    qq[3 * k + 1] = qq[3 * k + 2] = 0.0;
    if (dummy) {
        pb[3 * k] = pb[3 * k + 1] = pb[3 * k + 2] = 1.0;
        qq[3 * k] = 0.0;
        r0[0] = r1[0] = r2[0] = 0.0;
        l[k] = l[m + k] = l[2 * m + k] = -1e30;
        u[k] = u[m + k] = u[2 * m + k] = 1e30;
        if (!last) {
            r3[0] = r3[1] = r3[2] = r3[3] = r4[0] = r4[1] = r4[2] = r4[3] = 0.0;
            l[3 * m + k] = l[4 * m - 1 + k] = -1e30;
            u[3 * m + k] = u[4 * m - 1 + k] = 1e30;
        }
        return;
    }
    const double sigma = (double)a.steps[((size_t)b * m + k) * 2] * a.ds;
    const double* cor = a.corridor + ((size_t)b * m + k) * 3;
    pb[3 * k] = 2.0 * a.w_ref;
    pb[3 * k + 1] = 0.0;
    pb[3 * k + 2] = 2.0 * a.w_accel + (double)((k > 0) + (last ? 0 : 1)) * (2.0 * jerk);
    if (!last) pb[(size_t)3 * nv + 3 * k + 2] = -(2.0 * jerk);
    qq[3 * k] = -(2.0 * a.w_ref) * sigma;
    r0[0] = r1[0] = r2[0] = 1.0;
    if (k == 0) {
        l[0] = u[0] = 0.0;
        l[m] = u[m] = a.v_start[b];
    } else {
        l[k] = cor[0]; u[k] = cor[1];
        l[m + k] = 0.0; u[m + k] = cor[2];
    }
    l[2 * m + k] = last ? 0.0 : -a.d_max;
    u[2 * m + k] = last ? 0.0 : a.a_max;
    if (!last) {
        r3[0] = -1.0; r3[1] = -a.dt; r3[2] = -(0.5 * (a.dt * a.dt)); r3[3] = 1.0;
        r4[0] = -1.0; r4[1] = -a.dt; r4[2] = 1.0; r4[3] = 0.0;
        l[3 * m + k] = u[3 * m + k] = 0.0;
        l[4 * m - 1 + k] = u[4 * m - 1 + k] = 0.0;
    }
}

__global__ void __launch_bounds__(kRefineThreads) refine_finish_kernel(const RefineArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    const int m = a.m;
    const bool kept_early = (a.flags[b] & PQP_REFINE_KEPT) != 0;
    const int st = kept_early ? PQP_STATUS_UNSOLVED : a.status[b];
    double* __restrict__ traj = a.traj + (size_t)b * m * PQP_TRAJ_STRIDE;
    double* bounds = a.bounds ? a.bounds + (size_t)b * m * 3 : nullptr;
    if (st != PQP_STATUS_SOLVED) {
        const double* __restrict__ from = a.search_traj + (size_t)b * m * PQP_TRAJ_STRIDE;
        for (long long e = lane; e < (long long)m * PQP_TRAJ_STRIDE; e += kRefineThreads) traj[e] = from[e];
        if (bounds)
            for (int e = lane; e < 3 * m; e += kRefineThreads) bounds[e] = 0.0;
        if (lane == 0) {
            a.cost[b] = NAN;
            if (a.excess) a.excess[b] = NAN;
            a.status[b] = st;
            if (kept_early) a.iters[b] = 0;
            a.flags[b] = PQP_REFINE_KEPT | (st == PQP_STATUS_PRIMAL_INFEASIBLE ? PQP_REFINE_INFEASIBLE : 0);
        }
        return;
    }
    const int c = driven_count(clamped_count(a.n_of, b, a.n), a.stop_before, b);
    const double* __restrict__ p = a.paths + (size_t)b * a.n * a.stride;
    const double* __restrict__ prof = a.profile + (size_t)b * a.n * PQP_SPEED_STRIDE;
    const double* __restrict__ x = a.x + (size_t)b * 3 * m;
    const double* __restrict__ cor = a.corridor + (size_t)b * m * 3;
    const int32_t* __restrict__ steps = a.steps + (size_t)b * m * 2;
    const double jerk = a.w_jerk / (a.dt * a.dt);
    double over = -INFINITY, total = 0.0;
    for (int k0 = 0; k0 < m; k0 += 64) {
        const int k = k0 + lane;
        const bool on = k < m;
        double s = -INFINITY, v = 0.0, acc = 0.0, term = 0.0, lo = 0.0, hi = 0.0, vcap = 0.0;
        if (on) {
            const double sk = x[3 * k], ak = x[3 * k + 2];
            lo = cor[3 * k]; hi = cor[3 * k + 1]; vcap = cor[3 * k + 2];
            s = fmin(fmax(sk, lo), hi);
            v = fmax(x[3 * k + 1], 0.0);
            acc = k == m - 1 ? 0.0 : ak;
            const double dev = sk - (double)steps[2 * k] * a.ds;
            term = a.w_ref * (dev * dev) + a.w_accel * (ak * ak);
            if (k < m - 1) { const double da = x[3 * k + 5] - ak; term = term + jerk * (da * da); }
        }
        const int cnt = st_count(prof, c, s, lane);
        double gap = -INFINITY;
        if (on) {
            double w;
            const PathPose o = st_pose(p, prof, a.stride, c, cnt, s, &w);
            gap = v - sqrt(fmax(w, 0.0));
            double* r = traj + (size_t)k * PQP_TRAJ_STRIDE;
            r[0] = o.x; r[1] = o.y; r[2] = o.heading; r[3] = o.k; r[4] = s; r[5] = v; r[6] = acc; r[7] = (double)k * a.dt;
            if (bounds) { bounds[3 * k] = lo; bounds[3 * k + 1] = hi; bounds[3 * k + 2] = vcap; }
        }
        over = fmax(over, wave_max(gap));
        total = total + wave_sum(term);
    }
    if (lane == 0) {
        a.cost[b] = total;
        if (a.excess) a.excess[b] = over;
        a.flags[b] = PQP_REFINE_REFINED;
    }
}

}  // namespace pqp
