// pqp_speed_kernels.inc — instantiated by pqp_speed.hip; includes pqp_driven_path.hpp.  Planned paths to trajectories (pqp_speed_profile): arc
// length, speed, acceleration and time of every waypoint.  The reference's State carries s, v and a (include/data_struct/data_struct.hpp:14-26)
// and nothing fills them; getOptimizedPath adds the chords up in tmp_s and drops the sum (src/solver/base_solver.cpp:268,282-284).
//
// The speed is the textbook forward pass (acceleration) then backward pass (braking) over w = v^2, which in closed form is
//   w_i = min( cap_i, min_{j < i} (cap_j + 2 a_max (s_i - s_j)), min_{j > i} (cap_j + 2 d_max (s_j - s_i)) )
// - a prefix minimum of cap_j - 2 a_max s_j and a suffix minimum of cap_j + 2 d_max s_j on top of a prefix sum for s and one for t.  min is
// exact and associative, so only the sums round.  The cap_i term stays explicit and the minima run over j != i: the j = i term of the
// shifted form, (cap_i - 2 a s_i) + 2 a s_i, does not give cap_i back bit for bit.
//
// speed_profile_kernel: one wavefront per path, four per workgroup, one waypoint per lane, tiles of 64 waypoints with the carries in
// registers, so n has no cap.  The scans are DPP (pqp_wave.hpp): no LDS, no atomics.  Three sweeps, the profile's own rows as the
// workspace between them (they stay in this CU's cache and in L2):
//   A  tiles ascending    reads x, y, k (and v_limit); writes s, the forward-limited w, cap, the chord that arrives at the waypoint
//   B  tiles descending   lane L of a tile holds waypoint top - L, so the suffix minimum is the same prefix scan; writes v, a and the time
//                         of the chord that leaves the waypoint
//   C  tiles ascending    the prefix sum of those times
// A row is written by one lane in a sweep and read by another in the next, hence the workgroup fence between the sweeps.
// The order of a path's additions depends on its driven count alone.

#include "pqp_driven_path.hpp"

namespace pqp {

constexpr int kSpeedThreads = 256;

struct SpeedArgs {
    int batch, n, stride;
    const double* paths;             // [batch][n][stride]  x, y at 0, 1 and k at 5
    const int32_t* n_of;             // [batch] or nullptr: all have n
    const int32_t* stop_before;      // [batch] or nullptr
    const double* v_limit;           // [batch][n] or nullptr
    const double* v_start;           // [batch]
    const double* v_end;             // [batch] or nullptr
    pqp_speed_params prm;
    double* profile;                 // [batch][n][PQP_SPEED_STRIDE]
    int32_t* flags;                  // [batch]
};

__global__ void __launch_bounds__(kSpeedThreads) speed_profile_kernel(const SpeedArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kSpeedThreads / 64) + (threadIdx.x >> 6)));
    if (b >= a.batch) return;
    const int count = clamped_count(a.n_of, b, a.n);
    const int c = driven_count(count, a.stop_before, b);
    const bool early = c < count;
    double* prof = a.profile + (size_t)b * a.n * PQP_SPEED_STRIDE;
    // rows that are not driven: zeros (four doubles a row: one contiguous span)
    for (long long e = (long long)c * PQP_SPEED_STRIDE + lane; e < (long long)a.n * PQP_SPEED_STRIDE; e += 64) prof[e] = 0.0;
    if (c == 0) {
        if (lane == 0) a.flags[b] = PQP_SPEED_EMPTY | (early ? PQP_SPEED_STOPS_EARLY : 0);
        return;
    }
    const double* __restrict__ p = a.paths + (size_t)b * a.n * a.stride;
    const double* __restrict__ vl = a.v_limit ? a.v_limit + (size_t)b * a.n : nullptr;
    const double vs = a.v_start[b], ve = a.v_end ? a.v_end[b] : NAN;
    const double vs2 = vs * vs;
    const double two_a = 2.0 * a.prm.a_max, two_d = 2.0 * a.prm.d_max, vmax2 = a.prm.v_max * a.prm.v_max;
    const int tiles = (c + 63) / 64;
    // a speed that is read must be a number that is not negative; v_end may be NaN: free
    bool bad = !(vs >= 0.0 && vs < INFINITY) || (!early && ve == ve && !(ve >= 0.0 && ve < INFINITY));

    // ---- A: s, cap and the forward-limited w ------------------------------------------------------------------------------------------
    {
        double s_carry = 0.0, g_carry = INFINITY, x_carry = 0.0, y_carry = 0.0;
        for (int t = 0; t < tiles; ++t) {
            const int i = t * 64 + lane;
            const bool valid = i < c;
            double x = 0.0, y = 0.0, k = 0.0, lim = INFINITY;
            if (valid) {
                const double* r = p + (size_t)i * a.stride;
                x = r[0]; y = r[1]; k = r[5];
                if (vl) lim = vl[i];
            }
            const double xp = wave_shift_up(x, x_carry), yp = wave_shift_up(y, y_carry);
            x_carry = wave_read<63>(x); y_carry = wave_read<63>(y);
            const double dx = x - xp, dy = y - yp;
            const double d_in = (valid && i > 0) ? sqrt(dx * dx + dy * dy) : 0.0;       // the chord from waypoint i - 1
            const double s = s_carry + wave_prefix_sum(d_in);
            s_carry = wave_read<63>(s);
            double cap = vmax2;
            cap = fmin(cap, lim * lim);
            if (k != 0.0) cap = fmin(cap, a.prm.a_lat_max / fabs(k));
            if (i == 0) cap = fmin(cap, vs2);
            if (i == c - 1) cap = early ? 0.0 : (ve == ve ? fmin(cap, ve * ve) : cap);
            bad = bad || (valid && (!isfinite(x) || !isfinite(y) || !isfinite(k) || !(lim >= 0.0) || !isfinite(s)));
            const double g = valid ? cap - two_a * s : INFINITY;
            const double g_incl = fmin(wave_prefix_min(g), g_carry);
            const double g_before = wave_shift_up(g_incl, g_carry);                       // min over j < i
            g_carry = wave_read<63>(g_incl);
            const double w_fwd = fmin(cap, g_before + two_a * s);
            if (valid) {
                double* o = prof + (size_t)i * PQP_SPEED_STRIDE;
                o[0] = s; o[1] = w_fwd; o[2] = cap; o[3] = d_in;
            }
        }
    }
    if (__ballot(bad)) {
        for (long long e = lane; e < (long long)c * PQP_SPEED_STRIDE; e += 64) prof[e] = NAN;
        if (lane == 0) a.flags[b] = PQP_SPEED_NOT_FINITE;
        return;
    }
    __threadfence_block();

    // ---- B: the braking limit from behind, then v, a and the time of the chord that leaves each waypoint ----------------------------------
    bool never = false, too_fast = false;
    {
        double h_carry = INFINITY, w_carry = 0.0, d_carry = 0.0;
        for (int t = 0; t < tiles; ++t) {
            const int i = c - 1 - t * 64 - lane;                                          // descending along the lanes
            const bool valid = i >= 0;
            double s = 0.0, w_fwd = 0.0, cap = INFINITY, d_in = 0.0;
            if (valid) {
                const double* o = prof + (size_t)i * PQP_SPEED_STRIDE;
                s = o[0]; w_fwd = o[1]; cap = o[2]; d_in = o[3];
            }
            const double hh = valid ? cap + two_d * s : INFINITY;
            const double h_incl = fmin(wave_prefix_min(hh), h_carry);
            const double h_behind = wave_shift_up(h_incl, h_carry);                       // min over j > i
            h_carry = wave_read<63>(h_incl);
            // (the scan's s may step back by an ulp over a duplicate waypoint: a zero cap behind it must not come out as -1e-16)
            const double w = fmax(fmin(w_fwd, h_behind - two_d * s), 0.0);
            const double w_next = wave_shift_up(w, w_carry), d_out = wave_shift_up(d_in, d_carry);       // waypoint i + 1's w, the chord to it
            w_carry = wave_read<63>(w); d_carry = wave_read<63>(d_in);
            const double v = sqrt(w), v_next = sqrt(w_next);
            double acc = 0.0, dt = 0.0;
            if (valid && i < c - 1 && d_out != 0.0) {
                acc = (w_next - w) / (2.0 * d_out);
                const double vv = v + v_next;
                dt = vv == 0.0 ? INFINITY : 2.0 * d_out / vv;
                never = never || vv == 0.0;
            }
            if (valid) {
                double* o = prof + (size_t)i * PQP_SPEED_STRIDE;
                o[1] = v; o[2] = acc; o[3] = dt;
            }
            if (i == 0) too_fast = w < vs2;
        }
    }
    __threadfence_block();

    // ---- C: t --------------------------------------------------------------------------------------------------------------------------
    {
        double t_carry = 0.0, dt_carry = 0.0;
        for (int t = 0; t < tiles; ++t) {
            const int i = t * 64 + lane;
            const bool valid = i < c;
            double* o = prof + (size_t)i * PQP_SPEED_STRIDE + 3;
            const double dt = valid ? *o : 0.0;
            const double dt_in = wave_shift_up(dt, dt_carry);                             // of the chord from waypoint i - 1; 0 at waypoint 0
            dt_carry = wave_read<63>(dt);
            const double tt = t_carry + wave_prefix_sum(dt_in);
            t_carry = wave_read<63>(tt);
            if (valid) *o = tt;
        }
    }
    const int fl = (__ballot(too_fast) ? PQP_SPEED_START_TOO_FAST : 0) | (early ? PQP_SPEED_STOPS_EARLY : 0) |
                   (__ballot(never) ? PQP_SPEED_NEVER_ARRIVES : 0);
    if (lane == 0) a.flags[b] = fl;
}

}  // namespace pqp
