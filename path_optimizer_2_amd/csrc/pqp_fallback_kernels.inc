// pqp_fallback_kernels.inc — instantiated by pqp_select.hip behind pqp_stitch_kernels.inc; includes pqp_driven_path.hpp, pqp_free_motion.hpp
// and pqp_wave.hpp for itself.  What the car does in a cycle that ends without a winner (pqp_fallback_rows, pqp_fallback_pick): it
// brakes along the plan it is already on - or, where there is no usable plan, along the arc it is on - at one of a few braking levels,
// the acceleration leaving the value the old plan had at the seam (column 6 of the stitch's state row) at a bounded jerk; the plans go
// through the agent check and the footprint check as they stand, and the pick takes the gentlest level that passes both.  The reference
// has no counterpart: it returns false and leaves the caller without a path.  include/pqp.h states both definitions operation by operation.
//
// fallback_rows_kernel: one wavefront per (group, level), four per workgroup, no LDS, no scratch, no atomics.
//   1  the state row and the level are read wave-uniform (scalar loads); a bad state zeroes the plan's rows and is done.  t1, ts, T, v1,
//      s1 and e(T) are the same in every lane
//   2  tiles of 64 rows of prev, one row per lane: whether the five columns read are numbers is a ballot, the maximum of the s column a
//      DPP maximum.  A group that is not stitched, or has fewer than two rows, reads none of them
//   3  tiles of 64 samples ascending, one sample per lane: the braking law in closed form, then the place.  On the plan sigma ascends
//      with the sample, so the s column is walked forward (walk_tile of pqp_driven_path.hpp, the trajectory's overload) by a
//      wave-uniform cursor, as sample_trajectory_kernel walks its t column: a tile of rows is taken while its last running maximum is
//      <= the sample tile's greatest sigma, and the cursor moves on where it is <= the sample tile's least.  A lane then gathers its
//      segment's two rows and places itself on the chord (chord_pose_at_station).  On the arc a lane takes ctra_functions at k0 e.  The
//      row of eight doubles is written by plain vector stores
//   4  stop_row is a count of ballots; the flags are wave-uniform
// fallback_pick_kernel: one wavefront per group.  The levels' verdicts are read wave-uniform and the decision is the same in every lane;
// the chosen rows - the winner's, a level's, or zeros - are copied 64 consecutive doubles at a time.
// A result depends on its own group, its level and the parameters alone.

#include "pqp_driven_path.hpp"
#include "pqp_free_motion.hpp"
#include "pqp_wave.hpp"

#include <climits>

namespace pqp {

constexpr int kFallbackThreads = 256;
constexpr long long kFallbackMaxBlocks = 1ll << 22;     // beyond that many workgroups a wavefront takes several plans in turn
constexpr int kFallbackMaxRows = INT_MAX - 64;          // M: a sample tile's f0 + lane stays inside an int

struct FallbackArgs {
    int groups, levels, mp, stride, r, M;
    double dt, a_cap;
    double level[PQP_FALLBACK_MAX_LEVELS][2];       // d, j
    const double* prev;              // [groups][mp][stride] or nullptr  x, y, heading, k, s at offsets 0 .. 4
    const int32_t* prev_m;           // [groups] or nullptr: all have mp
    const double* state;             // [groups][PQP_TRAJ_STRIDE]
    const int32_t* stitch_flags;     // [groups] or nullptr: all stitched
    double* rows;                    // [groups][levels][M][PQP_TRAJ_STRIDE]
    double* stop;                    // [groups][levels][2]
    int32_t* stop_row;               // [groups][levels]
    int32_t* flags;                  // [groups][levels]
};

// one braking plan, by a whole wavefront
__device__ __forceinline__ void fallback_plan(const FallbackArgs& a, long long item, int lane) {
#pragma clang fp contract(off)
    const int g = (int)(item / a.levels), l = (int)(item % a.levels);
    const int M = a.M, stride = a.stride;
    const double* __restrict__ st = a.state + (size_t)g * PQP_TRAJ_STRIDE;
    double* __restrict__ out = a.rows + (size_t)item * M * PQP_TRAJ_STRIDE;
    const double x0 = st[0], y0 = st[1], h0 = st[2], k0 = st[3], s_st = st[4], v0 = st[5], a_in = st[6];
    const int sf = a.stitch_flags ? a.stitch_flags[g] : PQP_STITCH_STITCHED;
    const bool bad = !(isfinite(x0) && isfinite(y0) && isfinite(h0) && isfinite(k0) && isfinite(s_st) && isfinite(v0) && isfinite(a_in)) || v0 < 0.0 ||
                     (sf & PQP_STITCH_BAD) != 0;
    if (bad) {
        const long long cells = (long long)M * PQP_TRAJ_STRIDE;
        for (long long e = lane; e < cells; e += 64) out[e] = 0.0;
        if (lane < 2) a.stop[(size_t)item * 2 + lane] = 0.0;
        if (lane == 0) { a.stop_row[item] = 0; a.flags[item] = PQP_FALLBACK_BAD; }
        return;
    }

    // ---- 1: the level's constants ------------------------------------------------------------------------------------------------------------
    const double d = a.level[l][0], j = a.level[l][1];
    const double a0 = fmin(fmax(a_in, -d), a.a_cap);
    const double t1 = (a0 + d) / j;
    const double ts = (a0 + sqrt(a0 * a0 + (2.0 * j) * v0)) / j;
    const bool in_ramp = ts <= t1;
    const double v1 = fmax(v0 + (a0 - (0.5 * j) * t1) * t1, 0.0);
    const double s1 = (v0 + (0.5 * a0 - (j * t1) / 6.0) * t1) * t1;
    const double u1 = v1 / d;
    const double T = in_ramp ? ts : t1 + u1;
    const double eT = fmax(in_ramp ? (v0 + (0.5 * a0 - (j * ts) / 6.0) * ts) * ts : s1 + (v1 - (0.5 * d) * u1) * u1, 0.0);

    // ---- 2: is there a plan to brake along --------------------------------------------------------------------------------------------------
    const double* __restrict__ prev = a.prev + (size_t)g * a.mp * stride;
    const int Mp = a.prev ? clamped_count(a.prev_m, g, a.mp) : 0;
    int fl = 0;
    bool arc = !(sf & PQP_STITCH_STITCHED) || Mp < 2;
    double s_top = -INFINITY;                    // the maximum of the s column
    if (!arc) {
        bool not_numbers = false;
        for (int i0 = 0; i0 < Mp; i0 += 64) {
            const int i = i0 + lane;
            double s = -INFINITY;
            if (i < Mp) {
                const double* r = prev + (size_t)i * stride;
                s = r[4];
                not_numbers = not_numbers || !(isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]) && isfinite(r[3]) && isfinite(s));
            }
            s_top = fmax(s_top, wave_max(s));
        }
        if (__ballot(not_numbers)) { arc = true; fl |= PQP_FALLBACK_BAD_PLAN; }
    }
    if (arc) fl |= PQP_FALLBACK_ARC;
    double sh0 = 0.0, ch0 = 1.0;
    if (arc) sincos(h0, &sh0, &ch0);
    const double* last = prev + (size_t)max(Mp - 1, 0) * stride;

    // ---- 3: the samples ----------------------------------------------------------------------------------------------------------------------
    int wt = 0;                                  // the tile of rows the walk stands in: every running maximum before it is <= every sigma to come
    double carry = -INFINITY;                    // the running maximum in front of that tile
    int moving = 0;
    bool beyond = false;
    for (int f0 = 0; f0 < M; f0 += 64) {
        const int f = f0 + lane;
        const bool valid = f < M;
        const double t = (double)(f / a.r) * a.dt + ((double)(f % a.r) * a.dt) / (double)a.r;
        double e, v, acc;
        if (t >= T) {
            e = eT; v = 0.0; acc = 0.0;
        } else if (t < t1) {
            e = (v0 + (0.5 * a0 - (j * t) / 6.0) * t) * t;
            v = v0 + (a0 - (0.5 * j) * t) * t;
            acc = a0 - j * t;
        } else {
            const double u = t - t1;
            e = s1 + (v1 - (0.5 * d) * u) * u;
            v = v1 - d * u;
            acc = -d;
        }
        e = fmin(fmax(e, 0.0), eT);
        v = fmax(v, 0.0);
        moving += __popcll(__ballot(valid && t < T));
        PathPose at;
        if (arc) {
            const double th = k0 * e;
            double sinc, cosc, f1, f2;
            ctra_functions(th, sinc, cosc, f1, f2);
            const double p = e * sinc, q = e * cosc;
            at = {x0 + (p * ch0 - q * sh0), y0 + (p * sh0 + q * ch0), constrain_angle(h0 + th), k0};
        } else {
            const double sigma = s_st + e;
            const double sigma_hi = wave_max(valid ? sigma : -INFINITY), sigma_lo = -wave_max(valid ? -sigma : -INFINITY);
            int cnt = min(wt * 64, Mp);
            int w = wt;
            double cw = carry;
            while (w * 64 < Mp) {
                double S_end;
                cnt += walk_tile(prev, stride, 4, Mp, w, cw, sigma, lane, &S_end);            // #{ i in this tile : S_i <= sigma }
                if (!(S_end <= sigma_hi)) break;
                ++w; cw = S_end;
                if (S_end <= sigma_lo) { wt = w; carry = cw; }
            }
            const int i = max(cnt - 1, 0);           // (cnt = 0: sigma lies in front of row 0, and the chord's lambda is 0 there)
            if (i < Mp - 1) {
                at = chord_pose_at_station(prev + (size_t)i * stride, stride, sigma);
            } else {
                at = {last[0], last[1], last[2], last[3]};
                beyond = beyond || (valid && sigma > s_top);
            }
        }
        if (valid) {
            double* o = out + (size_t)f * PQP_TRAJ_STRIDE;
            o[0] = at.x; o[1] = at.y; o[2] = at.heading; o[3] = at.k; o[4] = e; o[5] = v; o[6] = acc; o[7] = t;
        }
    }

    // ---- 4: the plan's records ---------------------------------------------------------------------------------------------------------------
    if (__ballot(beyond)) fl |= PQP_FALLBACK_PATH_SHORT;
    if (moving == M) fl |= PQP_FALLBACK_HORIZON;
    if (lane < 2) a.stop[(size_t)item * 2 + lane] = lane == 0 ? T : eT;
    if (lane == 0) { a.stop_row[item] = moving; a.flags[item] = fl; }
}

__global__ void __launch_bounds__(kFallbackThreads) fallback_rows_kernel(const FallbackArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long items = (long long)a.groups * a.levels;
    const long long step = (long long)gridDim.x * (kFallbackThreads / 64);
    for (long long item = (long long)blockIdx.x * (kFallbackThreads / 64) + wave; item < items; item += step) fallback_plan(a, item, lane);
}

struct FallbackPickArgs {
    int groups, levels, M;
    const int32_t* best;             // [groups] or nullptr: every group falls back
    const double* best_traj;         // [groups][M][PQP_TRAJ_STRIDE] or nullptr
    const int32_t* best_m;           // [groups] or nullptr
    const double* rows;              // [groups][levels][M][PQP_TRAJ_STRIDE]
    const int32_t* row_flags;        // [groups][levels]
    const int32_t* first_hit;        // [groups * levels] or nullptr
    const int32_t* first_collision;  // [groups * levels] or nullptr
    double* final_traj;              // [groups][M][PQP_TRAJ_STRIDE]
    int32_t* final_m;                // [groups]
    int32_t* level;                  // [groups]
    int32_t* flags;                  // [groups]
};

__global__ void __launch_bounds__(kFallbackThreads) fallback_pick_kernel(const FallbackPickArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long step = (long long)gridDim.x * (kFallbackThreads / 64);
    const int M = a.M, L = a.levels;
    const long long cells = (long long)M * PQP_TRAJ_STRIDE;
    for (long long g = (long long)blockIdx.x * (kFallbackThreads / 64) + wave; g < a.groups; g += step) {
        const double* src = nullptr;
        int count = 0, lv = -1, fl = 0;
        if (a.best && a.best[g] >= 0) {
            if (a.best_traj) { src = a.best_traj + (size_t)g * cells; count = a.best_m[g]; }
        } else {
            const size_t first = (size_t)g * L;
            int gentlest = -1, latest = 0, latest_at = INT_MIN;          // (a verdict is read as it is: a negative one is the earliest contact)
            bool bad = false;
            for (int l = 0; l < L; ++l) {
                const int rf = a.row_flags[first + l];
                const int hit = a.first_hit ? a.first_hit[first + l] : M, col = a.first_collision ? a.first_collision[first + l] : M;
                const int contact = min(hit, col);
                bad = bad || (rf & PQP_FALLBACK_BAD) != 0;
                if (gentlest < 0 && !(rf & (PQP_FALLBACK_BAD | PQP_FALLBACK_PATH_SHORT)) && hit == M && col == M) gentlest = l;
                if (contact >= latest_at) { latest_at = contact; latest = l; }
            }
            if (bad) {
                fl = PQP_FALLBACK_BAD;
            } else {
                lv = gentlest >= 0 ? gentlest : latest;
                fl = a.row_flags[first + lv] | PQP_FALLBACK_TAKEN | (gentlest >= 0 ? 0 : PQP_FALLBACK_NOT_CLEAR);
                src = a.rows + (first + lv) * (size_t)cells;
                count = M;
            }
        }
        double* __restrict__ out = a.final_traj + (size_t)g * cells;
        for (long long e = lane; e < cells; e += 64) out[e] = src ? src[e] : 0.0;
        if (lane == 0) { a.final_m[g] = count; a.level[g] = lv; a.flags[g] = fl; }
    }
}

}  // namespace pqp
