// pqp_stitch_kernels.inc — instantiated by pqp_select.hip behind pqp_select_kernels.inc (whose group_rows it reads group_start with);
// includes pqp_free_motion.hpp.  The start of a planning cycle from the previous cycle's plan (pqp_stitch_trajectory): per group the
// previous plan's rows - pqp_select_plans' best_traj as it lies -, a measured state and the time since that plan began become the state
// the new cycle plans from, the verdict, the deviations, the re-based piece of the old plan that leads to the start, and the same start
// spread over the group's candidates in the arrays pqp_optimize_path_device and pqp_speed_profile read.  The reference has no
// counterpart: it plans one path per call from the state it is given.  include/pqp.h states the definition operation by operation.
//
// stitch_trajectory_kernel: one launch, one wavefront per group, four per workgroup, no LDS, no scratch, no atomics.
//   1  the measurement is read wave-uniform; a bad one zeroes the group's outputs and is done
//   2  tiles of 64 rows, one row per lane (t, x, y: three of a row's eight doubles, the rows 64 B apart with stride 8): the two time
//      matches are ballots, the first set bit of the first tile that has one; the running least squared distance is a DPP minimum per
//      tile, taken over with a strict <, and a ballot of the lanes that hold it gives the lowest index.  Nothing caps m
//   3  the matched rows are read wave-uniform (scalar loads), the deviations, the flags and the verdict are the same in every lane; a
//      replanned group advances its measurement by the free model, every lane the same
//   4  the state row and the prefix are written 64 consecutive doubles at a time, a lane re-basing its element when its column is s or t
//   5  lanes stride over the group's candidates
// A group's result depends on its own inputs alone.

#include "pqp_free_motion.hpp"

namespace pqp {

constexpr int kStitchThreads = 256;
constexpr long long kStitchMaxBlocks = 1ll << 22;       // beyond that many workgroups a wavefront takes several groups in turn

struct StitchArgs {
    int groups, m, stride, batch, keep, prefix_max;
    double t_ahead, lat_max, lon_max, dh_max, v_still, v_cap;
    const double* prev;              // [groups][m][stride]  x, y, heading, k, s, v, a, t at offsets 0 .. 7
    const int32_t* m_of;             // [groups] or nullptr: all have m
    const double* meas;              // [groups][6]  x, y, heading, v, a, yaw rate
    const double* t_now;             // [groups]
    const int32_t* group_start;      // [groups + 1] or nullptr: candidate g is group g's
    double* state;                   // [groups][PQP_TRAJ_STRIDE]
    int32_t* flags;                  // [groups]
    double* dev;                     // [groups][3]
    int32_t* idx;                    // [groups][3]
    double* prefix;                  // [groups][prefix_max][PQP_TRAJ_STRIDE] or nullptr
    int32_t* prefix_n;               // [groups]
    double* start;                   // [batch][3] or nullptr
    double* start_k;                 // [batch] or nullptr
    double* v_start;                 // [batch] or nullptr
};

// whether the eight columns of a row are numbers
__device__ __forceinline__ bool stitch_row_finite(const double* r) {
    return isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]) && isfinite(r[3]) && isfinite(r[4]) && isfinite(r[5]) && isfinite(r[6]) && isfinite(r[7]);
}

// element `lane` of a row of eight, for the lanes below 8
__device__ __forceinline__ double stitch_pick(int lane, double e0, double e1, double e2, double e3, double e4, double e5, double e6, double e7) {
    return lane == 0 ? e0 : lane == 1 ? e1 : lane == 2 ? e2 : lane == 3 ? e3 : lane == 4 ? e4 : lane == 5 ? e5 : lane == 6 ? e6 : e7;
}

// one group, by a whole wavefront
__device__ __forceinline__ void stitch_group(const StitchArgs& a, int g, int lane) {
#pragma clang fp contract(off)
    const double* __restrict__ rows = a.prev + (size_t)g * a.m * a.stride;
    const double* __restrict__ ms = a.meas + (size_t)g * 6;
    const int stride = a.stride;
    const int M = clamped_count(a.m_of, g, a.m);
    const double x = ms[0], y = ms[1], hd = ms[2], v = ms[3], acc = ms[4], om = ms[5], t_now = a.t_now[g];

    int flags = 0, i_now = -1, p = -1, i_start = -1, i0 = 0, count = 0;
    double lon = 0.0, lat = 0.0, dh = 0.0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;          // the state row
    const bool bad = !(isfinite(x) && isfinite(y) && isfinite(hd) && isfinite(v) && isfinite(acc) && isfinite(om) && isfinite(t_now)) || v < 0.0;
    const double tq = t_now + a.t_ahead;
    if (bad) {
        flags = PQP_STITCH_BAD;
    } else if (M < 2) {
        flags = PQP_STITCH_NO_PREVIOUS;
    } else {
        // ---- 2: the time matches and the nearest row ----------------------------------------------------------------------------------------
        double least = INFINITY;
        for (int f0 = 0; f0 < M; f0 += 64) {
            const int f = f0 + lane;
            const bool in = f < M;
            const double* r = rows + (size_t)(in ? f : 0) * stride;
            const double t = r[7], ex = x - r[0], ey = y - r[1];
            if (i_now < 0) {
                const unsigned long long at = __ballot(in && t >= t_now);
                if (at) i_now = f0 + __builtin_ctzll(at);
            }
            if (i_start < 0) {
                const unsigned long long at = __ballot(in && t >= tq);
                if (at) i_start = f0 + __builtin_ctzll(at);
            }
            double d2 = ex * ex + ey * ey;
            if (!in || !isfinite(d2)) d2 = INFINITY;
            const double tile_least = wave_read<63>(wave_prefix_min(d2));
            if (tile_least < least) {
                least = tile_least;
                p = f0 + __builtin_ctzll(__ballot(d2 == tile_least));
            }
        }
        if (t_now < rows[7] || i_start < 0) flags |= PQP_STITCH_TIME;
        // ---- 3: the matched rows, the deviations --------------------------------------------------------------------------------------------
        bool numbers = p >= 0 && stitch_row_finite(rows + (size_t)p * stride);
        if (i_now >= 0) numbers = numbers && stitch_row_finite(rows + (size_t)i_now * stride);
        if (i_now >= 1) numbers = numbers && stitch_row_finite(rows + (size_t)(i_now - 1) * stride);
        if (i_start >= 0) numbers = numbers && stitch_row_finite(rows + (size_t)i_start * stride);
        if (!numbers) flags |= PQP_STITCH_BAD_PLAN;
        if (numbers && i_now >= 0) {
            const double* rp = rows + (size_t)p * stride;
            double sh, ch;
            sincos(rp[2], &sh, &ch);
            const double dx = x - rp[0], dy = y - rp[1];                         // global2Local((x_p, y_p, heading_p), the measured point)
            lat = -dx * sh + dy * ch;
            double s_ref = rows[4];
            if (i_now > 0) {
                const double* r1 = rows + (size_t)i_now * stride;
                const double* r0 = r1 - stride;
                s_ref = r0[4] + (r1[4] - r0[4]) * ((t_now - r0[7]) / (r1[7] - r0[7]));
            }
            lon = s_ref - (rp[4] + (dx * ch + dy * sh));
            dh = constrain_angle(hd - rp[2]);
            if (!(fabs(lat) <= a.lat_max)) flags |= PQP_STITCH_LATERAL;
            if (!(fabs(lon) <= a.lon_max)) flags |= PQP_STITCH_LONGITUDINAL;
            if (!(fabs(dh) <= a.dh_max)) flags |= PQP_STITCH_HEADING;
        }
    }

    // ---- the verdict, the state row ---------------------------------------------------------------------------------------------------------
    if (!bad) {
        if (flags & (PQP_STITCH_NO_PREVIOUS | PQP_STITCH_TIME | PQP_STITCH_BAD_PLAN | PQP_STITCH_LATERAL | PQP_STITCH_LONGITUDINAL | PQP_STITCH_HEADING)) {
            flags |= PQP_STITCH_REPLAN;
            double te, ve, px, py, ph, sh0, ch0;
            bool stops = false, capped = false;
            free_speed(v, acc, a.v_cap, a.t_ahead, te, ve, stops, capped);
            const double tc = a.t_ahead - te;
            sincos(hd, &sh0, &ch0);
            free_pose(x, y, hd, sh0, ch0, v, acc, om, te, ve, tc, px, py, ph);
            s0 = px; s1 = py; s2 = ph;
            s3 = ve > a.v_still ? om / ve : 0.0;
            s4 = 0.0; s5 = ve;
            s6 = (stops || capped) ? 0.0 : acc;
            s7 = tq;
            if (ve == 0.0) flags |= PQP_STITCH_STANDING;
            count = 1;
        } else {
            flags |= PQP_STITCH_STITCHED;
            const double* rs = rows + (size_t)i_start * stride;
            s0 = rs[0]; s1 = rs[1]; s2 = rs[2]; s3 = rs[3]; s4 = rs[4]; s5 = rs[5]; s6 = rs[6]; s7 = rs[7];
            i0 = max(0, i_now - a.keep);
            if (a.prefix && i_start - i0 + 1 > a.prefix_max) {
                i0 = i_start - a.prefix_max + 1;
                flags |= PQP_STITCH_PREFIX_CUT;
            }
            count = i_start - i0 + 1;
        }
    }
    const bool stitched = (flags & PQP_STITCH_STITCHED) != 0;

    // ---- 4: the group's records ---------------------------------------------------------------------------------------------------------------
    if (lane < PQP_TRAJ_STRIDE) a.state[(size_t)g * PQP_TRAJ_STRIDE + lane] = stitch_pick(lane, s0, s1, s2, s3, s4, s5, s6, s7);
    if (lane < 3) {
        a.dev[(size_t)g * 3 + lane] = lane == 0 ? lon : lane == 1 ? lat : dh;
        a.idx[(size_t)g * 3 + lane] = lane == 0 ? i_now : lane == 1 ? p : i_start;
    }
    if (lane == 0) {
        a.flags[g] = flags;
        a.prefix_n[g] = count;
    }
    if (a.prefix) {
        double* __restrict__ out = a.prefix + (size_t)g * a.prefix_max * PQP_TRAJ_STRIDE;
        const long long total = (long long)a.prefix_max * PQP_TRAJ_STRIDE;
        for (long long e = lane; e < total; e += 64) {
            const long long j = e >> 3;
            const int col = (int)(e & 7);
            double w = 0.0;
            if (j < count) {
                if (stitched) {
                    w = rows[(size_t)(i0 + j) * stride + col];
                    if (col == 4) w = w - s4;
                    if (col == 7) w = w - s7;
                } else {
                    w = col == 7 ? 0.0 : stitch_pick(col, s0, s1, s2, s3, s4, s5, s6, s7);
                }
            }
            out[e] = w;
        }
    }

    // ---- 5: the group's candidates ---------------------------------------------------------------------------------------------------------------
    int lo = min(g, a.batch), hi = min(g + 1, a.batch);
    if (a.group_start) group_rows(a.group_start, g, a.batch, &lo, &hi);
    for (int b = lo + lane; b < hi; b += 64) {
        if (a.start) {
            double* o = a.start + (size_t)b * 3;
            o[0] = s0; o[1] = s1; o[2] = s2;
        }
        if (a.start_k) a.start_k[b] = s3;
        if (a.v_start) a.v_start[b] = s5;
    }
}

__global__ void __launch_bounds__(kStitchThreads) stitch_trajectory_kernel(const StitchArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long step = (long long)gridDim.x * (kStitchThreads / 64);
    for (long long g = (long long)blockIdx.x * (kStitchThreads / 64) + wave; g < a.groups; g += step) stitch_group(a, (int)g, lane);
}

}  // namespace pqp
