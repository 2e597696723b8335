// pqp_driven_path.hpp - what the kernels of pqp_maps.hip, pqp_agents.hip, pqp_speed.hip and pqp_select.hip share about a solved path and
// its speed profile, each .inc including it for itself: the count an optional array gives an item, how many of a path's waypoints are
// driven, whether a driven row holds numbers, the walk along a monotone column of the profile and the pose on a chord between two
// waypoints.  include/pqp.h states each of them once, operation by operation; this is the one place the kernels state them.  Device code
// only.  Every function is forced inline, and those that compute keep fp contraction off: a fused multiply-add here breaks bit equality
// with the definition.
#pragma once
#include "pqp_path_lane.hpp"
#include "pqp_wave.hpp"

namespace pqp {

// the count an optional per-item array gives item b, inside 0 .. full; no array: full
__device__ __forceinline__ int clamped_count(const int32_t* of, long long b, int full) { return of ? min(max(of[b], 0), full) : full; }

// the driven count: of a path's `count` waypoints (clamped_count of n_of), those in front of stop_before[b]
__device__ __forceinline__ int driven_count(int count, const int32_t* stop_before, long long b) {
    return stop_before ? min(count, max(stop_before[b], 0)) : count;
}

// "what is read must be numbers": x, y, heading, k of a path row and s, v, a of its profile row.  A kernel adds what else it reads.
__device__ __forceinline__ bool row_not_finite(const double* r, const double* o) {
    return !isfinite(r[0]) || !isfinite(r[1]) || !isfinite(r[2]) || !isfinite(r[5]) || !isfinite(o[0]) || !isfinite(o[1]) || !isfinite(o[2]);
}

// One tile of the walk along a column of the profile (0: s, 3: t), by a whole wavefront: M_i is the running maximum of the column up to
// waypoint i - a DPP prefix minimum of the negated column, which is exact, on top of `carry`, the maximum in front of tile w - and the
// lane's answer is #{ i in tile w, i < c : M_i <= bound }, by a binary search across the lanes, which with a monotone M is that count.
// *last is the tile's last M: the next tile's carry, and what the caller's loop control looks at.
__device__ __forceinline__ int walk_tile(const double* __restrict__ prof, int col, int c, int w, double carry, double bound, int lane, double* last) {
#pragma clang fp contract(off)
    const int i = w * 64 + lane;
    const int nv = min(64, c - w * 64);
    const double neg = i < c ? -prof[(size_t)i * PQP_SPEED_STRIDE + col] : INFINITY;
    const double M = fmax(carry, -wave_prefix_min(neg));                                  // lanes behind the count repeat the last M
    int pos = 0;
#pragma unroll
    for (int step = 64; step >= 1; step >>= 1) {
        const int at = pos + step - 1;
        const double Mv = __shfl(M, at & 63);
        if (at < nv && Mv <= bound) pos += step;
    }
    *last = wave_read<63>(M);
    return pos;
}

// The same tile of the same walk along column `col` of rows that lie `stride` doubles apart: a trajectory's rows (PQP_TRAJ_STRIDE's
// columns, s at 4), which have their own stride where the profile's is PQP_SPEED_STRIDE.
__device__ __forceinline__ int walk_tile(const double* __restrict__ rows, int stride, int col, int c, int w, double carry, double bound, int lane,
                                         double* last) {
#pragma clang fp contract(off)
    const int i = w * 64 + lane;
    const int nv = min(64, c - w * 64);
    const double neg = i < c ? -rows[(size_t)i * stride + col] : INFINITY;
    const double M = fmax(carry, -wave_prefix_min(neg));
    int pos = 0;
#pragma unroll
    for (int step = 64; step >= 1; step >>= 1) {
        const int at = pos + step - 1;
        const double Mv = __shfl(M, at & 63);
        if (at < nv && Mv <= bound) pos += step;
    }
    *last = wave_read<63>(M);
    return pos;
}

struct PathPose { double x, y, heading, k; };

// a waypoint itself: the last driven one, where there is no chord to stand on
__device__ __forceinline__ PathPose waypoint_pose(const double* r) { return {r[0], r[1], r[2], r[5]}; }

// the pose on the chord of length d from path row r0 to the row behind it, e = min(max(want, 0), d) along it; *e_out is that e
__device__ __forceinline__ PathPose chord_pose(const double* r0, int stride, double want, double* e_out) {
#pragma clang fp contract(off)
    const double* r1 = r0 + stride;
    const double x0 = r0[0], y0 = r0[1], h0 = r0[2], c0 = r0[5], x1 = r1[0], y1 = r1[1], h1 = r1[2], c1 = r1[5];
    const double dx = x1 - x0, dy = y1 - y0;
    const double d = sqrt(dx * dx + dy * dy);
    const double e = fmin(fmax(want, 0.0), d);
    const double lam = d > 0.0 ? e / d : 0.0;
    *e_out = e;
    return {x0 + lam * dx, y0 + lam * dy, constrain_angle(h0 + lam * constrain_angle(h1 - h0)), c0 + lam * (c1 - c0)};
}

// the same chord expressions between trajectory row r0 (x, y, heading, k, s at 0 .. 4) and the row behind it, the place on the chord
// given by the station: lam = (sigma - s0) / (s1 - s0) inside [0, 1], and 0 where s does not grow along the segment
__device__ __forceinline__ PathPose chord_pose_at_station(const double* r0, int stride, double sigma) {
#pragma clang fp contract(off)
    const double* r1 = r0 + stride;
    const double x0 = r0[0], y0 = r0[1], h0 = r0[2], c0 = r0[3], s0 = r0[4], x1 = r1[0], y1 = r1[1], h1 = r1[2], c1 = r1[3], s1 = r1[4];
    const double dx = x1 - x0, dy = y1 - y0, ds = s1 - s0;
    const double lam = ds > 0.0 ? fmin(fmax((sigma - s0) / ds, 0.0), 1.0) : 0.0;
    return {x0 + lam * dx, y0 + lam * dy, constrain_angle(h0 + lam * constrain_angle(h1 - h0)), c0 + lam * (c1 - c0)};
}

}  // namespace pqp
