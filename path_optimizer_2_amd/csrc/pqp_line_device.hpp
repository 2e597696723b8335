// pqp_line_device.hpp — device helpers that several kernel families share: the line's spline table (tk::spline::operator() / deriv,
// src/tools/spline.cpp:251-318), Map::getObstacleDistance (src/tools/Map.cpp:16-22), getCurvature and getProjection (src/tools/tools.cpp).
// All __device__ __forceinline__; the arithmetic is kept in the reference's operation order with FMA contraction off.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pqp.h"

namespace pqp {

struct SplineView {
    const double *x, *y, *a, *b, *c;
    double b0, c0;
    int m;
};

__device__ __forceinline__ int spline_segment(const SplineView& s, double v) {      // std::lower_bound - 1, clamped at 0
    int lo = 0, hi = s.m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s.x[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo - 1 > 0 ? lo - 1 : 0;
}

__device__ __forceinline__ void spline_eval3(const SplineView& s, double v, double& f, double& d1, double& d2) {
#pragma clang fp contract(off)
    const int n = s.m;
    const int idx = spline_segment(s, v);
    const double h = v - s.x[idx];
    if (v < s.x[0]) {
        f = (s.b0 * h + s.c0) * h + s.y[0];
        d1 = 2.0 * s.b0 * h + s.c0;
        d2 = 2.0 * s.b0 * h;                       // sic: the reference's left-extrapolated second derivative (spline.cpp:288)
    } else if (v > s.x[n - 1]) {
        f = (s.b[n - 1] * h + s.c[n - 1]) * h + s.y[n - 1];
        d1 = 2.0 * s.b[n - 1] * h + s.c[n - 1];
        d2 = 2.0 * s.b[n - 1];
    } else {
        f = ((s.a[idx] * h + s.b[idx]) * h + s.c[idx]) * h + s.y[idx];
        d1 = (3.0 * s.a[idx] * h + 2.0 * s.b[idx]) * h + s.c[idx];
        d2 = 6.0 * s.a[idx] * h + 2.0 * s.b[idx];
    }
}

// a / b, correctly rounded, from y = 1 / b rounded to nearest: the quotient by the reciprocal, corrected twice with the exact residual a - b q
// (fused multiply-add).  After the first correction q is within half an ulp and a bit of a / b, and the second one then rounds to the nearest
// double (Markstein's theorem; 520 M random and cell-boundary cases against `/` with 13 divisors: 0 mismatches already after one correction).
// Five instructions where the IEEE division sequence (two scalings, rcp, Newton steps, fix-ups) takes ~15: a map sample divides four times by the
// cell size, and the kernels around the map are bound by VALU issue.  Differs from `/` only in the sign of a zero quotient.
__device__ __forceinline__ double exact_div(double a, double b, double y) {
    double q = a * y;
    q = fma(fma(-b, q, a), y, q);
    return fma(fma(-b, q, a), y, q);
}

// GridMap::getPosition along one axis: the centre of the cell with index `index`, of a map centred at `pos` with extent `length`.  The one
// text of it: obstacle_distance below and overlay_kernel (pqp_overlay_kernels.inc) place their cells by it.
__device__ __forceinline__ double cell_centre(double pos, double length, double resolution, int index) {
#pragma clang fp contract(off)
    return (pos + (0.5 * length - 0.5 * resolution)) + resolution * (double)(-index);
}

// grid_map_core 1.6.x: isInside, getIndex, getPosition, atPositionLinearInterpolated, nearest fallback (restated from the
// published sources; oracle/corridor_oracle.py carries the same restatement and the notes on its border behaviour)
__device__ __forceinline__ double obstacle_distance(const float* __restrict__ dist, const pqp_grid_geometry& g, double px, double py) {
#pragma clang fp contract(off)
    const double tx = -(px - g.pos_x - 0.5 * g.length_x), ty = -(py - g.pos_y - 0.5 * g.length_y);
    if (!(tx >= 0.0 && ty >= 0.0 && tx < g.length_x && ty < g.length_y)) return 0.0;
    const double inv_res = 1.0 / g.resolution;           // (the same for every sample of the kernel: hoisted by the compiler)
    const int i0x = -(int)exact_div(px - 0.5 * g.length_x - g.pos_x, g.resolution, inv_res);
    const int i0y = -(int)exact_div(py - 0.5 * g.length_y - g.pos_y, g.resolution, inv_res);
    const double cx = cell_centre(g.pos_x, g.length_x, g.resolution, i0x), cy = cell_centre(g.pos_y, g.length_y, g.resolution, i0y);
    const bool dirx = px >= cx, diry = py >= cy;
    const int i1x = dirx ? i0x - 1 : i0x + 1;          // indices[1] = (i1x, i0y), indices[2] = (i0x, i2y), indices[3] = (i1x, i2y)
    const int i2y = diry ? i0y - 1 : i0y + 1;
    // idxShift: which of the four cells is f[0] (the one whose centre is the interpolation origin), f[1] (+x), f[2] (+y), f[3]
    int fx[4], fy[4];
    const int ax = dirx ? i0x : i1x, bx = dirx ? i1x : i0x;       // ax: cell at relative x = 0, bx: at relative x = 1
    const int ay = diry ? i0y : i2y, by = diry ? i2y : i0y;
    fx[0] = ax; fy[0] = ay; fx[1] = bx; fy[1] = ay; fx[2] = ax; fy[2] = by; fx[3] = bx; fy[3] = by;
    // (32-bit: the entry points refuse maps of 2^30 cells and more; the indices are within one cell of the map, the point being inside it)
    const int end_lin = g.rows * g.cols;
    int lin[4];
    float f[4];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lin[k] = fy[k] * g.rows + fx[k];                              // column-major linear index; negative = huge size_t upstream
        const bool in = lin[k] >= 0 && lin[k] < end_lin;
        ok = ok && in;
        lin[k] = in ? lin[k] : 0;
    }
    // all four cells in flight at once (a cell outside the layer reads cell 0 instead of branching around the load: four dependent
    // round trips to L2 per sample became one)
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = dist[lin[k]];
    if (!ok) return (double)dist[i0y * g.rows + i0x];                // INTER_NEAREST fallback of GridMap::atPosition
    const double qx = cell_centre(g.pos_x, g.length_x, g.resolution, ax), qy = cell_centre(g.pos_y, g.length_y, g.resolution, ay);
    const double rx = exact_div(px - qx, g.resolution, inv_res), ry = exact_div(py - qy, g.resolution, inv_res);
    const double ux = 1.0 - rx, uy = 1.0 - ry;
    const double v = (double)f[0] * ux * uy + (double)f[1] * rx * uy + (double)f[2] * ux * ry + (double)f[3] * rx * ry;
    return (double)(float)v;
}

// getCurvature (tools.cpp:38-44): (x' y'' - y' x'') / pow(x'^2 + y'^2, 1.5).  v * sqrt(v) is within an ulp of pow(v, 1.5), as
// libm's pow is of ocml's; the walk below evaluates it at every step, where a double-precision pow would dominate.
__device__ __forceinline__ double curvature_of(double dx, double dy, double ddx, double ddy) {
#pragma clang fp contract(off)
    const double v = dx * dx + dy * dy;
    return (dx * ddy - dy * ddx) / (v * sqrt(v));
}

// getProjection (src/tools/tools.cpp:66-96) with getProjectionByNewton (:98-126): the abscissa of the point of the line nearest to
// (tx, ty) - a 1 m grid search from 0, the end point, then Newton on the squared distance (20 steps, |ds| < 1e-5), clipped to the length.
// Computed by a whole wavefront (every lane of it calls this, every lane gets the result): the coarse scan at 1 m steps - up to 40 spline
// evaluations in a row for one lane - is one evaluation per lane; the first minimum wins as in a serial scan from 0 with a strict `<`
// (its abscissae 0, 1, 2, ... are exact in both forms), the Newton iterations run redundantly on all lanes.
__device__ __forceinline__ double spline_projection_wave(const SplineView& sx, const SplineView& sy, double tx, double ty, double length) {
#pragma clang fp contract(off)
    if (!(length > 0.0)) return 0.0;
    const int lane = threadIdx.x & 63;
    double best_s = 0.0, best = 1.7976931348623157e308;
    for (int base = 0; (double)base <= length; base += 64) {
        const int k = base + lane;
        const double tmp = (double)k;
        double d = 1.7976931348623157e308;
        if (tmp <= length) {
            double x, y, d1, d2;
            spline_eval3(sx, tmp, x, d1, d2); spline_eval3(sy, tmp, y, d1, d2);
            d = sqrt((x - tx) * (x - tx) + (y - ty) * (y - ty));
        }
        int kk = k;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __shfl_xor(d, off, 64);
            const int ok = __shfl_xor(kk, off, 64);
            if (od < d || (od == d && ok < kk)) { d = od; kk = ok; }
        }
        if (d < best) { best = d; best_s = (double)kk; }
    }
    double xe, ye, d1, d2;
    spline_eval3(sx, length, xe, d1, d2); spline_eval3(sy, length, ye, d1, d2);
    if (sqrt((xe - tx) * (xe - tx) + (ye - ty) * (ye - ty)) < best) return length;
    double cur = fmin(best_s, length), prev = cur;
    for (int it = 0; it < 20; ++it) {
        double x, dx, ddx, y, dy, ddy;
        spline_eval3(sx, cur, x, dx, ddx); spline_eval3(sy, cur, y, dy, ddy);
        const double j = (x - tx) * dx + (y - ty) * dy;
        const double h = dx * dx + (x - tx) * ddx + dy * dy + (y - ty) * ddy;
        cur -= j / h;
        if (fabs(cur - prev) < 1e-5) break;
        prev = cur;
    }
    return fmin(cur, length);
}

}  // namespace pqp
