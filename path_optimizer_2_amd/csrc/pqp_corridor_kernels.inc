// pqp_corridor_kernels.inc — included by pqp_kernels.hip.  Corridor bounds of every waypoint from the obstacle distance map
// (SURVEY.md §8f rank 1): the step that produces the `bounds` input of the path QP.
//   ReferencePathImpl::updateBoundsImproved            src/data_struct/reference_path_impl.cpp:177-230
//   ReferencePathImpl::getClearanceWithDirectionStrict src/data_struct/reference_path_impl.cpp:232-312
//   Map::getObstacleDistance                           src/tools/Map.cpp:16-22   (grid_map_core isInside + atPosition(INTER_LINEAR))
//   getDirectionalProjectionByNewton                   src/tools/tools.cpp:156-189
//   tk::spline::operator() / deriv                     src/tools/spline.cpp:251-318
// One workgroup per scenario, one lane per (waypoint, circle): circle 0 = front, 1 = rear, 2 = centre.  Every lane walks its
// own ray through the distance map (<= 2 x (20 + 5) bilinear samples of 4 floats, L2-resident map), so the kernel is a
// latency-bound gather; the arithmetic is kept in the reference's operation order with FMA contraction off, so that apart
// from sin/cos (ocml vs libm) every sample position, hence every step count, is the reference's.

namespace pqp {

struct CorridorArgs {
    int batch, n, m;                 // scenarios, waypoints, spline knots
    int tile;                        // waypoints the kernel holds in LDS at a time (n when a whole scenario fits; long paths go through in tiles)
    const double* ref;               // [batch][n][5]  s, k, heading, x, y
    const double* spl;               // [batch][9][m]  knots; y, a, b, c of x(s); y, a, b, c of y(s)
    const double* spl_ext;           // [batch][4]     b0, c0 of x(s); b0, c0 of y(s)   (left extrapolation)
    const float* dist;               // [n_maps][cols][rows]  the "distance" layer, column major like Eigen::MatrixXf
    const int32_t* map_of;           // [batch] map index per scenario, or nullptr: all scenarios use map 0
    pqp_grid_geometry g;
    pqp_corridor_params p;
    const int32_t* n_of;             // [batch] waypoints of each scenario (<= n), or nullptr: all have n
    double* bounds;                  // [batch][n][6]  f_lb f_ub r_lb r_ub c_lb c_ub
    int32_t* n_valid;                // [batch] index of the first blocked waypoint (its own count: none)
};

struct RefStatesArgs {
    int batch, n_max, m;
    const double* spl;               // [batch][9][m]
    const double* spl_ext;           // [batch][4]
    const double* max_s;             // [batch] length of the reference line
    const double* start;             // [batch][3] vehicle start state x, y, heading, or nullptr
    double ds_small, ds_large;
    int dynamic;
    double* ref;                     // [batch][n_max][5]  s, k, heading, x, y
    int32_t* count;                  // [batch] states the loop produces (may exceed n_max: then only n_max rows were written)
    double* init_err;                // [batch][2] initial offset, initial heading error (needs start), or nullptr
    // dynamic == 2: ReferencePathSmoother::segmentRawReference (reference_path_smoother.cpp:48-85): abscissae 0, ds, 2 ds, ... up to
    // and including the first one >= max_s; curvature with pow(., 1.5); outputs as the five lists the smoother QPs take
    double *lx, *ly, *ls, *langle, *lk;          // [batch][n_max] each (only when dynamic == 2)
};

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
// cell size, and the kernels around the map are bound by VALU issue (DESIGN.md 8.0).  Differs from `/` only in the sign of a zero quotient.
__device__ __forceinline__ double exact_div(double a, double b, double y) {
    double q = a * y;
    q = fma(fma(-b, q, a), y, q);
    return fma(fma(-b, q, a), y, q);
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
    const double ox = 0.5 * g.length_x - 0.5 * g.resolution, oy = 0.5 * g.length_y - 0.5 * g.resolution;
    const double cx = (g.pos_x + ox) + g.resolution * (double)(-i0x), cy = (g.pos_y + oy) + g.resolution * (double)(-i0y);
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
    const double qx = (g.pos_x + ox) + g.resolution * (double)(-ax), qy = (g.pos_y + oy) + g.resolution * (double)(-ay);
    const double rx = exact_div(px - qx, g.resolution, inv_res), ry = exact_div(py - qy, g.resolution, inv_res);
    const double ux = 1.0 - rx, uy = 1.0 - ry;
    const double v = (double)f[0] * ux * uy + (double)f[1] * rx * uy + (double)f[2] * ux * ry + (double)f[3] * rx * ry;
    return (double)(float)v;
}

// Layout of the kernel's dynamic LDS in doubles; n = waypoints held at a time (CorridorArgs::tile), tasks = (waypoint, circle)
struct CorridorLds {
    int m, n;
    __host__ __device__ int spl() const { return 0; }                      // [9][m]   the scenario's spline table
    __host__ __device__ int acc() const { return 9 * m; }                  // [32]     delta_s added j + 1 times (the reference accumulates)
    __host__ __device__ int org() const { return acc() + 32; }             // [3n][8]  probe origin x, y; offset; cos, sin of the left normal; of the right; ok
    __host__ __device__ int cend() const { return org() + 3 * n * 8; }     // [3n][2]  bound after the coarse walk, per side
    __host__ __device__ int first() const { return cend() + 3 * n * 2; }   // int [3n][2]  first failing coarse step, then first failing fine step
    __host__ __device__ size_t total_bytes() const { return (size_t)first() * 8 + (size_t)3 * n * 2 * 4; }
};

// ReferencePathImpl::updateBoundsOnInputStates (src/data_struct/reference_path_impl.cpp:118-175) is the same walk, with the front and rear
// circle centres moved to where the planned heading error d_heading of input state i puts them (states_bounds_kernel below).
//
// One workgroup per scenario.  The reference walks every ray sample by sample (the first sample closer than 0.5 m to an obstacle
// ends the walk); here all candidate samples of all rays of the scenario are gathered in parallel and the first failing one is
// found with an LDS atomicMin: about twice the samples, but one gather latency per round instead of a chain of up to 25.  Every
// sample position is the reference's expression of the same accumulated step lengths, so the result is the walk's.
__global__ void __launch_bounds__(1024) corridor_bounds_kernel(const CorridorArgs a) {
#define PQP_CORRIDOR_ON_STATES 0
#include "pqp_corridor_body.inc"
#undef PQP_CORRIDOR_ON_STATES
}

// states [batch][a.n][stride]: d_heading at offset 4 (a path solve's `out` in place with stride 7); a.n_of: the states of each scenario.
// (named apart from corridor_bounds_kernel: tests/test_kernel_resources.py finds that one by a substring of its name)
__global__ void __launch_bounds__(1024) states_bounds_kernel(const CorridorArgs a, const double* __restrict__ states, int stride) {
#define PQP_CORRIDOR_ON_STATES 1
#include "pqp_corridor_body.inc"
#undef PQP_CORRIDOR_ON_STATES
}

// Reference states from the spline of the reference line + the initial error of the vehicle (SURVEY.md 8f rank 2):
//   ReferencePathImpl::buildReferenceFromSpline  src/data_struct/reference_path_impl.cpp:314-338   (sequential in s: the next
//       step length depends on the curvature just computed -> one lane per scenario walks its own line)
//   PathOptimizer::processInitState              src/path_optimizer.cpp:73-85
// getCurvature (tools.cpp:38-44): (x' y'' - y' x'') / pow(x'^2 + y'^2, 1.5).  v * sqrt(v) is within an ulp of pow(v, 1.5), as
// libm's pow is of ocml's; the walk below evaluates it at every step, where a double-precision pow would dominate.
__device__ __forceinline__ double curvature_of(double dx, double dy, double ddx, double ddy) {
#pragma clang fp contract(off)
    const double v = dx * dx + dy * dy;
    return (dx * ddy - dy * ddx) / (v * sqrt(v));
}

// One wavefront per scenario: the spline table is staged in LDS, lane 0 walks s (it only needs the curvature at each step),
// then all lanes evaluate the states of the walk's abscissae in parallel and write them coalesced.
__global__ void __launch_bounds__(64) reference_states_kernel(const RefStatesArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];          // [9][m] spline table, [n_max] abscissae
    __shared__ int cnt_sh;
    const int qp = blockIdx.x;
    const int n = a.m;
    {
        const double* src = a.spl + (size_t)qp * 9 * n;
        for (int k = threadIdx.x; k < 9 * n; k += blockDim.x) lds[k] = src[k];
    }
    __syncthreads();
    const double* tab = lds;
    double* s_of = lds + 9 * n;
    const double* ext = a.spl_ext + (size_t)qp * 4;
    const SplineView sx{tab, tab + n, tab + 2 * n, tab + 3 * n, tab + 4 * n, ext[0], ext[1], n};
    const SplineView sy{tab, tab + 5 * n, tab + 6 * n, tab + 7 * n, tab + 8 * n, ext[2], ext[3], n};
    const double max_s = a.max_s[qp];
    if (threadIdx.x == 0) {
        const double large_k = 0.2, small_k = 0.08;
        int cnt = 0;
        double tmp_s = 0.0;
        int seg = 0;                 // s only grows: the segment of std::lower_bound advances with it
        if (a.dynamic == 2) {            // s_list = {0}; while (back < max_s) push(back + delta_s); if (max_s - back > 1) push(max_s)
            s_of[0] = 0.0;
            cnt = 1;
            while (tmp_s < max_s && cnt < (1 << 20)) {
                tmp_s += a.ds_large;
                if (cnt < a.n_max) s_of[cnt] = tmp_s;
                cnt += 1;
            }
            if (max_s - tmp_s > 1.0) {   // (:68-70 as written; cannot happen after the loop above)
                if (cnt < a.n_max) s_of[cnt] = max_s;
                cnt += 1;
            }
        }
        while (a.dynamic != 2 && tmp_s <= max_s && cnt < (1 << 20)) {
            if (cnt < a.n_max) s_of[cnt] = tmp_s;
            cnt += 1;
            if (a.dynamic) {
                double x, dx, ddx, y, dy, ddy;
                if (tmp_s > sx.x[n - 1]) {       // right extrapolation: the general evaluator
                    spline_eval3(sx, tmp_s, x, dx, ddx);
                    spline_eval3(sy, tmp_s, y, dy, ddy);
                } else {
                    while (seg + 1 < n && sx.x[seg + 1] < tmp_s) ++seg;      // idx = max(lower_bound(s) - 1, 0)
                    const double h = tmp_s - sx.x[seg];
                    dx = (3.0 * sx.a[seg] * h + 2.0 * sx.b[seg]) * h + sx.c[seg];
                    ddx = 6.0 * sx.a[seg] * h + 2.0 * sx.b[seg];
                    dy = (3.0 * sy.a[seg] * h + 2.0 * sy.b[seg]) * h + sy.c[seg];
                    ddy = 6.0 * sy.a[seg] * h + 2.0 * sy.b[seg];
                }
                const double ak = fabs(curvature_of(dx, dy, ddx, ddy));
                const double k_share = ak > large_k ? 1.0 : (ak < small_k ? 0.0 : (ak - small_k) / (large_k - small_k));
                tmp_s += a.ds_large - k_share * (a.ds_large - a.ds_small);
            } else {
                tmp_s += a.ds_large;
            }
        }
        cnt_sh = cnt;
        a.count[qp] = cnt;
        if (a.init_err && a.start) {
            double ix, dx, ddx, iy, dy, ddy;
            spline_eval3(sx, 0.0, ix, dx, ddx);
            spline_eval3(sy, 0.0, iy, dy, ddy);
            const double ih = atan2(dy, dx);
            const double sx0 = a.start[3 * qp], sy0 = a.start[3 * qp + 1], sh0 = a.start[3 * qp + 2];
            const double ex = ix - sx0, ey = iy - sy0;
            const double local_y = -ex * sin(sh0) + ey * cos(sh0);
            const double dist = sqrt((sx0 - ix) * (sx0 - ix) + (sy0 - iy) * (sy0 - iy));
            a.init_err[2 * qp] = local_y < 0.0 ? dist : -dist;
            a.init_err[2 * qp + 1] = constrain_angle(sh0 - ih);
        }
    }
    __syncthreads();
    const int cnt = cnt_sh < a.n_max ? cnt_sh : a.n_max;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        const double s = s_of[i];
        double x, dx, ddx, y, dy, ddy;
        spline_eval3(sx, s, x, dx, ddx);
        spline_eval3(sy, s, y, dy, ddy);
        if (a.dynamic == 2) {
            const size_t o = (size_t)qp * a.n_max + i;
            a.lx[o] = x; a.ly[o] = y; a.ls[o] = s; a.langle[o] = atan2(dy, dx);
            a.lk[o] = (dx * ddy - dy * ddx) / pow(dx * dx + dy * dy, 1.5);                // :79
            continue;
        }
        double* r = a.ref + ((size_t)qp * a.n_max + i) * PQP_REF_STRIDE;
        r[0] = s; r[1] = curvature_of(dx, dy, ddx, ddy); r[2] = atan2(dy, dx); r[3] = x; r[4] = y;
    }
}

// ReferencePathSmoother::bSpline (src/reference_path_smoother/reference_path_smoother.cpp:490-521): the input points are the control
// points of a clamped B-spline (tinyspline::BSpline(n, 2, degree), degree 3 / 4 / 5 by the points' average spacing), sampled at
// t = 0, 1/length, 2/length, ... while t < 1 and at t = 1; s = accumulated chord length.  tinyspline is not part of the reference
// tree: its clamped knot vector and de Boor evaluation are restated from its published behaviour (oracle/corridor_oracle.py says
// what that is and that this parity is unpinned).  One wavefront per scenario: lane 0 walks t (the accumulation is sequential as
// written), all lanes evaluate the samples in parallel, lane 0 accumulates the chord lengths in the reference's order.
struct BsplineArgs {
    int batch, p_max, n_max;
    const double* pts;               // [batch][p_max][2] input points x, y
    const int32_t* n_pts;            // [batch] points of each scenario (4 .. p_max; fewer: count = 0, the reference's "Few reference points")
    double *x, *y, *s;               // [batch][n_max]
    int32_t* count;                  // [batch] samples the loop produces (when it exceeds n_max only n_max were written)
};

template <int DEG>
__device__ __forceinline__ void de_boor(const double* ctrl, const double* knots, int n, double u, double& ox, double& oy) {
#pragma clang fp contract(off)
    int k = DEG;
    while (k + 1 < n && knots[k + 1] <= u) ++k;                // knots[k] <= u < knots[k + 1]
    double dx[DEG + 1], dy[DEG + 1];
#pragma unroll
    for (int j = 0; j <= DEG; ++j) { dx[j] = ctrl[2 * (j + k - DEG)]; dy[j] = ctrl[2 * (j + k - DEG) + 1]; }
#pragma unroll
    for (int r = 1; r <= DEG; ++r) {
#pragma unroll
        for (int j = DEG; j >= r; --j) {
            const int i = j + k - DEG;
            const double a = (u - knots[i]) / (knots[i + DEG - r + 1] - knots[i]);
            dx[j] = (1.0 - a) * dx[j - 1] + a * dx[j];
            dy[j] = (1.0 - a) * dy[j - 1] + a * dy[j];
        }
    }
    ox = dx[DEG]; oy = dy[DEG];
}

__global__ void __launch_bounds__(64) bspline_resample_kernel(const BsplineArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];          // [p_max][2] points, [p_max + 6] knots, [n_max] t, x, y
    __shared__ int cnt_sh, deg_sh;
    const int qp = blockIdx.x;
    const int n = a.n_pts[qp];
    double* ctrl = lds;
    double* knots = lds + 2 * a.p_max;
    double* t_of = knots + a.p_max + 6;
    double* px = t_of + a.n_max;
    double* py = px + a.n_max;
    if (n < 4 || n > a.p_max) {             // reference_path_smoother.cpp:33-36
        if (threadIdx.x == 0) a.count[qp] = 0;
        return;
    }
    for (int k = threadIdx.x; k < 2 * n; k += blockDim.x) ctrl[k] = a.pts[(size_t)qp * a.p_max * 2 + k];
    __syncthreads();
    if (threadIdx.x == 0) {
        double length = 0.0;
        for (int i = 0; i + 1 < n; ++i) {
            const double ex = ctrl[2 * i] - ctrl[2 * i + 2], ey = ctrl[2 * i + 1] - ctrl[2 * i + 3];
            length += sqrt(ex * ex + ey * ey);
        }
        const double average_length = length / (double)(n - 1);
        const int degree = average_length > 10.0 ? 3 : (average_length > 5.0 ? 4 : 5);
        int cnt = 0;
        // tinyspline refuses a degree that is not below the number of control points (the reference's bSpline throws there): no line, as
        // for fewer than 4 points - de Boor would read control points that are not there
        if (n > degree) {
            const int order = degree + 1, n_knots = n + order;
            const double fac = 1.0 / (double)(n_knots - 2 * degree - 1);
            for (int i = 0; i < n_knots; ++i) knots[i] = i < order ? 0.0 : (i < n_knots - order ? (double)(i - degree) * fac : 1.0);
            const double delta_t = 1.0 / length;
            double tmp_t = 0.0;
            while (tmp_t < 1.0 && cnt < (1 << 20)) {
                if (cnt < a.n_max) t_of[cnt] = tmp_t;
                cnt += 1;
                tmp_t += delta_t;
            }
            if (cnt < a.n_max) t_of[cnt] = 1.0;
            cnt += 1;
        }
        cnt_sh = cnt; deg_sh = degree;
        a.count[qp] = cnt;
    }
    __syncthreads();
    const int cnt = cnt_sh < a.n_max ? cnt_sh : a.n_max;
    const int degree = deg_sh;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        const double u = t_of[i];
        double ox, oy;
        if (u <= 0.0) { ox = ctrl[0]; oy = ctrl[1]; }
        else if (u >= 1.0) { ox = ctrl[2 * (n - 1)]; oy = ctrl[2 * (n - 1) + 1]; }
        else if (degree == 3) de_boor<3>(ctrl, knots, n, u, ox, oy);
        else if (degree == 4) de_boor<4>(ctrl, knots, n, u, ox, oy);
        else de_boor<5>(ctrl, knots, n, u, ox, oy);
        px[i] = ox; py[i] = oy;
        a.x[(size_t)qp * a.n_max + i] = ox;
        a.y[(size_t)qp * a.n_max + i] = oy;
    }
    __syncthreads();
    if (threadIdx.x == 0 && cnt > 0) {
        double acc = 0.0;
        a.s[(size_t)qp * a.n_max] = 0.0;
        for (int i = 1; i < cnt; ++i) {
            const double ex = px[i] - px[i - 1], ey = py[i] - py[i - 1];
            acc += sqrt(ex * ex + ey * ey);
            a.s[(size_t)qp * a.n_max + i] = acc;
        }
    }
}

// getProjection (src/tools/tools.cpp:66-96) with getProjectionByNewton (:98-126): the abscissa of the point of the line nearest to
// (tx, ty) - a 1 m grid search from 0, the end point, then Newton on the squared distance (20 steps, |ds| < 1e-5), clipped to the length.
__device__ __forceinline__ double spline_projection(const SplineView& sx, const SplineView& sy, double tx, double ty, double length) {
#pragma clang fp contract(off)
    if (!(length > 0.0)) return 0.0;                  // max_s <= start_s: the state at start_s, whose s stays 0 (:71-74)
    double tmp = 0.0, best_s = 0.0, best = 1.7976931348623157e308;
    while (tmp <= length) {
        double x, y, d1, d2;
        spline_eval3(sx, tmp, x, d1, d2); spline_eval3(sy, tmp, y, d1, d2);
        const double d = sqrt((x - tx) * (x - tx) + (y - ty) * (y - ty));
        if (d < best) { best = d; best_s = tmp; }
        tmp += 1.0;
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

// The same projection computed by a whole wavefront (every lane of it calls this, every lane gets the result): the coarse scan at 1 m
// steps - up to 40 spline evaluations in a row for one lane - is one evaluation per lane; the first minimum wins as in the serial scan
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

// PathOptimizer::setReferencePathLength (src/path_optimizer.cpp:87-104): when the target state lies behind the end of the reference
// line (its x in the end state's frame is <= 0), the line is cut at the target's projection.  One wavefront per scenario (the spline
// table goes through LDS as in the other kernels; the projection's coarse scan runs one sample per lane).
struct RefLengthArgs {
    int batch, m;
    const double* spl;               // [batch][9][m]
    const double* spl_ext;           // [batch][4]
    const double* length;            // [batch] ReferencePath::getLength()
    const double* target;            // [batch][3] target state x, y, heading
    double* length_out;              // [batch]
};

__global__ void __launch_bounds__(64) reference_length_kernel(const RefLengthArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];          // [9][m]
    const int qp = blockIdx.x;
    const int n = a.m;
    {
        const double* src = a.spl + (size_t)qp * 9 * n;
        for (int k = threadIdx.x; k < 9 * n; k += blockDim.x) lds[k] = src[k];
    }
    __syncthreads();
    const double* tab = lds;
    const double* ext = a.spl_ext + (size_t)qp * 4;
    const SplineView sx{tab, tab + n, tab + 2 * n, tab + 3 * n, tab + 4 * n, ext[0], ext[1], n};
    const SplineView sy{tab, tab + 5 * n, tab + 6 * n, tab + 7 * n, tab + 8 * n, ext[2], ext[3], n};
    const double L = a.length[qp];
    const double tx = a.target[3 * qp], ty = a.target[3 * qp + 1];
    double ex, dx, ddx, ey, dy, ddy;
    spline_eval3(sx, L, ex, dx, ddx); spline_eval3(sy, L, ey, dy, ddy);
    const double eh = atan2(dy, dx);
    const double local_x = (tx - ex) * cos(eh) + (ty - ey) * sin(eh);          // global2Local(end_ref_state, target).x   tools.cpp:57-64
    const double out = local_x > 0.0 ? L : spline_projection_wave(sx, sy, tx, ty, L);     // (local_x is the same in every lane)
    if (threadIdx.x == 0) a.length_out[qp] = out;
}

// The tail of ReferencePathSmoother::postSmooth (src/reference_path_smoother/reference_path_smoother.cpp:559-573): the QP's lateral
// offsets at the layers' abscissae become points x = x_s(s) + l cos(heading + pi/2), y = y_s(s) + l sin(heading + pi/2) with the
// accumulated chord length as their new abscissa - the knots of the final reference line's splines (:574-576, pqp_spline_fit).
// One wavefront per scenario: the lanes evaluate the points, lane 0 accumulates the chord lengths in the reference's order.
struct OffsetsArgs {
    int batch, m_spl, m;
    const double* spl;               // [batch][9][m_spl]
    const double* spl_ext;           // [batch][4]
    const double* at_s;              // [batch][m] abscissae on the line (layers_s_list_)
    const double* l;                 // [batch][m] lateral offsets (QPSolution(i))
    const int32_t* m_of;             // [batch] points of each scenario, or nullptr (all m)
    double *x, *y, *s;               // [batch][m]
};

__global__ void __launch_bounds__(64) offsets_to_points_kernel(const OffsetsArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];          // [9][m_spl] spline table, [m] x, [m] y
    const int qp = blockIdx.x;
    const int n = a.m_spl;
    {
        const double* src = a.spl + (size_t)qp * 9 * n;
        for (int k = threadIdx.x; k < 9 * n; k += blockDim.x) lds[k] = src[k];
    }
    __syncthreads();
    const double* tab = lds;
    double* px = lds + 9 * n;
    double* py = px + a.m;
    const double* ext = a.spl_ext + (size_t)qp * 4;
    const SplineView sx{tab, tab + n, tab + 2 * n, tab + 3 * n, tab + 4 * n, ext[0], ext[1], n};
    const SplineView sy{tab, tab + 5 * n, tab + 6 * n, tab + 7 * n, tab + 8 * n, ext[2], ext[3], n};
    int cnt = a.m_of ? a.m_of[qp] : a.m;
    cnt = cnt < a.m ? (cnt > 0 ? cnt : 0) : a.m;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        const size_t o = (size_t)qp * a.m + i;
        const double rs = a.at_s[o];
        double fx, dx, ddx, fy, dy, ddy;
        spline_eval3(sx, rs, fx, dx, ddx);
        spline_eval3(sy, rs, fy, dy, ddy);
        const double dir = atan2(dy, dx);
        const double x = fx + a.l[o] * cos(dir + kPi2), y = fy + a.l[o] * sin(dir + kPi2);
        px[i] = x; py[i] = y;
        a.x[o] = x; a.y[o] = y;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int i = 0; i < cnt; ++i) {
            if (i > 0) {
                const double ex = px[i] - px[i - 1], ey = py[i] - py[i - 1];
                acc += sqrt(ex * ex + ey * ey);
            }
            a.s[(size_t)qp * a.m + i] = acc;
        }
    }
}

// Natural cubic spline through (s_i, v_i) - what tk::spline::set_points computes (src/tools/spline.cpp:161-249: behaviour, not text), the
// refit that glues the smoother QPs, the reference states and the path QP together (SURVEY.md 8f rank 3; called at
// tension_smoother.cpp:36-38, reference_path_smoother.cpp:58-59,574-576, reference_path_impl.cpp:349-350).
// Formulation (round 6, written from the textbook moment equations, independent of the reference's band-matrix LU): with h_i = s_{i+1} - s_i,
// d_i = (v_{i+1} - v_i) / h_i and the moments M_i = f''(s_i), M_0 = M_{n-1} = 0 (the reference never calls set_boundary),
//     h_{i-1} M_{i-1} + 2 (h_{i-1} + h_i) M_i + h_i M_{i+1} = 6 (d_i - d_{i-1}),   i = 1 .. n-2,
// solved by the Thomas recurrence (forward: pivot reciprocal, modified super-diagonal and right-hand side; backward: substitution), FMA
// contraction allowed; the table's coefficients of f = a (s - s_i)^3 + b (s - s_i)^2 + c (s - s_i) + v_i follow from the moments:
// b_i = M_i / 2, a_i = (M_{i+1} - M_i) / (6 h_i), c_i = d_i - h_i (2 M_i + M_{i+1}) / 6.  Agreement with the reference's compiled
// tk::spline (oracle/_ref/libref_spline.so): a few ulp of the largest coefficient of a row (tests/test_gpu_corridor.py).
// The recurrence is a chain in the knot index, so one wavefront fits one coordinate of one scenario: the lanes stage knots and values in
// LDS, compute h, d and the right-hand sides in parallel and write the coefficient rows back coalesced; lane 0 runs the two sweeps.
struct SplineFitArgs {
    int batch, m;
    const int32_t* m_of;             // [batch] knots of each scenario (3 .. m; m is then the array stride) or nullptr: all have m
    const double* s;                 // [batch][m] knots
    const double* vx;                // [batch][m] x values
    const double* vy;                // [batch][m] y values
    double* spl;                     // [batch][9][m]
    double* spl_ext;                 // [batch][4]
};

__global__ void __launch_bounds__(64) spline_fit_kernel(const SplineFitArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];          // knots, values, h, d, right-hand sides / moments, sweep work / cubic coefficients, linear coefficients: [7][m]
    const int idx = blockIdx.x;
    const int qp = idx >> 1, coord = idx & 1;
    const int stride = a.m;
    // A scenario with fewer knots than the stride: the fit runs on its own n knots; the table is then padded with knots far beyond the
    // line (x_last + 1e6 j, zero coefficients).  Every evaluation beyond the last real knot lands in segment n - 1, whose cubic
    // coefficient is 0 - term by term the reference's right-hand extrapolation (spline.cpp:262-266,295-306) - so the consumers of the
    // table need no count of their own.  (Fewer than 3 knots: tk::spline asserts; the table is filled with the first point.)
    const int n_raw = a.m_of ? a.m_of[qp] : stride;
    const int n = n_raw < 3 ? stride : (n_raw < stride ? n_raw : stride);
    const bool degenerate = n_raw < 3;
    double* x = lds;
    double* y = x + n;
    double* h = y + n;               // h_i = x_{i+1} - x_i
    double* d = h + n;               // d_i = (y_{i+1} - y_i) / h_i
    double* mo = d + n;              // right-hand sides, then the moments M_i
    double* cp = mo + n;             // modified super-diagonal of the forward sweep; afterwards the cubic coefficients a_i
    double* cl = cp + n;             // the linear coefficients c_i
    {
        const double* gx = a.s + (size_t)qp * stride;
        const double* gy = (coord ? a.vy : a.vx) + (size_t)qp * stride;
        for (int i = threadIdx.x; i < n; i += blockDim.x) { x[i] = degenerate ? (double)i : gx[i]; y[i] = degenerate ? gy[0] : gy[i]; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n - 1; i += blockDim.x) {
        const double hi = x[i + 1] - x[i];
        h[i] = hi;
        d[i] = (y[i + 1] - y[i]) / hi;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) mo[i] = (i >= 1 && i < n - 1) ? 6.0 * (d[i] - d[i - 1]) : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
        // forward sweep over the interior rows (M_0 = 0 drops the first row's sub-diagonal term), backward substitution (M_{n-1} = 0)
        double cprev = 0.0, dprev = 0.0;
        for (int i = 1; i < n - 1; ++i) {
            const double sub = h[i - 1];
            const double piv = 1.0 / (2.0 * (sub + h[i]) - sub * cprev);
            cprev = h[i] * piv;
            dprev = (mo[i] - sub * dprev) * piv;
            cp[i] = cprev; mo[i] = dprev;
        }
        double mnext = 0.0;
        for (int i = n - 2; i >= 1; --i) {
            mnext = mo[i] - cp[i] * mnext;
            mo[i] = mnext;
        }
    }
    __syncthreads();
    // coefficients from the moments (cp is free now: it takes the cubic coefficients)
    for (int i = threadIdx.x; i < n - 1; i += blockDim.x) {
        cp[i] = (mo[i + 1] - mo[i]) / (6.0 * h[i]);
        cl[i] = d[i] - h[i] * (2.0 * mo[i] + mo[i + 1]) * (1.0 / 6.0);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.spl_ext[4 * qp + 2 * coord] = 0.5 * mo[0];                               // b, c of the left extrapolation (b_0 = M_0 / 2 = 0)
        a.spl_ext[4 * qp + 2 * coord + 1] = cl[0];
        const double hl = h[n - 2];                                                // the last knot continues the last segment's slope: f'(s_{n-1})
        cp[n - 1] = 0.0;
        cl[n - 1] = 3.0 * cp[n - 2] * hl * hl + mo[n - 2] * hl + cl[n - 2];        // (2 b_{n-2} = M_{n-2})
    }
    __syncthreads();
    double* tab = a.spl + (size_t)qp * 9 * stride;
    double* rows = tab + (size_t)(1 + 4 * coord) * stride;     // y, a, b, c of this coordinate
    for (int i = threadIdx.x; i < stride; i += blockDim.x) {
        const bool pad = i >= n;
        if (coord == 0) tab[i] = pad ? x[n - 1] + 1e6 * (double)(i - n + 1) : x[i];
        rows[i] = pad ? y[n - 1] : y[i];
        rows[stride + i] = pad ? 0.0 : cp[i]; rows[2 * stride + i] = pad ? 0.0 : 0.5 * mo[i]; rows[3 * stride + i] = pad ? 0.0 : cl[i];
    }
}

// dst[b] = src[b][count[b] - 1] + add: the length of a line from its abscissa list (the hand-over between the chain's steps)
__global__ void gather_last_kernel(int batch, int stride, const int32_t* __restrict__ count, const double* __restrict__ src, double add,
                                   double* __restrict__ dst) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    int c = count[b];
    c = c < 1 ? 1 : (c > stride ? stride : c);
    dst[b] = src[(size_t)b * stride + c - 1] + add;
}

// Layered DP corridor search between the smoother QP and the postSmooth QP (SURVEY.md 8f rank 4):
//   ReferencePathSmoother::graphSearchDp    src/reference_path_smoother/reference_path_smoother.cpp:142-295
//   ReferencePathSmoother::calculateCostAt  :107-140        getProjection / getProjectionByNewton  src/tools/tools.cpp:66-126
// One workgroup of four wavefronts per scenario.  Layers are sequential (the cost of a node needs the costs of the previous layer).
// Within a layer the lanes of the first wavefront are the lateral samples (34 with the default +-10 m / 0.6 m): each samples the
// distance map and decides feasibility; then ALL 256 lanes evaluate the (node, predecessor) edges - 34 x 34 atan2-heavy costs, the
// kernel's whole arithmetic, 4-5 per lane instead of 34 in a row - into LDS, and the node lanes pick their cheapest predecessor
// (first one on ties, as the reference's strict `<` scan does).  Parents are kept per (layer, lane); lane 0 walks them back, then
// the lanes refine the bounds of the chosen node of every layer in parallel (0.2 m steps along the normal, as the reference does).
struct DpArgs {
    int batch, m, max_layers;
    const double* spl;               // [batch][9][m]
    const double* spl_ext;           // [batch][4]
    const double* length;            // [batch] reference->getLength()
    const double* start;             // [batch][3] start_state_ x, y, heading
    const float* dist;
    const int32_t* map_of;
    pqp_grid_geometry g;
    pqp_dp_params p;
    double* layers_s;                // [batch][max_layers]
    double* lb;                      // [batch][max_layers]
    double* ub;                      // [batch][max_layers]
    int32_t* count;                  // [batch] layers of the corridor; 0: graphSearchDp returns false / nothing reachable; -1: more than max_layers
    double* vehicle_l;               // [batch] vehicle_l_wrt_smoothed_ref_
};

constexpr int kDpChunk = 32;        // layers whose nodes are prepared at once (bounds the LDS table whatever max_layers is)
struct DpLds {
    int m, lmax, nlat;
    __host__ __device__ int spl() const { return 0; }                          // [9][m]
    __host__ __device__ int s_layer() const { return 9 * m; }                  // [lmax]
    __host__ __device__ int node() const { return s_layer() + lmax; }          // [2][64][2]  dir, cost of the previous / current layer's nodes
    __host__ __device__ int misc() const { return node() + 2 * 64 * 2; }       // [8]
    __host__ __device__ int mask() const { return misc() + 8; }                // unsigned long long [lmax]  feasibility of a layer's nodes
    __host__ __device__ int ltab() const { return mask() + lmax; }             // [64] lateral offset of sample j
    __host__ __device__ int lay() const { return ltab() + 64; }                // [lmax][8]  rx, ry, rh, cos, sin of the normal, rk, 1/rk of a layer
    __host__ __device__ int self() const { return lay() + 8 * lmax; }          // [kDpChunk + 1][nlat] own cost of a node (< 0: infeasible), ring of layers
    __host__ __device__ int edge() const { return self() + (kDpChunk + 1) * nlat; }   // [nlat][nlat] cost of reaching node j through predecessor jp
    __host__ __device__ int edir() const { return edge() + nlat * nlat; }      // [nlat][nlat] direction of that edge (the node phase takes its parent's from here instead of a second atan2)
    __host__ __device__ int parent() const { return edir() + nlat * nlat; }    // unsigned char [lmax][nlat] (255: none), then int path[lmax]
    __host__ __device__ size_t parent_bytes() const { return (((size_t)lmax * nlat + 7) / 8) * 8; }
    __host__ __device__ size_t total_bytes() const { return (size_t)parent() * 8 + parent_bytes() + (size_t)lmax * 4; }
};
constexpr int kDpThreads = 256;
// lateral samples per layer: -range, -range + spacing, ... while <= range, as the reference accumulates them (at most 64)
__host__ __device__ inline int dp_lateral_samples(double range, double spacing) {
    int nlat = 0;
    double c = -range;
    while (c <= range && nlat < 64) { c += spacing; nlat += 1; }
    return nlat;
}

__device__ __forceinline__ double dp_dist(const float* __restrict__ dist, const pqp_grid_geometry& g, double x, double y) {
#pragma clang fp contract(off)
    const double tx = -(x - g.pos_x - 0.5 * g.length_x), ty = -(y - g.pos_y - 0.5 * g.length_y);
    const bool inside = tx >= 0.0 && ty >= 0.0 && tx < g.length_x && ty < g.length_y;
    return inside ? obstacle_distance(dist, g, x, y) : -1.0;                   // isInside ? getObstacleDistance : -1   (:191)
}

__global__ void __launch_bounds__(kDpThreads) dp_corridor_kernel(const DpArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int qp = blockIdx.x, lane = threadIdx.x;          // lane < 64: the lateral sample `lane` in the per-node phases
    const double range = a.p.lateral_range, spacing = a.p.lateral_spacing;
    const int nlat = dp_lateral_samples(range, spacing);
    const DpLds L{a.m, a.max_layers, nlat};
    const int n = a.m;
    {
        const double* src = a.spl + (size_t)qp * 9 * n;
        for (int k = lane; k < 9 * n; k += kDpThreads) lds[k] = src[k];
    }
    __syncthreads();
    const double* tab = lds;
    const double* ext = a.spl_ext + (size_t)qp * 4;
    const SplineView sx{tab, tab + n, tab + 2 * n, tab + 3 * n, tab + 4 * n, ext[0], ext[1], n};
    const SplineView sy{tab, tab + 5 * n, tab + 6 * n, tab + 7 * n, tab + 8 * n, ext[2], ext[3], n};
    const float* dist = a.dist + (size_t)(a.map_of ? a.map_of[qp] : 0) * a.g.rows * a.g.cols;
    double* s_layer = lds + L.s_layer();
    double* misc = lds + L.misc();
    double* ltab = lds + L.ltab();
    double* lay = lds + L.lay();
    double* self = lds + L.self();
    double* edge_cost = lds + L.edge();
    double* edge_dir = lds + L.edir();
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(lds + L.mask());
    unsigned char* parent = reinterpret_cast<unsigned char*>(lds + L.parent());
    int* path = reinterpret_cast<int*>(parent + L.parent_bytes());
    const double length = a.length[qp];
    const double stx = a.start[3 * qp], sty = a.start[3 * qp + 1], sth = a.start[3 * qp + 2];
    const double thr = a.p.car_width / 2.0 + 0.2;
    constexpr double kNone = 1.7976931348623157e308;

    double s0_proj = 0.0;
    if (lane < 64) s0_proj = spline_projection_wave(sx, sy, stx, sty, length);    // getProjection(x_s, y_s, start, length).s, first wavefront
    if (lane == 0) {
        const double s0 = s0_proj;
        const double search_ds = length > 6.0 ? a.p.longitudinal_spacing : 0.5;
        int nl = 0;
        double tmp = s0;
        while (tmp < length) { if (nl < a.max_layers) s_layer[nl] = tmp; nl += 1; tmp += search_ds; }
        if (nl < a.max_layers) s_layer[nl] = length;
        nl += 1;
        double px, dx, ddx, py, dy, ddy;
        const double vs = s_layer[0];
        spline_eval3(sx, vs, px, dx, ddx); spline_eval3(sy, vs, py, dy, ddy);
        const double ph = atan2(dy, dx);
        const double ex = stx - px, ey = sty - py;
        const double vl = -ex * sin(ph) + ey * cos(ph);            // global2Local(proj_point, start_state_).y
        misc[0] = (double)nl; misc[1] = vl;
        misc[2] = (double)(int)((range + vl) / spacing);          // start_lateral_index
    }
    if (lane >= 64 && lane < 128) {
        // lateral offset of sample j: -range + j additions of the spacing, as the reference accumulates it
        double l = -range;
        for (int q = 0; q < lane - 64; ++q) l += spacing;
        ltab[lane - 64] = l;
    }
    __syncthreads();
    const int nl = (int)misc[0];
    const double vehicle_l = misc[1];
    const int start_idx = (int)misc[2];
    if (lane == 0) a.vehicle_l[qp] = vehicle_l;
    if (nl > a.max_layers) { if (lane == 0) a.count[qp] = -1; return; }
    if (fabs(vehicle_l) > range) { if (lane == 0) a.count[qp] = 0; return; }       // "Vehicle far from ref, quit graph search."

    // -- everything of a layer that does not depend on the layers before it, all layers at once: the reference point, heading and
    //    curvature of the layer (one lane per layer) ...
    for (int i = lane; i < nl; i += kDpThreads) {
        double rx, dx, ddx, ry, dy, ddy;
        spline_eval3(sx, s_layer[i], rx, dx, ddx); spline_eval3(sy, s_layer[i], ry, dy, ddy);
        const double rh = atan2(dy, dx);
        const double rk = curvature_of(dx, dy, ddx, ddy);
        double* w = lay + 8 * i;
        w[0] = rx; w[1] = ry; w[2] = rh; w[3] = cos(rh + kPi2); w[4] = sin(rh + kPi2); w[5] = rk; w[6] = 1.0 / rk;
    }
    __syncthreads();
    const bool node_lane = lane < nlat;
    if (lane < 64) {         // layer 0: only the start node, cost 0, heading of the start state
        double* cn = lds + L.node() + 2 * lane;
        const bool st = node_lane && lane == start_idx;
        cn[0] = st ? sth : 0.0; cn[1] = st ? 0.0 : kNone;
        if (node_lane) parent[lane] = (unsigned char)255;
    }

    int max_layer = 0;
    bool stopped = false;
    for (int c0 = 0; c0 < nl && !stopped; c0 += kDpChunk) {
        const int c1 = c0 + kDpChunk < nl ? c0 + kDpChunk : nl;
        //    ... and position, distance to the obstacles, feasibility and own cost of every node of the next kDpChunk layers (one lane per
        //    node, the map gathers of all of them in flight together)
        for (int p = lane + c0 * nlat; p < c1 * nlat; p += kDpThreads) {
            const int i = p / nlat, j = p - i * nlat;
            const double* w = lay + 8 * i;
            const double lj = ltab[j], rk = w[5], rr = w[6];
            const double x = w[0] + lj * w[3], y = w[1] + lj * w[4];
            const double d = dp_dist(dist, a.g, x, y);
            bool feas = !((rk < 0.0 && lj < rr) || (rk > 0.0 && lj > rr) || d < thr);
            if (i == 0) feas = j == start_idx;
            double self_cost = 0.0;
            if (d < 3.0) self_cost += (3.0 - d) / 3.0 * 0.5;
            self_cost += fabs(lj) / range * 1.0;
            self[(i % (kDpChunk + 1)) * nlat + j] = feas ? self_cost : -1.0;
        }
        __syncthreads();
        for (int i = lane + c0; i < c1; i += kDpThreads) {
            unsigned long long m = 0ull;
            for (int j = 0; j < nlat; ++j) m |= (self[(i % (kDpChunk + 1)) * nlat + j] >= 0.0 ? 1ull : 0ull) << j;
            mask[i] = m;
        }
        for (int i = c0 > 1 ? c0 : 1; i < c1; ++i) {
            const double* w = lay + 8 * i;
            const double* wp = lay + 8 * (i - 1);
            const double rh = w[2];
            const double* pn = lds + L.node() + ((i - 1) & 1) * 64 * 2;       // dir, cost of the previous layer's nodes
            const double* sc = self + (i % (kDpChunk + 1)) * nlat;
            const double* sp = self + ((i - 1) % (kDpChunk + 1)) * nlat;
            const double ds = s_layer[i] - s_layer[i - 1];
            // -- calculateCostAt for every (node j, predecessor jp) edge, all lanes.  Only predecessors within ds laterally are admissible
            //    (:124): they are enumerated inside the window |jp - j| <= ds / spacing + 1 (a superset; the exact test stays), which
            //    makes a layer 34 x 7 = 238 edges - one per lane - instead of 34 x 34 of which 85 % fail the test
            const int R = (int)(ds / spacing) + 1;
            const bool full = 2 * R + 1 >= nlat;
            const int W = full ? nlat : 2 * R + 1;
            for (int p = lane; p < nlat * W; p += kDpThreads) {
                const int j = p / W, jp = (full ? 0 : j - R) + (p - j * W);
                double total = kNone;
                if (jp >= 0 && jp < nlat) {
                    const double lj = ltab[j], lp = ltab[jp];
                    if (sc[j] >= 0.0 && sp[jp] >= 0.0 && !(fabs(lp - lj) > ds)) {
                        const double x = w[0] + lj * w[3], y = w[1] + lj * w[4];
                        const double qx = wp[0] + lp * wp[3], qy = wp[1] + lp * wp[4];
                        const double direction = atan2(y - qy, x - qx);
                        const double edge = exact_div(fabs(constrain_angle(direction - pn[2 * jp])), kPi2, 1.0 / kPi2) * 16.0 + exact_div(fabs(constrain_angle(direction - rh)), kPi2, 1.0 / kPi2) * 0.5;
                        total = sc[j] + edge + pn[2 * jp + 1];
                        edge_dir[p] = direction;
                    }
                }
                edge_cost[p] = total;
            }
            __syncthreads();
            // -- the cheapest predecessor of every node (the first one on ties: the window is scanned in ascending jp)
            if (lane < 64) {
                double cost = kNone, dir = 0.0;
                int par = -1;
                if (node_lane && sc[lane] >= 0.0) {
                    double min_cost = kNone;
                    int kbest = 0;
                    for (int k = 0; k < W; ++k) {
                        const double total = edge_cost[lane * W + k];
                        if (total < min_cost) { min_cost = total; kbest = k; par = (full ? 0 : lane - R) + k; }
                    }
                    if (par >= 0) { cost = min_cost; dir = edge_dir[lane * W + kbest]; }      // (the direction the edge phase computed: the same expression)
                }
                const bool any_parent = __ballot(par >= 0) != 0ull;
                if (lane == 0) misc[4] = any_parent ? 1.0 : 0.0;
                double* cn = lds + L.node() + (i & 1) * 64 * 2 + 2 * lane;
                cn[0] = dir; cn[1] = cost;
                if (node_lane) parent[(size_t)i * nlat + lane] = (unsigned char)(par < 0 ? 255 : par);
            }
            __syncthreads();
            if (misc[4] == 0.0) { stopped = true; break; }               // layer not reachable: the search stops (:238)
            max_layer = i;
        }
    }
    __syncthreads();

    // retrieve: cheapest node of the last layer reached (first one on ties), then walk the parents back
    if (lane < 64) {
        const double* cn = lds + L.node() + (max_layer & 1) * 64 * 2 + 2 * lane;
        double c = node_lane ? cn[1] : kNone;
        int idx = (c < kNone) ? lane : 64;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double oc = __shfl_xor(c, off, 64);
            const int oi = __shfl_xor(idx, off, 64);
            if (oc < c || (oc == c && oi < idx)) { c = oc; idx = oi; }
        }
        if (lane == 0) {
            int cnt = 0;
            if (idx < 64) {
                int j = idx;
                for (int i = max_layer; i >= 0; --i) { path[i] = j; j = parent[(size_t)i * nlat + j]; }
                cnt = max_layer + 1;
            }
            misc[3] = (double)cnt;
        }
    }
    __syncthreads();
    const int cnt = (int)misc[3];
    if (lane == 0) a.count[qp] = cnt;

    // bounds of the chosen node of every layer (:256-289): one wavefront per layer, lanes 0..31 probe the upper side, 32..63 the
    // lower side - candidate k is the k-th 0.2 m step of the reference's loop, all of a chunk of 32 steps sampled at once.
    const int wave = lane >> 6, wl = lane & 63, side = wl >> 5, k0 = wl & 31;
    for (int i = wave; i < cnt; i += kDpThreads / 64) {
        double lo = -10.0, up = 10.0;                               // layer 0: literally (-10, 10)
        if (i > 0) {
            const int j = path[i];
            const unsigned long long m = mask[i];
            int jlo = j, jup = j;
            while (jlo > 0 && ((m >> (jlo - 1)) & 1ull)) --jlo;       // rough bounds: the run of feasible samples around j
            while (jup < nlat - 1 && ((m >> (jup + 1)) & 1ull)) ++jup;
            const double check_s = 0.2, limit = 6.0;
            const double* w = lay + 8 * i;
            const double rx = w[0], ry = w[1], ca = w[3], sa = w[4];
            // this lane's side: v starts at the rough bound +- check_s and moves away from the node in steps of check_s while the
            // sample is free and |v| < limit; a blocked sample steps back once and ends the walk
            const double sgn = side == 0 ? 1.0 : -1.0;
            double v = side == 0 ? check_s + ltab[jup] : -check_s + ltab[jlo];
            double res = 0.0;
            bool done = false;
            for (int q = 0; q < k0; ++q) v += sgn * check_s;         // candidate k0 of the first chunk
            for (;;) {
                // state of candidate k: the walk reaches it iff all earlier candidates were inside the limit and free
                const bool inside = side == 0 ? v < limit : v > -limit;
                const bool free_here = inside && dp_dist(dist, a.g, rx + v * ca, ry + v * sa) > thr;
                // first candidate of this chunk (per side) that ends the walk: outside the limit (result v) or blocked (result v -+ check_s)
                const unsigned long long stop = __ballot(!free_here);
                const unsigned int mine = (unsigned int)(side == 0 ? (stop & 0xffffffffull) : (stop >> 32));
                if (!done && mine != 0u) {
                    const int first = __builtin_ctz(mine);
                    // the value of the first stopping candidate, from its lane
                    const double vf = __shfl(v, (side << 5) + first, 64);
                    const bool in_f = side == 0 ? vf < limit : vf > -limit;
                    res = in_f ? vf - sgn * check_s : vf;
                    done = true;
                }
                const unsigned long long all_done = __ballot(done);
                if (all_done == ~0ull) break;
                for (int q = 0; q < 32; ++q) v += sgn * check_s;     // the same candidate of the next chunk
            }
            const double r_up = __shfl(res, 0, 64), r_lo = __shfl(res, 32, 64);
            up = r_up; lo = r_lo;
        }
        if (wl == 0) {
            a.layers_s[(size_t)qp * a.max_layers + i] = s_layer[i];
            a.lb[(size_t)qp * a.max_layers + i] = lo;
            a.ub[(size_t)qp * a.max_layers + i] = up;
        }
    }
}

}  // namespace pqp
