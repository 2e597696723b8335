// pqp_long_line_kernels.inc — included by pqp_kernels.hip after pqp_corridor_kernels.inc.  The long forms of the line-geometry kernels
// (PQP_OPT_LONG_LINES, pqp.h): the LDS kernels of pqp_corridor_kernels.inc stage a line's spline table (9 doubles per knot) and their
// per-element arrays in one CU's LDS, which caps the line they take (DESIGN.md 8.3).  Each kernel here is its LDS kernel with what does not
// fit moved out of the LDS, nothing else changed - the same expressions in the same order, so the same bits:
//   - the spline table is read where it lies, in HBM: the binary search of spline_segment touches ~log2(m) knots per evaluation, its first
//     levels shared by every lane of a wavefront (L1 / L2 hits), and the walks in s move through the table in order;
//   - abscissae and points a kernel writes to its outputs anyway are read back from there instead of from an LDS copy;
//   - the rest (the spline fit's seven sweep arrays, the DP's per-layer arrays and parents, the B-spline's knot vector) goes to a workspace
//     of the handle (pqp_handle::line_ws), one slice per workgroup.
// (Named so that no existing kernel's name is a substring of theirs: tests/test_kernel_resources.py finds kernels by substring.)
namespace pqp {

// long_dp_kernel: what stays in LDS - the two node rows, the lateral offsets and the per-chunk cost tables, whatever the line's length
struct DpLongLds {
    int nlat;
    __host__ __device__ int node() const { return 0; }                            // [2][64][2]
    __host__ __device__ int misc() const { return node() + 2 * 64 * 2; }          // [8]
    __host__ __device__ int ltab() const { return misc() + 8; }                   // [64]
    __host__ __device__ int self() const { return ltab() + 64; }                  // [kDpChunk + 1][nlat]
    __host__ __device__ int edge() const { return self() + (kDpChunk + 1) * nlat; }   // [nlat][nlat]
    __host__ __device__ int edir() const { return edge() + nlat * nlat; }         // [nlat][nlat]
    __host__ __device__ size_t total_bytes() const { return (size_t)(edir() + nlat * nlat) * 8; }
};
// ... and what moves to the workspace, per scenario (in doubles): the arrays of DpLds that grow with the layers
struct DpLongWs {
    int lmax, nlat;
    __host__ __device__ size_t s_layer() const { return 0; }                                  // [lmax]
    __host__ __device__ size_t mask() const { return (size_t)lmax; }                          // unsigned long long [lmax]
    __host__ __device__ size_t lay() const { return 2 * (size_t)lmax; }                       // [lmax][8]
    __host__ __device__ size_t parent() const { return 10 * (size_t)lmax; }                   // unsigned char [lmax][nlat]
    __host__ __device__ size_t path() const { return parent() + ((size_t)lmax * nlat + 7) / 8; }   // int [lmax]
    __host__ __device__ size_t doubles() const { return path() + ((size_t)lmax + 1) / 2; }
};


// corridor_bounds_kernel / states_bounds_kernel with the table in HBM: the LDS holds the probes of a tile of waypoints alone
__global__ void __launch_bounds__(1024) long_corridor_kernel(const CorridorArgs a) {
#define PQP_CORRIDOR_ON_STATES 0
#define PQP_CORRIDOR_LONG 1
#include "pqp_corridor_body.inc"
#undef PQP_CORRIDOR_LONG
#undef PQP_CORRIDOR_ON_STATES
}

__global__ void __launch_bounds__(1024) long_states_kernel(const CorridorArgs a, const double* __restrict__ states, int stride) {
#define PQP_CORRIDOR_ON_STATES 1
#define PQP_CORRIDOR_LONG 1
#include "pqp_corridor_body.inc"
#undef PQP_CORRIDOR_LONG
#undef PQP_CORRIDOR_ON_STATES
}

// spline_fit_kernel: ws = [2 batch][7][m], the seven arrays of a (scenario, coordinate)
__global__ void __launch_bounds__(64) long_fit_kernel(const SplineFitArgs a, double* __restrict__ ws) {
    // knots, values, h, d, right-hand sides / moments, sweep work / cubic coefficients, linear coefficients: [7][m] of the workspace
    // per (scenario, coordinate); the two sweeps stream through it
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
    double* x = ws + (size_t)idx * 7 * stride;
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

// reference_states_kernel: the abscissae of the walk go to their output column and are read back by the lanes
__global__ void __launch_bounds__(64) long_ref_states_kernel(const RefStatesArgs a) {
#pragma clang fp contract(off)
    __shared__ int cnt_sh;
    const int qp = blockIdx.x;
    const int n = a.m;
    const double* tab = a.spl + (size_t)qp * 9 * n;
    // the walk's abscissae go straight to their output column (s of a reference state / the `s` list), where the lanes read them back
    double* s_of = a.dynamic == 2 ? a.ls + (size_t)qp * a.n_max : a.ref + (size_t)qp * a.n_max * PQP_REF_STRIDE;
    const int s_step = a.dynamic == 2 ? 1 : PQP_REF_STRIDE;
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
                if (cnt < a.n_max) s_of[(size_t)cnt * s_step] = tmp_s;
                cnt += 1;
            }
            if (max_s - tmp_s > 1.0) {   // (:68-70 as written; cannot happen after the loop above)
                if (cnt < a.n_max) s_of[(size_t)cnt * s_step] = max_s;
                cnt += 1;
            }
        }
        while (a.dynamic != 2 && tmp_s <= max_s && cnt < (1 << 20)) {
            if (cnt < a.n_max) s_of[(size_t)cnt * s_step] = tmp_s;
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
        const double s = s_of[(size_t)i * s_step];
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

// reference_length_kernel
__global__ void __launch_bounds__(64) long_ref_length_kernel(const RefLengthArgs a) {
#pragma clang fp contract(off)
    const int qp = blockIdx.x;
    const int n = a.m;
    const double* tab = a.spl + (size_t)qp * 9 * n;
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

// offsets_to_points_kernel: the points are read back from the x / y outputs for the chord lengths
__global__ void __launch_bounds__(64) long_offsets_kernel(const OffsetsArgs a) {
#pragma clang fp contract(off)
    const int qp = blockIdx.x;
    const int n = a.m_spl;
    const double* tab = a.spl + (size_t)qp * 9 * n;
    const double* px = a.x + (size_t)qp * a.m;         // the points are read back from the outputs for the chord lengths
    const double* py = a.y + (size_t)qp * a.m;
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

// bspline_resample_kernel: ws = [batch][p_max + 6] knot vectors
__global__ void __launch_bounds__(64) long_bspline_kernel(const BsplineArgs a, double* __restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ int cnt_sh, deg_sh;
    const int qp = blockIdx.x;
    const int n = a.n_pts[qp];
    // the points from the input, the knot vector in the workspace ([batch][p_max + 6]), t in the `s` output until the chord lengths
    // overwrite it, the samples read back from the x / y outputs
    const double* ctrl = a.pts + (size_t)qp * a.p_max * 2;
    double* knots = ws + (size_t)qp * (a.p_max + 6);
    double* t_of = a.s + (size_t)qp * a.n_max;
    const double* px = a.x + (size_t)qp * a.n_max;
    const double* py = a.y + (size_t)qp * a.n_max;
    if (n < 4 || n > a.p_max) {             // reference_path_smoother.cpp:33-36
        if (threadIdx.x == 0) a.count[qp] = 0;
        return;
    }
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

// dp_corridor_kernel: ws = [batch][DpLongWs::doubles()]; the LDS holds DpLongLds
__global__ void __launch_bounds__(kDpThreads) long_dp_kernel(const DpArgs a, double* __restrict__ ws) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int qp = blockIdx.x, lane = threadIdx.x;          // lane < 64: the lateral sample `lane` in the per-node phases
    const double range = a.p.lateral_range, spacing = a.p.lateral_spacing;
    const int nlat = dp_lateral_samples(range, spacing);
    const DpLongLds L{nlat};
    const DpLongWs G{a.max_layers, nlat};
    const int n = a.m;
    const double* tab = a.spl + (size_t)qp * 9 * n;
    double* gw = ws + (size_t)qp * G.doubles();
    const double* ext = a.spl_ext + (size_t)qp * 4;
    const SplineView sx{tab, tab + n, tab + 2 * n, tab + 3 * n, tab + 4 * n, ext[0], ext[1], n};
    const SplineView sy{tab, tab + 5 * n, tab + 6 * n, tab + 7 * n, tab + 8 * n, ext[2], ext[3], n};
    const float* dist = a.dist + (size_t)(a.map_of ? a.map_of[qp] : 0) * a.g.rows * a.g.cols;
    double* s_layer = gw + G.s_layer();
    double* misc = lds + L.misc();
    double* ltab = lds + L.ltab();
    double* lay = gw + G.lay();
    double* self = lds + L.self();
    double* edge_cost = lds + L.edge();
    double* edge_dir = lds + L.edir();
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(gw + G.mask());
    unsigned char* parent = reinterpret_cast<unsigned char*>(gw + G.parent());
    int* path = reinterpret_cast<int*>(gw + G.path());
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
