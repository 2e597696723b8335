// pqp_bspline_body.inc — the body of bspline_resample_kernel (PQP_LINE_LONG = 0) and of its long form long_bspline_kernel (PQP_LINE_LONG = 1,
// PQP_OPT_LONG_LINES), pqp_corridor_kernels.inc, which says what the long forms are.  In scope there: `a` (BsplineArgs); in the long form also `ws`.
#pragma clang fp contract(off)
    __shared__ int cnt_sh, deg_sh;
    const int qp = blockIdx.x;
    const int n = a.n_pts[qp];
#if PQP_LINE_LONG
    // the points from the input, the knot vector in the workspace ([batch][p_max + 6]), t in the `s` output until the chord lengths
    // overwrite it, the samples read back from the x / y outputs
    const double* ctrl = a.pts + (size_t)qp * a.p_max * 2;
    double* knots = ws + (size_t)qp * (a.p_max + 6);
    double* t_of = a.s + (size_t)qp * a.n_max;
    const double* px = a.x + (size_t)qp * a.n_max;
    const double* py = a.y + (size_t)qp * a.n_max;
#else
    extern __shared__ __attribute__((aligned(16))) double lds[];          // [p_max][2] points, [p_max + 6] knots, [n_max] t, x, y
    double* ctrl = lds;
    double* knots = lds + 2 * a.p_max;
    double* t_of = knots + a.p_max + 6;
    double* px = t_of + a.n_max;
    double* py = px + a.n_max;
#endif
    if (n < 4 || n > a.p_max) {             // reference_path_smoother.cpp:33-36
        if (threadIdx.x == 0) a.count[qp] = 0;
        return;
    }
#if !PQP_LINE_LONG
    for (int k = threadIdx.x; k < 2 * n; k += blockDim.x) ctrl[k] = a.pts[(size_t)qp * a.p_max * 2 + k];
    __syncthreads();
#endif
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
#if !PQP_LINE_LONG
        px[i] = ox; py[i] = oy;
#endif
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
