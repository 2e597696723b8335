// pqp_ref_states_body.inc — the body of reference_states_kernel (PQP_LINE_LONG = 0) and of its long form long_ref_states_kernel (PQP_LINE_LONG = 1,
// PQP_OPT_LONG_LINES), pqp_corridor_kernels.inc, which says what the long forms are.  In scope there: `a` (RefStatesArgs).
#pragma clang fp contract(off)
#if !PQP_LINE_LONG
    extern __shared__ __attribute__((aligned(16))) double lds[];          // [9][m] spline table, [n_max] abscissae
#endif
    __shared__ int cnt_sh;
    const int qp = blockIdx.x;
    const int n = a.m;
#if PQP_LINE_LONG
    // the walk's abscissae go straight to their output column (s of a reference state / the `s` list), where the lanes read them back
    const double* tab = a.spl + (size_t)qp * 9 * n;
    double* s_of = a.dynamic == 2 ? a.ls + (size_t)qp * a.n_max : a.ref + (size_t)qp * a.n_max * PQP_REF_STRIDE;
    const int s_step = a.dynamic == 2 ? 1 : PQP_REF_STRIDE;
#else
    {
        const double* src = a.spl + (size_t)qp * 9 * n;
        for (int k = threadIdx.x; k < 9 * n; k += blockDim.x) lds[k] = src[k];
    }
    __syncthreads();
    const double* tab = lds;
    double* s_of = lds + 9 * n;
    constexpr int s_step = 1;
#endif
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
        // isEqual(max_s_, 0.0) (FLAGS_epsilon = 1e-6, planning_flags.cpp:108): "ref length is zero", the reference returns false and builds
        // no state (:316-319)
        const bool zero_length = a.dynamic != 2 && fabs(max_s) < 1e-6;
        while (a.dynamic != 2 && !zero_length && tmp_s <= max_s && cnt < (1 << 20)) {
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
