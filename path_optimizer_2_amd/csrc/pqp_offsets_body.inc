// pqp_offsets_body.inc — the body of offsets_to_points_kernel (PQP_LINE_LONG = 0) and of its long form long_offsets_kernel (PQP_LINE_LONG = 1,
// PQP_OPT_LONG_LINES), pqp_corridor_kernels.inc, which says what the long forms are.  In scope there: `a` (OffsetsArgs).
#pragma clang fp contract(off)
#if !PQP_LINE_LONG
    extern __shared__ __attribute__((aligned(16))) double lds[];          // [9][m_spl] spline table, [m] x, [m] y
#endif
    const int qp = blockIdx.x;
    const int n = a.m_spl;
#if PQP_LINE_LONG
    const double* tab = a.spl + (size_t)qp * 9 * n;
    const double* px = a.x + (size_t)qp * a.m;         // the points are read back from the outputs for the chord lengths
    const double* py = a.y + (size_t)qp * a.m;
#else
    {
        const double* src = a.spl + (size_t)qp * 9 * n;
        for (int k = threadIdx.x; k < 9 * n; k += blockDim.x) lds[k] = src[k];
    }
    __syncthreads();
    const double* tab = lds;
    double* px = lds + 9 * n;
    double* py = px + a.m;
#endif
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
#if !PQP_LINE_LONG
        px[i] = x; py[i] = y;
#endif
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
