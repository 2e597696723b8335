// pqp_spline_fit_body.inc — the body of spline_fit_kernel (PQP_LINE_LONG = 0) and of its long form long_fit_kernel (PQP_LINE_LONG = 1,
// PQP_OPT_LONG_LINES), pqp_corridor_kernels.inc, which says what the long forms are.  In scope there: `a` (SplineFitArgs); in the long form also `ws`.
    // knots, values, h, d, right-hand sides / moments, sweep work / cubic coefficients, linear coefficients: [7][m], in LDS or - the long
    // form - the (scenario, coordinate)'s slice of the workspace, which the two sweeps stream through
#if !PQP_LINE_LONG
    extern __shared__ __attribute__((aligned(16))) double lds[];
#endif
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
#if PQP_LINE_LONG
    double* x = ws + (size_t)idx * 7 * stride;
#else
    double* x = lds;
#endif
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
