// pqp_corridor_body.inc — the four phases of the corridor walk, included as the body of corridor_bounds_kernel
// (ReferencePathImpl::updateBoundsImproved) and of states_bounds_kernel (updateBoundsOnInputStates), pqp_corridor_kernels.inc.
// In scope there: `a` (CorridorArgs); with PQP_CORRIDOR_ON_STATES = 1 also `states` and `stride`, which only phase 1 reads.
// With PQP_CORRIDOR_LONG = 1 (long_corridor_kernel / long_states_kernel; PQP_OPT_LONG_LINES) the spline table
// stays in HBM and the LDS holds the probes of a tile alone: the Newton projection's few evaluations per task read the table through the caches.
// (One text in two kernels rather than a __device__ function both call: such a function is simplified on its own before it is inlined,
//  where the kernel arguments are loads through a pointer, and corridor_bounds_kernel's gfx950 code came out different.  The same was seen
//  for the five pqp_*_body.inc of the line kernels - as a template <bool kLong> __forceinline__ function taking the arguments by reference
//  or by value, spline_fit_kernel kept its 649 instructions with operands of commutative ones swapped, the others changed in count - but not
//  for reference_length_kernel, whose body is such a function.)
#pragma clang fp contract(off)
    __shared__ int first_blocked;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int qp = blockIdx.x;
    const int nq = a.n_of ? (a.n_of[qp] < a.n ? a.n_of[qp] : a.n) : a.n;
#if defined(PQP_CORRIDOR_LONG) && PQP_CORRIDOR_LONG
    const CorridorLds L{0, a.tile};
#else
    const CorridorLds L{a.m, a.tile};
#endif
    int ncoarse = (int)(a.p.search_range / a.p.delta_s);                     // 20 (:243)
    ncoarse = ncoarse > 32 ? 32 : ncoarse;
    const int nfine = (int)(a.p.delta_s / a.p.smaller_ds) - 1;               // static_cast<int>(0.3 / 0.05) = 5: steps i = 1..4 (:278)
    const double radius = a.p.search_radius, ds2 = a.p.smaller_ds;
    int* first = reinterpret_cast<int*>(lds + L.first());
    if (threadIdx.x == 0) {
        first_blocked = nq;
        double acc = 0.0;
        for (int j = 0; j < ncoarse; ++j) { acc += a.p.delta_s; lds[L.acc() + j] = acc; }
    }
#if defined(PQP_CORRIDOR_LONG) && PQP_CORRIDOR_LONG
    const float* dist = a.dist + (size_t)(a.map_of ? a.map_of[qp] : 0) * a.g.rows * a.g.cols;
    const double* tab = a.spl + (size_t)qp * 9 * a.m;
#else
    {
        const double* src = a.spl + (size_t)qp * 9 * a.m;
        for (int k = threadIdx.x; k < 9 * a.m; k += blockDim.x) lds[k] = src[k];
    }
    const float* dist = a.dist + (size_t)(a.map_of ? a.map_of[qp] : 0) * a.g.rows * a.g.cols;
    const double* tab = lds;
#endif
    const double* ext = a.spl_ext + (size_t)qp * 4;
    const SplineView sx{tab, tab + a.m, tab + 2 * a.m, tab + 3 * a.m, tab + 4 * a.m, ext[0], ext[1], a.m};
    const SplineView sy{tab, tab + 5 * a.m, tab + 6 * a.m, tab + 7 * a.m, tab + 8 * a.m, ext[2], ext[3], a.m};
    // (the waypoints are independent of each other - only the index of the first blocked one joins them -: a path longer than the LDS holds
    //  goes through in tiles of a.tile waypoints, each the same four phases)
    for (int i0 = 0; i0 < nq; i0 += a.tile) {
        const int ntask = 3 * (nq - i0 < a.tile ? nq - i0 : a.tile);
        for (int k = threadIdx.x; k < 2 * ntask; k += blockDim.x) first[k] = ncoarse;
        __syncthreads();

        // phase 1: probe origin of every (waypoint, circle): the circle centre projected on the line (front, rear) or the state itself
        for (int t = threadIdx.x; t < ntask; t += blockDim.x) {
            const int i = i0 + t / 3, part = t - 3 * (t / 3);
            const double* r = a.ref + ((size_t)qp * a.n + i) * PQP_REF_STRIDE;
            const double s = r[0], heading = r[2], x = r[3], y = r[4];
            double px = x, py = y, off = 0.0;
            if (part != 2) {
                const double len = part == 0 ? a.p.front_length : a.p.rear_length;
                const double ch = cos(heading), sh = sin(heading);
#if PQP_CORRIDOR_ON_STATES
                // front_length_new = FLAGS_front_length - FLAGS_front_length * cos(d_heading) (:127-128; rear alike); the Newton
                // guess below keeps the flag's length (:139-150).  A d_heading that is not finite gives NaN centres, hence NaN
                // front / rear rows, never blocked - as in the reference.
                const double clen = len - len * cos(states[((size_t)qp * a.n + i) * stride + 4]);
#else
                const double clen = len;
#endif
                const double cx = x + clen * ch, cy = y + clen * sh;
                // getDirectionalProjectionByNewton(xs, ys, cx, cy, heading + pi/2, s + 5, s + len)
                const double max_s = s + a.p.projection_window;
                const double angle = heading + kPi2;
                const double v1 = sin(angle), v2 = -cos(angle);
                double cur = fmin(s + len, max_s), prev = cur;
                for (int it = 0; it < 20; ++it) {
                    double fxv, dxv, ddx, fyv, dyv, ddy;
                    spline_eval3(sx, cur, fxv, dxv, ddx);
                    spline_eval3(sy, cur, fyv, dyv, ddy);
                    const double p1 = v1 * (fxv - cx) + v2 * (fyv - cy);
                    const double p2 = v1 * dxv + v2 * dyv;
                    const double j = p1 * p2;
                    const double h = p1 * (v1 * ddx + v2 * ddy) + p2 * p2;
                    cur -= j / h;
                    if (fabs(cur - prev) < 1e-5) break;
                    prev = cur;
                }
                cur = fmin(cur, max_s);
                double d1, d2;
                spline_eval3(sx, cur, px, d1, d2);
                spline_eval3(sy, cur, py, d1, d2);
                const double dx = px - cx, dy = py - cy;        // offset = global2Local(circle centre, projection).y   (tools.cpp:57-64)
                off = -dx * sh + dy * ch;
            }
            const double left_angle = constrain_angle(heading + kPi2), right_angle = constrain_angle(heading - kPi2);
            double* o = lds + L.org() + 8 * t;
            o[0] = px; o[1] = py; o[2] = off;
            o[3] = cos(left_angle); o[4] = sin(left_angle); o[5] = cos(right_angle); o[6] = sin(right_angle);
            o[7] = obstacle_distance(dist, a.g, px, py) > radius ? 1.0 : 0.0;       // "original position is collision free" (:246)
        }
        __syncthreads();

        // phase 2: coarse samples (task, side, j): origin + acc[j] * normal (:249-270); first failing j per (task, side)
        // (w / ncoarse by the float reciprocal: exact below 2^22 work items - (w + 0.5) / n is at least 0.5 / n away from an integer -, a few
        //  instructions where the 32-bit integer division takes ~25)
        const float inv_coarse = 1.0f / (float)ncoarse, inv_fine = 1.0f / (float)(nfine > 0 ? nfine : 1);
        for (int w = threadIdx.x; w < ntask * 2 * ncoarse; w += blockDim.x) {
            int ts = (int)(((float)w + 0.5f) * inv_coarse), j = w - ts * ncoarse;
            if (j < 0) { ts -= 1; j += ncoarse; } else if (j >= ncoarse) { ts += 1; j -= ncoarse; }      // (never taken below 2^22 items; kept as the guarantee)
            const int side = ts & 1, t = ts >> 1;        // side 0 = left, 1 = right
            const double* o = lds + L.org() + 8 * t;
            if (o[7] == 0.0) continue;
            const double st = lds[L.acc() + j];
            const double c = side ? o[5] : o[3], sn = side ? o[6] : o[4];
            if (obstacle_distance(dist, a.g, o[0] + st * c, o[1] + st * sn) < radius) atomicMin(&first[ts], j);
        }
        __syncthreads();
        // the walk's left_s / right_s when it stops -> left_bound / right_bound (:271-272); re-arm first[] for the fine steps
        for (int ts = threadIdx.x; ts < 2 * ntask; ts += blockDim.x) {
            const int jf = first[ts];
            const double s_end = lds[L.acc() + (jf < ncoarse ? jf : ncoarse - 1)];
            lds[L.cend() + ts] = (ts & 1) ? -(s_end - a.p.delta_s) : (s_end - a.p.delta_s);
            first[ts] = nfine + 1;
        }
        __syncthreads();

        // phase 3: fine samples (task, side, k), k = 1..nfine (:277-300).  As written in the reference the right-hand probe is
        //          state + right_bound * (cos, sin)(right_angle) with right_bound negative, i.e. it samples the LEFT side.
        for (int w = threadIdx.x; w < ntask * 2 * (nfine > 0 ? nfine : 0); w += blockDim.x) {
            int ts = (int)(((float)w + 0.5f) * inv_fine), k = w - ts * nfine;
            if (k < 0) { ts -= 1; k += nfine; } else if (k >= nfine) { ts += 1; k -= nfine; }
            k += 1;
            const int side = ts & 1, t = ts >> 1;
            const double* o = lds + L.org() + 8 * t;
            if (o[7] == 0.0) continue;
            double v = lds[L.cend() + ts];
            for (int q = 0; q < k; ++q) v = side ? v - ds2 : v + ds2;
            const double c = side ? o[5] : o[3], sn = side ? o[6] : o[4];
            if (obstacle_distance(dist, a.g, o[0] + v * c, o[1] + v * sn) < radius) atomicMin(&first[ts], k);
        }
        __syncthreads();

        // phase 4: margins (:301-311), offset, blocked test (:219), output
        for (int t = threadIdx.x; t < ntask; t += blockDim.x) {
            const int i = i0 + t / 3, part = t - 3 * (t / 3);
            const double* o = lds + L.org() + 8 * t;
            double ub = 0.0, lb = 0.0;
            if (o[7] != 0.0) {
                double left = lds[L.cend() + 2 * t], right = lds[L.cend() + 2 * t + 1];
                const int kl = first[2 * t], kr = first[2 * t + 1];
                for (int q = 0; q < (kl <= nfine ? kl : nfine); ++q) left += ds2;
                if (kl <= nfine) left -= ds2;                       // the failing step is undone
                for (int q = 0; q < (kr <= nfine ? kr : nfine); ++q) right -= ds2;
                if (kr <= nfine) right += ds2;
                const double diff_radius = a.p.car_width * 0.5 - radius;
                left -= diff_radius;
                right += diff_radius;
                if (!(left < right)) {
                    const double space = left - right;
                    const double max_margin = fmax(0.0, (space - a.p.min_space) / 2.0);
                    const double margin = fmin(a.p.safety_margin, max_margin);
                    ub = left - margin;
                    lb = right + margin;
                }
            }
            if (part != 2) {
                ub += o[2]; lb += o[2];
                if (fabs(ub - lb) < a.p.epsilon) atomicMin(&first_blocked, i);         // isEqual(bound[0], bound[1]) -> blocked (:219)
            }
            double* out = a.bounds + ((size_t)qp * a.n + i) * PQP_BOUNDS_STRIDE + 2 * part;
            out[0] = lb; out[1] = ub;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) a.n_valid[qp] = first_blocked;
