// pqp_dp_body.inc — the body of dp_corridor_kernel (PQP_LINE_LONG = 0) and of its long form long_dp_kernel (PQP_LINE_LONG = 1,
// PQP_OPT_LONG_LINES), pqp_corridor_kernels.inc, which says what the long forms are.  In scope there: `a` (DpArgs); in the long form also `ws`.
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int qp = blockIdx.x, lane = threadIdx.x;          // lane < 64: the lateral sample `lane` in the per-node phases
    const double range = a.p.lateral_range, spacing = a.p.lateral_spacing;
    const int nlat = dp_lateral_samples(range, spacing);
    const int n = a.m;
    // L: the arrays in the LDS; G: the block of the per-layer arrays, at `per` - the LDS again, or the scenario's slice of the workspace
#if PQP_LINE_LONG
    const DpBlock<false, true> L{a.m, a.max_layers, nlat};
    const DpBlock<true, false> G{a.m, a.max_layers, nlat};
    const double* tab = a.spl + (size_t)qp * 9 * n;
    double* per = ws + (size_t)qp * G.doubles();
#else
    const DpBlock<true, true> L{a.m, a.max_layers, nlat}, G = L;
    {
        const double* src = a.spl + (size_t)qp * 9 * n;
        for (int k = lane; k < 9 * n; k += kDpThreads) lds[k] = src[k];
    }
    __syncthreads();
    const double* tab = lds;
    double* per = lds;
#endif
    const double* ext = a.spl_ext + (size_t)qp * 4;
    const SplineView sx{tab, tab + n, tab + 2 * n, tab + 3 * n, tab + 4 * n, ext[0], ext[1], n};
    const SplineView sy{tab, tab + 5 * n, tab + 6 * n, tab + 7 * n, tab + 8 * n, ext[2], ext[3], n};
    const float* dist = a.dist + (size_t)(a.map_of ? a.map_of[qp] : 0) * a.g.rows * a.g.cols;
    double* s_layer = per + G.s_layer();
    double* misc = lds + L.misc();
    double* ltab = lds + L.ltab();
    double* lay = per + G.lay();
    double* self = lds + L.self();
    double* edge_cost = lds + L.edge();
    double* edge_dir = lds + L.edir();
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(per + G.mask());
    unsigned char* parent = reinterpret_cast<unsigned char*>(per + G.parent());
    // behind the parents; each form keeps its own expression of that address, which its gfx950 code follows
#if PQP_LINE_LONG
    int* path = reinterpret_cast<int*>(per + G.path());
#else
    int* path = reinterpret_cast<int*>(parent + G.parent_bytes());
#endif
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
