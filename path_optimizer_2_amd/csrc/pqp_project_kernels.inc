// pqp_project_kernels.inc — included by pqp_lines.hip after pqp_corridor_kernels.inc.  Many points onto their reference line: Cartesian to
// Frenet (pqp_project_points), the inverse of pqp_offsets_to_points.
//   getProjection / getProjectionByNewton      src/tools/tools.cpp:66-126
//   getHeading, getCurvature, global2Local     src/tools/tools.cpp:32-44, 57-64
//   the signed offset and the heading error    src/path_optimizer.cpp:73-85, src/reference_path_smoother/reference_path_smoother.cpp:148-165
// spline_projection_wave (pqp_line_device.hpp) is the same search for ONE point of a line.  Its 1 m coarse scan evaluates the spline at
// 0, 1, 2, ... <= length whatever the point is, so here a workgroup makes those evaluations once - one sample per lane, spline_eval3 on the
// table where it lies (HBM through L2: ~log2(m) knots per evaluation, no knot-count cap, no workspace) - and leaves them in LDS, 16 bytes per
// sample, kProjectTile samples at a time with the end sample behind them.  Then every lane owns one point and scans the samples: all
// lanes read the same address, a broadcast without a bank conflict.  A lane carries its running minimum from tile to tile, so the first
// strict minimum wins across tile borders as in the serial scan; the end compare and the Newton steps are spline_projection_wave's, word for word.
//
// The scan compares sqrt(dx*dx + dy*dy) as the reference does, but takes the square root only of a candidate: with d2 the squared distance
// of a sample and best2 that of the minimum so far, d2 >= best2 implies sqrt(d2) >= sqrt(best2) (a correctly rounded square root is
// monotone), which the reference's strict `<` rejects; only d2 < best2 needs the root and the reference's own compare.  The first minimum,
// hence s, is bit for bit what spline_projection_wave returns.

namespace pqp {

constexpr int kProjectThreads = 256;                  // points of a workgroup, one per lane
constexpr int kProjectTile = PQP_PROJECT_TILE_SAMPLES;
// the reference's scan has floor(length) + 1 steps: an infinite length would never end it and an absurd one would hold a compute unit for
// seconds, so a line of 2^20 m (1049 km, 1024 tiles per workgroup) and more is refused like a point that is not finite
constexpr double kProjectMaxLength = 1048576.0;

struct ProjectArgs {
    int batch, m, q_max, stride, has_heading;
    const double* spl;               // [batch][9][m]
    const double* spl_ext;           // [batch][4]
    const double* length;            // [batch]
    const double* points;            // [batch][q_max][stride]  x, y (, heading) at offsets 0, 1 (, 2)
    const int32_t* q_of;             // [batch] points of each line, or nullptr: all have q_max
    double* proj;                    // [batch][q_max][PQP_PROJ_STRIDE]  s, l, t, d_heading, x_p, y_p, heading_p, k_p
    int32_t* flags;                  // [batch][q_max]
};

__global__ void __launch_bounds__(kProjectThreads) project_points_kernel(const ProjectArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double smp[2 * (kProjectTile + 1)];      // x, y of a tile of coarse samples; the end sample last
    const int line = blockIdx.x;
    const int q = blockIdx.y * kProjectThreads + threadIdx.x;
    const int count = a.q_of ? min(max(a.q_of[line], 0), a.q_max) : a.q_max;
    const size_t row = (size_t)line * a.q_max + q;
    if ((int)(blockIdx.y * kProjectThreads) >= count) {          // (the whole workgroup: no barrier below is reached by a part of it)
        if (q < a.q_max) {
#pragma unroll
            for (int c = 0; c < PQP_PROJ_STRIDE; ++c) a.proj[row * PQP_PROJ_STRIDE + c] = 0.0;
            a.flags[row] = 0;
        }
        return;
    }
    const int n = a.m;
    const double* tab = a.spl + (size_t)line * 9 * n;
    const double* ext = a.spl_ext + (size_t)line * 4;
    const SplineView sx{tab, tab + n, tab + 2 * n, tab + 3 * n, tab + 4 * n, ext[0], ext[1], n};
    const SplineView sy{tab, tab + 5 * n, tab + 6 * n, tab + 7 * n, tab + 8 * n, ext[2], ext[3], n};
    const double L = a.length[line];
    const bool scan = L > 0.0 && L < kProjectMaxLength;            // (the same in every lane)
    const bool too_long = L >= kProjectMaxLength;
    const bool mine = q < count;
    double tx = 0.0, ty = 0.0, th = 0.0;
    if (mine) {
        const double* p = a.points + row * a.stride;
        tx = p[0]; ty = p[1];
        if (a.has_heading) th = p[2];
    }
    bool bad = !(isfinite(tx) && isfinite(ty) && isfinite(th)) || too_long;
    bool not_converged = false;
    double s = 0.0;
    if (scan) {
        const int last = (int)L;                                   // samples 0 .. last, (double)k <= L exactly as the serial scan counts them
        double best = 1.7976931348623157e308, best2 = INFINITY, best_s = 0.0;
        for (int base = 0; base <= last; base += kProjectTile) {
            const int here = min(kProjectTile, last - base + 1);
            if (base) __syncthreads();                             // the previous tile has been scanned
            for (int j = threadIdx.x; j < here; j += kProjectThreads) {
                double x, y, d1, d2;
                spline_eval3(sx, (double)(base + j), x, d1, d2); spline_eval3(sy, (double)(base + j), y, d1, d2);
                smp[2 * j] = x; smp[2 * j + 1] = y;
            }
            if (base == 0 && threadIdx.x == kProjectThreads - 1) {
                double x, y, d1, d2;
                spline_eval3(sx, L, x, d1, d2); spline_eval3(sy, L, y, d1, d2);
                smp[2 * kProjectTile] = x; smp[2 * kProjectTile + 1] = y;
            }
            __syncthreads();
            for (int j = 0; j < here; ++j) {
                const double x = smp[2 * j], y = smp[2 * j + 1];
                const double dd = (x - tx) * (x - tx) + (y - ty) * (y - ty);
                if (dd < best2) {
                    const double d = sqrt(dd);
                    if (d < best) { best = d; best2 = dd; best_s = (double)(base + j); }
                }
            }
        }
        const double xe = smp[2 * kProjectTile], ye = smp[2 * kProjectTile + 1];
        if (sqrt((xe - tx) * (xe - tx) + (ye - ty) * (ye - ty)) < best) {
            s = L;
        } else if (mine && !bad) {
            double cur = fmin(best_s, L), prev = cur;
            not_converged = true;
            for (int it = 0; it < 20; ++it) {
                double x, dx, ddx, y, dy, ddy;
                spline_eval3(sx, cur, x, dx, ddx); spline_eval3(sy, cur, y, dy, ddy);
                const double j = (x - tx) * dx + (y - ty) * dy;
                const double h = dx * dx + (x - tx) * ddx + dy * dy + (y - ty) * ddy;
                cur -= j / h;
                if (!isfinite(cur)) { bad = true; break; }
                if (fabs(cur - prev) < 1e-5) { not_converged = false; break; }
                prev = cur;
            }
            s = fmin(cur, L);
        }
    }
    if (q >= a.q_max) return;
    double* o = a.proj + row * PQP_PROJ_STRIDE;
    if (!mine) {
#pragma unroll
        for (int c = 0; c < PQP_PROJ_STRIDE; ++c) o[c] = 0.0;
        a.flags[row] = 0;
        return;
    }
    if (bad) {
#pragma unroll
        for (int c = 0; c < PQP_PROJ_STRIDE; ++c) o[c] = NAN;
        a.flags[row] = PQP_PROJ_NOT_FINITE;
        return;
    }
    double xp, dx, ddx, yp, dy, ddy;
    spline_eval3(sx, s, xp, dx, ddx); spline_eval3(sy, s, yp, dy, ddy);
    const double hp = atan2(dy, dx);                                       // getHeading
    const double ch = cos(hp), sh = sin(hp);
    const double ex = tx - xp, ey = ty - yp;                               // global2Local((x_p, y_p, heading_p), point)
    o[0] = s;
    o[1] = -ex * sh + ey * ch;
    o[2] = ex * ch + ey * sh;
    o[3] = a.has_heading ? constrain_angle(th - hp) : 0.0;                 // path_optimizer.cpp:83
    o[4] = xp;
    o[5] = yp;
    o[6] = hp;
    o[7] = curvature_of(dx, dy, ddx, ddy);
    a.flags[row] = (s == L ? PQP_PROJ_AT_END : 0) | (s < 0.0 ? PQP_PROJ_BEFORE_START : 0) | (not_converged ? PQP_PROJ_NOT_CONVERGED : 0);
}

}  // namespace pqp
