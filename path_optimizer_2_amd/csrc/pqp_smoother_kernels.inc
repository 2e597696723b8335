// pqp_smoother_kernels.inc — included by pqp_smoothers.hip.  GPU side of the reference-line smoothing QPs
// (SURVEY.md §8a rows S1-S3): per-type assemble kernels (values in the point-interleaved order that makes the reduced
// KKT banded), the generic banded ADMM solve kernel (pqp_banded_qp.hpp) and the per-type finish kernels - the reference's
// formulation and iteration, what a handle with polish = 0 runs -, and the exact kernels for handles that ask for optima:
// tension2_exact_kernel (S1: a Riccati sweep, one lane per scenario), tension_exact_kernel / post_exact_kernel (S2 / S3: box QPs
// in one unknown per point, active-set rounds with a banded LDL^T run down a wavefront's lanes).

namespace pqp {

// ---- device context of the banded core: one workgroup per QP, one lane per (padded) variable --------------------------
template <int K, bool MAX>
__device__ __forceinline__ void wg_reduce_dyn(double (&v)[K], double* red) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = MAX ? wave_max(v[k]) : wave_sum(v[k]);        // DPP, wave-uniform (pqp_wave.hpp)
    const int nw = (blockDim.x + 63) >> 6;
    if (nw > 1) {
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < K; ++k) red[k * 16 + w] = v[k];
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            double x = red[k * 16];
            for (int j = 1; j < nw; ++j) x = MAX ? fmax(x, red[k * 16 + j]) : x + red[k * 16 + j];
            v[k] = uniform(x);
        }
    }
    __syncthreads();
}

template <int B, bool STAGE>
struct BqDevCtx {
    static constexpr bool kStage = STAGE;
    BqLane<B> lane;
    double* shp;
    double* red;
    __device__ __forceinline__ int T() const { return (int)blockDim.x; }
    __device__ __forceinline__ double* sh() { return shp; }
    template <class F>
    __device__ __forceinline__ void phase(F f) {
        f((int)threadIdx.x, lane);
        __syncthreads();
    }
    template <int K, class F>
    __device__ __forceinline__ void reduce_max(double (&out)[K], F f) {
        f((int)threadIdx.x, out);
        wg_reduce_dyn<K, true>(out, red);
    }
    template <int K, class F>
    __device__ __forceinline__ void reduce_sum(double (&out)[K], F f) {
        f((int)threadIdx.x, out);
        wg_reduce_dyn<K, false>(out, red);
    }
};

// up to 16 wavefronts per QP (1024 padded variables).  Up to 256 threads a lane may use 512 registers, up to 512 threads
// 256; the 1024-thread variant (128 registers, spills) is the fallback for long reference lines.
// STAGE: the row data of A, the index lists and q in LDS (BqLayout::total(true)); the host picks it whenever that fits.
template <int B, int MAXT, bool STAGE>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 && B <= 4) ? 2 : 1) banded_solve_kernel(const BandedQpArgs args) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    for (int qp = blockIdx.x; qp < args.batch; qp += gridDim.x) {
        BqDevCtx<B, STAGE> ctx;
        ctx.shp = smem;
        ctx.red = smem + BqLayout{args.nv, args.nc, args.bw}.red();
        BandedQp<BqDevCtx<B, STAGE>, B> s(ctx, args, qp);
        s.run();
        __syncthreads();
    }
}

// ---- S1: TensionSmoother2 (tension_smoother_2.cpp:74-158).  Interleave (x, y, theta, k)_i -> 4i + {0,1,2,3} -----------
//   rows (reference order): i: x_{i+1} - x_i + ds sin(phi_i) theta_i = ds cos(phi_i)          (:121-126,135-136)
//                           (n-1)+i: y_{i+1} - y_i - ds cos(phi_i) theta_i = ds sin(phi_i)    (:122-127,137-138)
//                           2(n-1)+i: theta_{i+1} - theta_i - ds k_i = -ds k_list[i]          (:123-128,139-140)
//                           3(n-1), 3(n-1)+1: x_0 = x_list[0], y_0 = y_list[0]                (:130,143-144)
// n_of (or nullptr): points of each scenario.  The batch shares ONE sparsity pattern (that of n points); a scenario with fewer points is
// the same QP padded with decoupled dummies - points i >= n_of get unit cost and no rows, the rows that would couple them are zero rows
// with infinite bounds - so its real part has exactly the reference's optimum.
__global__ void tension2_assemble_kernel(int batch, int n, const int32_t* __restrict__ n_of, const double* __restrict__ xl,
                                         const double* __restrict__ yl, const double* __restrict__ al, const double* __restrict__ kl,
                                         const double* __restrict__ sl, double w_dev, double w_k, double w_dk, double* __restrict__ pband,
                                         double* __restrict__ q, double* __restrict__ aval, double* __restrict__ lo, double* __restrict__ up) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * n) return;
    const int b = idx / n, i = idx - b * n;
    const int nv = 4 * n - 1, nc = 3 * (n - 1) + 2;
    const int nq = n_of ? (n_of[b] < n ? (n_of[b] < 2 ? 2 : n_of[b]) : n) : n;
    if (i >= nq || (i == nq - 1 && nq < n)) {
        // a dummy point (i >= nq) or the last real point of a shortened line (its curvature variable and its rows do not exist)
        double* pbd = pband + (size_t)b * 5 * nv;
        double* qd = q + (size_t)b * nv;
        double* avd = aval + (size_t)b * nc * kRMax;
        const bool real_point = i < nq;
        for (int d = 0; d < 5; ++d) for (int c = 0; c < 4; ++c) if (4 * i + c < nv) pbd[(size_t)d * nv + 4 * i + c] = 0.0;
        for (int c = 0; c < 4; ++c) if (4 * i + c < nv) { pbd[4 * i + c] = (real_point && c < 2) ? w_dev * 2 : (real_point && c == 2 ? 0.0 : 1.0); qd[4 * i + c] = 0.0; }
        if (real_point) { qd[4 * i] = -2 * w_dev * xl[idx]; qd[4 * i + 1] = -2 * w_dev * yl[idx]; }
        if (i < n - 1)
            for (int r = 0; r < 3; ++r) {
                double* row = avd + (size_t)(r * (n - 1) + i) * kRMax;
                row[0] = row[1] = row[2] = row[3] = 0.0;
                lo[(size_t)b * nc + r * (n - 1) + i] = -1e30; up[(size_t)b * nc + r * (n - 1) + i] = 1e30;
            }
        return;
    }
    n = nq;                      // (below: the reference's assembly of a line of nq points, in the pattern of the launch)
    const int n_pat = (nc - 2) / 3 + 1;
    double* pb = pband + (size_t)b * 5 * nv;
    double* qq = q + (size_t)b * nv;
    double* av = aval + (size_t)b * nc * kRMax;
    double* l = lo + (size_t)b * nc;
    double* u = up + (size_t)b * nc;
    const double x = xl[idx], y = yl[idx];
    // Hessian (:82-92): 2 w_dev on x, y; 2 w_k on k; 2 w_dk [[1,-1],[-1,1]] on consecutive k
    for (int d = 0; d < 5; ++d) { pb[(size_t)d * nv + 4 * i] = 0.0; pb[(size_t)d * nv + 4 * i + 1] = 0.0; pb[(size_t)d * nv + 4 * i + 2] = 0.0; }
    pb[4 * i] = w_dev * 2; pb[4 * i + 1] = w_dev * 2;
    if (i < n - 1) {
        for (int d = 0; d < 5; ++d) pb[(size_t)d * nv + 4 * i + 3] = 0.0;
        double pk = w_k * 2;
        if (i <= n - 3) { pk += 2 * w_dk; pb[(size_t)4 * nv + 4 * i + 3] = -2 * w_dk; }
        if (i >= 1) pk += 2 * w_dk;
        pb[4 * i + 3] = pk;
    }
    // gradient (:147-158)
    qq[4 * i] = -2 * w_dev * x; qq[4 * i + 1] = -2 * w_dev * y; qq[4 * i + 2] = 0.0;
    if (i < n - 1) qq[4 * i + 3] = 0.0;
    if (i < n - 1) {
        const double ds = sl[idx + 1] - sl[idx];
        const double sn = sin(al[idx]), cs = cos(al[idx]);
        double* r0 = av + (size_t)i * kRMax;
        double* r1 = av + (size_t)(n_pat - 1 + i) * kRMax;
        double* r2 = av + (size_t)(2 * (n_pat - 1) + i) * kRMax;
        r0[0] = 1.0; r0[1] = -1.0; r0[2] = ds * sn; r0[3] = 0.0;
        r1[0] = 1.0; r1[1] = -1.0; r1[2] = -ds * cs; r1[3] = 0.0;
        r2[0] = 1.0; r2[1] = -1.0; r2[2] = -ds; r2[3] = 0.0;
        l[i] = u[i] = ds * cs;
        l[n_pat - 1 + i] = u[n_pat - 1 + i] = ds * sn;
        l[2 * (n_pat - 1) + i] = u[2 * (n_pat - 1) + i] = -ds * kl[idx];
    }
    if (i == 0) {
        double* r3 = av + (size_t)(3 * (n_pat - 1)) * kRMax;
        r3[0] = 1.0; r3[1] = r3[2] = r3[3] = 0.0; r3[4] = 1.0; r3[5] = r3[6] = r3[7] = 0.0;
        l[3 * (n_pat - 1)] = u[3 * (n_pat - 1)] = x;
        l[3 * (n_pat - 1) + 1] = u[3 * (n_pat - 1) + 1] = y;
    }
}

// ---- S1, exact: TensionSmoother2's QP as the linear-quadratic control problem it is, one LANE per scenario ---------------------------------
// Every row of the QP is an equality (tension_smoother_2.cpp:119-145): with the state (x, y, theta)_i and the control k_i the rows are the
// dynamics  x' = x - h sin(phi) theta + h cos(phi),  y' = y + h cos(phi) theta + h sin(phi),  theta' = theta + h k - h k_list   (h = ds_i),
// the cost is  w_dev sum ((x - X)^2 + (y - Y)^2) + w_k sum k_i^2 + w_dk sum (k_{i+1} - k_i)^2  (the Hessian and gradient of :82-92,147-158 up to
// a constant), x_0 and y_0 are given and theta_0 is free.  Its optimum is one backward Riccati sweep over the points - state (x, y, theta,
// previous k), 4 x 4 value matrices, a scalar control - the minimisation over theta_0, and one forward sweep that also accumulates the chord
// lengths (tension_smoother_2.cpp:61-70): 2 n sequential steps of ~150 flops with no search and no iteration, where the KKT system of the
// 4n-variable formulation needs a block factorisation across up to 1024 lanes.  A lane runs one scenario; the feedback gains of the backward
// sweep (5 doubles per point) live in a workspace laid out [point][k][scenario] so that a wavefront's accesses coalesce.  Coordinates are
// taken relative to the first point.  Used for handles with polish != 0 (exact optima; pqp_banded_qp.hpp: "solved as the polish solves it");
// the reference's ADMM setting runs the reference's formulation on the generic core.
// stage data of the sweeps, computed by one thread per (scenario, point) and laid out [point][6][scenario] so that the sweeps' loads coalesce:
// X - X_0, Y - Y_0, a = h sin(phi), b = h cos(phi), -h k_list, h   (the sines and cosines would otherwise sit on the sweeps' critical path)
__global__ void tension2_stage_kernel(int batch, int n, const int32_t* __restrict__ n_of, const double* __restrict__ xl, const double* __restrict__ yl,
                                      const double* __restrict__ al, const double* __restrict__ kl, const double* __restrict__ sl, double* __restrict__ sd) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * n) return;
    const int b = idx / n, i = idx - b * n;
    int nq = n_of ? n_of[b] : n;
    nq = nq < 2 ? 2 : (nq > n ? n : nq);
    if (i >= nq) return;
    const size_t row = (size_t)b * n;
    double* o = sd + (size_t)i * 6 * batch + b;
    o[0] = xl[idx] - xl[row]; o[batch] = yl[idx] - yl[row];
    double h = 0.0, sn = 0.0, cs = 0.0, kk = 0.0;
    if (i + 1 < nq) { h = sl[idx + 1] - sl[idx]; sincos(al[idx], &sn, &cs); kk = kl[idx]; }
    o[2 * (size_t)batch] = h * sn; o[3 * (size_t)batch] = h * cs; o[4 * (size_t)batch] = -h * kk; o[5 * (size_t)batch] = h;
}
__global__ void __launch_bounds__(64) tension2_exact_kernel(int batch, int n, const int32_t* __restrict__ n_of, const double* __restrict__ xl,
                                                            const double* __restrict__ yl, double w_dev, double w_k, double w_dk, const double* __restrict__ sd,
                                                            double* __restrict__ ws, double* __restrict__ ox, double* __restrict__ oy, double* __restrict__ os,
                                                            int32_t* __restrict__ status, int32_t* __restrict__ iters, double* __restrict__ info) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    int nq = n_of ? n_of[b] : n;
    nq = nq < 2 ? 2 : (nq > n ? n : nq);
    const size_t row = (size_t)b * n;
    const double X0 = xl[row], Y0 = yl[row];
    const double wd2 = 2.0 * w_dev;
    const size_t B1 = (size_t)batch;
    const double* sdb = sd + b;
    // value function after the last point: w_dev ((x - X)^2 + (y - Y)^2)
    double sxx = wd2, sxy = 0.0, sxt = 0.0, sxk = 0.0, syy = wd2, syt = 0.0, syk = 0.0, stt = 0.0, stk = 0.0, skk = 0.0;
    double vx = -wd2 * sdb[(size_t)(nq - 1) * 6 * B1], vy = -wd2 * sdb[((size_t)(nq - 1) * 6 + 1) * B1], vt = 0.0, vk = 0.0;
    // inputs of stage i, fetched one stage ahead of their use
    double nX, nY, na, nb, nc, nh;
    { const double* g = sdb + (size_t)(nq - 2) * 6 * B1; nX = g[0]; nY = g[B1]; na = g[2 * B1]; nb = g[3 * B1]; nc = g[4 * B1]; nh = g[5 * B1]; }
    for (int i = nq - 2; i >= 0; --i) {
        const double Xc = nX, Yc = nY, a = na, bb = nb, c2 = nc, hc = nh;
        if (i > 0) { const double* g = sdb + (size_t)(i - 1) * 6 * B1; nX = g[0]; nY = g[B1]; na = g[2 * B1]; nb = g[3 * B1]; nc = g[4 * B1]; nh = g[5 * B1]; }
        const double dk = i >= 1 ? 2.0 * w_dk : 0.0;
        // t = S' c + v', c = (bb, a, -h k_list, 0)
        const double tx = sxx * bb + sxy * a + sxt * c2 + vx, ty = sxy * bb + syy * a + syt * c2 + vy, tt = sxt * bb + syt * a + stt * c2 + vt,
                     tk = sxk * bb + syk * a + stk * c2 + vk;
        // m = G^T S', G = (0, 0, h, 1)
        const double mx = hc * sxt + sxk, my = hc * syt + syk, mt = hc * stt + stk, mk = hc * stk + skk;
        const double quu = 2.0 * w_k + dk + hc * mt + mk;
        const double iq = rcp(quu);
        const double ux = mx, uy = my, ut = mt - a * mx + bb * my, uk = -dk;        // Q_u,xi
        const double qu = hc * tt + tk;
        // N = T^T S3' T
        const double u1 = -a * sxx + bb * sxy + sxt, u2 = -a * sxy + bb * syy + syt, u3 = -a * sxt + bb * syt + stt;
        const double nxx = sxx, nxy = sxy, nyy = syy, nxt = u1, nyt = u2, ntt = -a * u1 + bb * u2 + u3;
        const double gx = -wd2 * Xc + tx, gy = -wd2 * Yc + ty, gt = -a * tx + bb * ty + tt;
        const double Kx = ux * iq, Ky = uy * iq, Kt = ut * iq, Kk = uk * iq, kf = qu * iq;
        double* w = ws + (size_t)i * 5 * batch + b;
        w[0] = Kx; w[batch] = Ky; w[2 * (size_t)batch] = Kt; w[3 * (size_t)batch] = Kk; w[4 * (size_t)batch] = kf;
        sxx = wd2 + nxx - ux * Kx; sxy = nxy - ux * Ky; sxt = nxt - ux * Kt; sxk = -ux * Kk;
        syy = wd2 + nyy - uy * Ky; syt = nyt - uy * Kt; syk = -uy * Kk;
        stt = ntt - ut * Kt; stk = -ut * Kk;
        skk = dk - uk * Kk;
        vx = gx - ux * kf; vy = gy - uy * kf; vt = gt - ut * kf; vk = -uk * kf;
    }
    // theta_0 minimises the value function at (x_0, y_0) = the first raw point (relative coordinates: 0, 0)
    double x = 0.0, y = 0.0, th = -vt / stt, kp = 0.0, s_acc = 0.0;
    bool finite = stt > 0.0;
    ox[row] = X0; oy[row] = Y0; os[row] = 0.0;
    { const double* g = sdb; na = g[2 * B1]; nb = g[3 * B1]; nc = g[4 * B1]; nh = g[5 * B1]; }
    double w0, w1, w2, w3, w4;
    { const double* w = ws + b; w0 = w[0]; w1 = w[B1]; w2 = w[2 * B1]; w3 = w[3 * B1]; w4 = w[4 * B1]; }
    for (int i = 0; i + 1 < nq; ++i) {
        const double a = na, bb = nb, c2 = nc, hc = nh;
        const double K0 = w0, K1 = w1, K2 = w2, K3 = w3, K4 = w4;
        if (i + 2 < nq) {
            const double* g = sdb + (size_t)(i + 1) * 6 * B1; na = g[2 * B1]; nb = g[3 * B1]; nc = g[4 * B1]; nh = g[5 * B1];
            const double* w = ws + (size_t)(i + 1) * 5 * B1 + b; w0 = w[0]; w1 = w[B1]; w2 = w[2 * B1]; w3 = w[3 * B1]; w4 = w[4 * B1];
        }
        const double u = -(K0 * x + K1 * y + K2 * th + K3 * kp + K4);
        const double xn = x - a * th + bb, yn = y + bb * th + a;
        th = th + hc * u + c2;
        kp = u;
        s_acc += sqrt((xn - x) * (xn - x) + (yn - y) * (yn - y));
        x = xn; y = yn;
        ox[row + i + 1] = X0 + x; oy[row + i + 1] = Y0 + y; os[row + i + 1] = s_acc;
        finite = finite && fabs(x) <= 1e300 && fabs(y) <= 1e300;
    }
    for (int i = nq; i < n; ++i) { ox[row + i] = X0 + x; oy[row + i] = Y0 + y; os[row + i] = s_acc; }       // (as tension_finish_kernel: the tail repeats the last point)
    status[b] = finite ? PQP_STATUS_SOLVED : PQP_STATUS_NUMERICAL;
    if (iters) iters[b] = 0;
    if (info) { double* f = info + (size_t)b * PQP_INFO_STRIDE; for (int k = 0; k < PQP_INFO_STRIDE; ++k) f[k] = 0.0; f[4] = 1.0; f[5] = 1.0; f[6] = 1.0; }
}

// ---- S2: TensionSmoother (tension_smoother.cpp:102-177).  Interleave (x, y, d)_i -> 3i + {0,1,2} -----------------------
//   rows: i: x_i - cos(phi_i + pi/2) d_i = x_list[i];  n+i: y_i - sin(phi_i + pi/2) d_i = y_list[i];  2n+i: d_i box
// n_of (or nullptr): points of each scenario, as for S1 - points i >= n_of are decoupled dummies (unit cost, zero rows with infinite
// bounds), the difference windows of the cost end at the scenario's last point, which also gets the end point's +-0.5 m box
__global__ void tension_assemble_kernel(int batch, int n, const int32_t* __restrict__ n_of, const double* __restrict__ xl, const double* __restrict__ yl,
                                        const double* __restrict__ al, const double* __restrict__ clearance, double w_k, double w_dk,
                                        double w_dev, double* __restrict__ pband, double* __restrict__ q, double* __restrict__ aval,
                                        double* __restrict__ lo, double* __restrict__ up) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * n) return;
    const int b = idx / n, i = idx - b * n;
    const int nv = 3 * n, nc = 3 * n;
    const int nq = n_of ? (n_of[b] < n ? (n_of[b] < 4 ? 4 : n_of[b]) : n) : n;
    double* pb = pband + (size_t)b * 10 * nv;
    double* qq = q + (size_t)b * nv;
    double* av = aval + (size_t)b * nc * kRMax;
    double* l = lo + (size_t)b * nc;
    double* u = up + (size_t)b * nc;
    double* r0 = av + (size_t)i * kRMax;
    double* r1 = av + (size_t)(n + i) * kRMax;
    double* r2 = av + (size_t)(2 * n + i) * kRMax;
    qq[3 * i] = 0.0; qq[3 * i + 1] = 0.0; qq[3 * i + 2] = 0.0;
    if (i >= nq) {               // a dummy point
        for (int dd = 0; dd < 10; ++dd) for (int c = 0; c < 3; ++c) pb[(size_t)dd * nv + 3 * i + c] = 0.0;
        pb[3 * i] = pb[3 * i + 1] = pb[3 * i + 2] = 1.0;
        for (int k = 0; k < 4; ++k) { r0[k] = 0.0; r1[k] = 0.0; r2[k] = 0.0; }
        l[i] = l[n + i] = l[2 * n + i] = -1e30; u[i] = u[n + i] = u[2 * n + i] = 1e30;
        return;
    }
    // Hessian (:108-124): sum of w_k [1,-2,1]^T[1,-2,1] over windows i..i+2 (i = 0..nq-3) and
    // w_dk [-1,3,-3,1]^T[-1,3,-3,1] over windows i..i+3 (i = 0..nq-4), on the x chain and on the y chain; w_dev on d
    const double v2[3] = {1.0, -2.0, 1.0}, v3[4] = {-1.0, 3.0, -3.0, 1.0};
    for (int e = 0; e <= 3; ++e) {          // entry (i + e, i) of the chain matrix
        double m = 0.0;
        if (i + e < nq) {
            for (int w = i + e - 2; w <= i; ++w)      // window start w covers w..w+2
                if (w >= 0 && w <= nq - 3 && e <= 2) m += w_k * v2[i - w] * v2[i + e - w];
            for (int w = i + e - 3; w <= i; ++w)
                if (w >= 0 && w <= nq - 4) m += w_dk * v3[i - w] * v3[i + e - w];
        }
        for (int c = 0; c < 3; ++c) {
            for (int dd = 3 * e; dd < 3 * e + 3 && dd < 10; ++dd) pb[(size_t)dd * nv + 3 * i + c] = 0.0;
        }
        pb[(size_t)(3 * e) * nv + 3 * i] = m;
        pb[(size_t)(3 * e) * nv + 3 * i + 1] = m;
    }
    pb[3 * i + 2] = w_dev;
    const double th = al[idx] + kPi2;
    r0[0] = 1.0; r0[1] = -cos(th); r0[2] = r0[3] = 0.0;
    r1[0] = 1.0; r1[1] = -sin(th); r1[2] = r1[3] = 0.0;
    r2[0] = 1.0; r2[1] = r2[2] = r2[3] = 0.0;
    l[i] = u[i] = xl[idx];
    l[n + i] = u[n + i] = yl[idx];
    double c = fmin(clearance[idx], 2.0);                                    // :163-175
    double dl = -c, du = c;
    if (i == 0) { dl = 0.0; du = 0.0; }                                      // :159-160
    if (i == nq - 1) { dl = -0.5; du = 0.5; }                                // :161-162
    l[2 * n + i] = dl; u[2 * n + i] = du;
}

// ---- S3: postSmooth (reference_path_smoother.cpp:582-636).  Interleave (l, l', l'')_i -> 3i + {0,1,2} ---------------------
//   rows: i: l_i in [lb_i, ub_i] (i = 0: pinned to the vehicle offset);  m+i: l_{i+1} - l_i - ds l'_i = 0;
//         2m-1+i: l'_{i+1} - l'_i - ds l''_i = 0
// m_of (or nullptr): layers of each scenario; layers beyond it are decoupled dummies (their rows are zero rows with infinite bounds)
__global__ void post_assemble_kernel(int batch, int m, const int32_t* __restrict__ m_of, const double* __restrict__ ls,
                                     const double* __restrict__ lb, const double* __restrict__ ub, const double* __restrict__ vehicle_l,
                                     double* __restrict__ pband, double* __restrict__ q, double* __restrict__ aval, double* __restrict__ lo,
                                     double* __restrict__ up) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * m) return;
    const int b = idx / m, i = idx - b * m;
    const int nv = 3 * m, nc = 3 * m - 2;
    const int mq = m_of ? (m_of[b] < m ? (m_of[b] < 1 ? 1 : m_of[b]) : m) : m;
    double* pb = pband + (size_t)b * nv;
    double* qq = q + (size_t)b * nv;
    double* av = aval + (size_t)b * nc * kRMax;
    double* l = lo + (size_t)b * nc;
    double* u = up + (size_t)b * nc;
    pb[3 * i] = 1.0; pb[3 * i + 1] = 100.0; pb[3 * i + 2] = 1000.0;        // :587-593
    qq[3 * i] = qq[3 * i + 1] = qq[3 * i + 2] = 0.0;
    double* r0 = av + (size_t)i * kRMax;
    if (i >= mq || i >= mq - 1) {
        // dummy layer, or the last real layer of a shortened corridor: no transition rows leave it
        if (i < m - 1) {
            double* r1 = av + (size_t)(m + i) * kRMax;
            double* r2 = av + (size_t)(2 * m - 1 + i) * kRMax;
            r1[0] = r1[1] = r1[2] = r1[3] = 0.0; r2[0] = r2[1] = r2[2] = r2[3] = 0.0;
            l[m + i] = l[2 * m - 1 + i] = -1e30; u[m + i] = u[2 * m - 1 + i] = 1e30;
        }
        if (i >= mq) { r0[0] = r0[1] = r0[2] = r0[3] = 0.0; l[i] = -1e30; u[i] = 1e30; return; }
        r0[0] = 1.0; r0[1] = r0[2] = r0[3] = 0.0;
        if (i == 0) { l[0] = u[0] = vehicle_l[b]; } else { l[i] = lb[idx]; u[i] = ub[idx]; }
        return;
    }
    r0[0] = 1.0; r0[1] = r0[2] = r0[3] = 0.0;
    if (i == 0) { l[0] = u[0] = vehicle_l[b]; }                               // :630-631
    else { l[i] = lb[idx]; u[i] = ub[idx]; }                                  // :632-635
    if (i < m - 1) {
        const double ds = ls[idx + 1] - ls[idx];
        double* r1 = av + (size_t)(m + i) * kRMax;
        double* r2 = av + (size_t)(2 * m - 1 + i) * kRMax;
        r1[0] = 1.0; r1[1] = -1.0; r1[2] = -ds; r1[3] = 0.0;                  // :610-616
        r2[0] = 1.0; r2[1] = -1.0; r2[2] = -ds; r2[3] = 0.0;                  // :618-624
        l[m + i] = u[m + i] = 0.0;
        l[2 * m - 1 + i] = u[2 * m - 1 + i] = 0.0;
    }
}

// ---- S3, exact: postSmooth's QP as a box QP in the offsets alone, one wavefront per scenario, one lane per layer ----------------------
// The two difference rows of a layer pair (reference_path_smoother.cpp:610-624) make l' and l'' functions of the offsets l:
//   l'_i = (l_{i+1} - l_i) / h_i,  l''_i = (l'_{i+1} - l'_i) / h_i   (h_i = s_{i+1} - s_i),
// the last layer's l' is only tied to the layer before it (minimised in closed form: it adds 1000 / (h^2 + 10) to the weight of l'_{m-2}) and its
// l'' appears in no row (0).  What is left is
//   minimise 1/2 sum l_i^2 + 1/2 sum W_i l'_i^2 + 500 sum l''_i^2   over lb_i <= l_i <= ub_i, l_0 = the vehicle's offset
// - same feasible set, same cost, hence the same optimum as the reference's 3m-variable QP - with a pentadiagonal SPD Hessian (condition
// ~1e3).  Solved by the primal-dual active-set iteration the polish of the generic core uses, each round one LDL^T of the pentadiagonal
// system with the active offsets pinned: the recursion runs down the lanes through v_readlane (m sequential steps of a few flops, no
// LDS, no barrier), everything else is one lane per layer (up to six layers per lane for long corridors) with shuffles.  Ends when the KKT conditions of the box QP hold to
// polish_tol (status SOLVED, iters 0), or - an inverted box - PRIMAL_INFEASIBLE.  Used for handles that ask for exact optima (polish = 1) and
// m <= 1024; the reference's ADMM setting runs the generic core on the reference's formulation.
__device__ __forceinline__ double readlane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// ---- where the exact kernels of S2 / S3 keep their per-element arrays ------------------------------------------------------------------------
// Element i of a scenario (a point, a layer) belongs to lane i mod 64, chunk k = i / 64.
// SmRegs<K>: K chunks in registers, neighbours by shuffles - up to 64 K elements, what a wavefront's register file holds (K <= 16: 1024).
// SmHbm: any count (the reference has no cap: tension_smoother.cpp:49-100, reference_path_smoother.cpp:526-580) - the arrays in a workspace
// in HBM, [array][element] per scenario: a chunk's loads and stores coalesce and stay in the CU's L1 / the XCD's L2, neighbours are read by
// address, and a phase that reads what other lanes wrote starts with sync().  The kernels below are written once over either.
template <int K>
struct SmRegs {
    static constexpr bool kHbm = false;
    typedef double Vec[K];                                // (plain arrays: wrapped in a struct the same code takes 15 % more registers)
    typedef int ActVec[K];
    int lane;
    __device__ __forceinline__ SmRegs(int lane_, double*, int) : lane(lane_) {}
    __device__ __forceinline__ int chunks() const { return K; }
    template <class A> __device__ __forceinline__ void bind(A&, int) const {}
    __device__ __forceinline__ void sync() const {}
    // element i + E (E = -3 .. 3) of an array; 0 beyond the ends.  E = +1, +2, -1, -2: one shuffle and one lane read.  (Run with every lane enabled.)
    template <int E> __device__ __forceinline__ double at(const Vec& v, int k) const {
        static_assert(E != 0 && E >= -3 && E <= 3, "neighbours up to three away");
        const int kn = k + 1 < K ? k + 1 : k, kp = k > 0 ? k - 1 : k;
        if constexpr (E == 1) { const double t = __shfl_down(v[k], 1); const double w = k + 1 < K ? readlane_f64(v[kn], 0) : 0.0; return lane == 63 ? w : t; }
        if constexpr (E == 2) { const double t = __shfl_down(v[k], 2); const double w = k + 1 < K ? __shfl(v[kn], (lane + 2) & 63) : 0.0; return lane >= 62 ? w : t; }
        if constexpr (E == -1) { const double t = __shfl_up(v[k], 1); const double w = k > 0 ? readlane_f64(v[kp], 63) : 0.0; return lane == 0 ? w : t; }
        if constexpr (E == -2) { const double t = __shfl_up(v[k], 2); const double w = k > 0 ? __shfl(v[kp], (lane + 62) & 63) : 0.0; return lane < 2 ? w : t; }
        if constexpr (E == 3 || E == -3) {
            const int src = lane + E;
            const double same = __shfl(v[k], src & 63);
            const double nxt = k + 1 < K ? __shfl(v[kn], src & 63) : 0.0;
            const double prv = k > 0 ? __shfl(v[kp], src & 63) : 0.0;
            return src > 63 ? nxt : (src < 0 ? prv : same);
        }
    }
};
struct SmHbm {
    static constexpr bool kHbm = true;
    struct Vec {
        double* p;                                        // this lane's element of chunk 0
        __device__ __forceinline__ double& operator[](int k) const { return p[64 * k]; }
    };
    typedef Vec ActVec;                                   // (every array of the workspace is one of doubles; the set holds -1, 0, 1)
    int lane, kc, npad;
    double* base;
    __device__ __forceinline__ SmHbm(int lane_, double* ws, int n) : lane(lane_), kc((n + 63) >> 6), npad(64 * ((n + 63) >> 6)), base(ws) {}
    __device__ __forceinline__ int chunks() const { return kc; }
    __device__ __forceinline__ void bind(Vec& v, int slot) const { v.p = base + (size_t)slot * npad + lane; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    template <int E> __device__ __forceinline__ double at(const Vec& v, int k) const { const int i = lane + 64 * k + E; return (i >= 0 && i < npad) ? v.p[64 * k + E] : 0.0; }
};
template <int K> struct SmStoreOf { typedef SmRegs<K> type; };
template <> struct SmStoreOf<0> { typedef SmHbm type; };
// arrays of the workspace (SmHbm): doubles per element
constexpr int kPostExactArrays = 25, kTensionExactArrays = 44;

// ---- what the exact kernels of S3 (BW = 2: pentadiagonal) and S2 (BW = 3: heptadiagonal, a linear term) share ---------------------------
// A symmetric band is held as its diagonal p, the sub-diagonals q, r, t (H[i+1][i], H[i+2][i], H[i+3][i]) and the same shifted to row i
// (q_m1 = H[i][i-1], r_m2 = H[i][i-2], t_m3 = H[i][i-3]); t and t_m3 only for BW = 3.  The sums keep the order each kernel had on its own.
// (H x + lin)_i, lin only with kLin
template <int BW, bool kLin, class St, class Vec = typename St::Vec>
__device__ __forceinline__ double band_gradient(const St& st, int k, const Vec& x, const Vec& p, const Vec& q, const Vec& r, const Vec& t, const Vec& q_m1,
                                                const Vec& r_m2, const Vec& t_m3, const Vec& lin) {
    double g = p[k] * x[k];
    if constexpr (kLin) g = lin[k] + g;
    g += q[k] * st.template at<1>(x, k);
    g += r[k] * st.template at<2>(x, k);
    if constexpr (BW == 3) g += t[k] * st.template at<3>(x, k);
    g += q_m1[k] * st.template at<-1>(x, k);
    g += r_m2[k] * st.template at<-2>(x, k);
    if constexpr (BW == 3) g += t_m3[k] * st.template at<-3>(x, k);
    return g;
}

// LDL^T of the band with diagonal pm and sub-diagonals qm, rm, tm (tm only for BW = 3), forward and back substitution: x (written, not read) =
// the solution on the first nq elements, 0 beyond.  The recursion runs down the lanes through v_readlane, a chunk at a time.  L's columns and z: slots slot .. slot + BW.
template <int BW, class St, class Vec = typename St::Vec>
__device__ __forceinline__ void band_ldl_solve(const St& st, int nq, const Vec& pm, const Vec& qm, const Vec& rm, const Vec& tm, const Vec& rhs, Vec& x,
                                               int slot) {
    static_assert(BW == 2 || BW == 3, "penta- or heptadiagonal");
    const int KC = st.chunks(), lane = st.lane;
    Vec l1, l2, l3, z;
    st.bind(l1, slot); st.bind(l2, slot + 1); st.bind(z, slot + BW);
    if constexpr (BW == 3) st.bind(l3, slot + 2);
    {
        double d1 = 0.0, d2 = 0.0, d3 = 0.0;           // d_{i-1}, d_{i-2}, d_{i-3}
        double a1 = 0.0;                               // l1_{i-1}
        double b1 = 0.0, b2 = 0.0;                     // l2_{i-1}, l2_{i-2}
        double c1 = 0.0, c2 = 0.0, c3 = 0.0;           // l3_{i-1}, l3_{i-2}, l3_{i-3}
        double y1 = 0.0, y2 = 0.0, y3 = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const double pk = pm[k], qk = qm[k], rk = rm[k], bk = rhs[k];
            double tk = 0.0;
            if constexpr (BW == 3) tk = tm[k];
            double l1k = 0.0, l2k = 0.0, l3k = 0.0, zk = 0.0;
            const int cnt = nq - 64 * k < 64 ? nq - 64 * k : 64;
            for (int l = 0; l < cnt; ++l) {
                const double pi = readlane_f64(pk, l), qi = readlane_f64(qk, l), ri = readlane_f64(rk, l), bi = readlane_f64(bk, l);
                double di = pi - a1 * a1 * d1 - b2 * b2 * d2, l1n = qi - b1 * a1 * d1, l2n = ri, yi = bi - a1 * y1 - b2 * y2, ti = 0.0;
                if constexpr (BW == 3) { ti = readlane_f64(tk, l); di -= c3 * c3 * d3; l1n -= c2 * b2 * d2; l2n -= c1 * a1 * d1; yi -= c3 * y3; }
                const double inv = rcp(di);
                const double l1i = l1n * inv, l2i = l2n * inv, l3i = ti * inv;
                // (selects, not a branch around four moves: two scalar branches per step cost more than eight v_cndmask - +6 % at 80 points, +23 % at 200)
                { const bool me = lane == l; l1k = me ? l1i : l1k; l2k = me ? l2i : l2k; l3k = me ? l3i : l3k; zk = me ? yi * inv : zk; }
                d3 = d2; d2 = d1; d1 = di;
                a1 = l1i;
                b2 = b1; b1 = l2i;
                c3 = c2; c2 = c1; c1 = l3i;
                y3 = y2; y2 = y1; y1 = yi;
            }
            l1[k] = l1k; l2[k] = l2k; z[k] = zk;
            if constexpr (BW == 3) l3[k] = l3k;
        }
    }
    {
        double x1 = 0.0, x2 = 0.0, x3 = 0.0;
#pragma unroll
        for (int k = KC - 1; k >= 0; --k) {
            const double zk = z[k], l1k = l1[k], l2k = l2[k];
            double l3k = 0.0;
            if constexpr (BW == 3) l3k = l3[k];
            double xk = 0.0;
            const int cnt = nq - 64 * k < 64 ? nq - 64 * k : 64;
            for (int l = cnt - 1; l >= 0; --l) {
                double xi = readlane_f64(zk, l) - readlane_f64(l1k, l) * x1 - readlane_f64(l2k, l) * x2;
                if constexpr (BW == 3) xi -= readlane_f64(l3k, l) * x3;
                xk = lane == l ? xi : xk;
                x3 = x2; x2 = x1; x1 = xi;
            }
            x[k] = lane + 64 * k < nq ? xk : 0.0;
        }
    }
}

// workspace slots (SmHbm) of the arrays the rounds use; tm only for BW = 3, the LDL^T's BW + 1 from ldl on
struct SmRoundSlots { int fix, frd, rhs, pm, qm, rm, tm, ldl, viol; };
struct SmRounds { bool ok, nonfinite; int factors; };

// Primal-dual active-set rounds of the box QP  minimise 1/2 x^T H x (+ lin^T x)  over lo <= x <= up  from the set act (-1 at lo, 1 at up,
// 0 free), x the first guess on entry and the last solve on exit.  Each round: one LDL^T with the active elements REMOVED from the system (their
// values pinned, their coupling moved to the right-hand side), then the KKT test of the box QP - free elements inside their box, active ones
// pushed against it - to tol relative to 1 + |x|_inf.  Every element that violates it changes sides; once the largest violation has not
// shrunk by 30 % in three rounds (or from the start: conservative) only those within loose(round) of the largest move.
template <int BW, bool kLin, class St, class Loose, class Vec = typename St::Vec, class ActVec = typename St::ActVec>
__device__ __forceinline__ SmRounds band_active_set_rounds(const St& st, int nq, const Vec& p, const Vec& q, const Vec& r, const Vec& t, const Vec& q_m1,
                                                           const Vec& r_m2, const Vec& t_m3, const Vec& lin, const Vec& lo, const Vec& up, ActVec& act,
                                                           Vec& x, double tol, int max_rounds, bool conservative, Loose loose, SmRoundSlots sl) {
    const int KC = st.chunks(), lane = st.lane;
    auto real = [&](int k) { return lane + 64 * k < nq; };
    auto pinned = [&](int k) { return real(k) && lo[k] == up[k]; };
    SmRounds res{false, false, 0};
    bool nonfinite = false;
    int stall = 0;
    double best = 1e300;
    for (int round = 0; round < max_rounds; ++round) {
        Vec fix, frd, rhs, pm, qm, rm, tm;
        st.bind(fix, sl.fix); st.bind(frd, sl.frd); st.bind(rhs, sl.rhs); st.bind(pm, sl.pm); st.bind(qm, sl.qm); st.bind(rm, sl.rm);
        if constexpr (BW == 3) st.bind(tm, sl.tm);
#pragma unroll
        for (int k = 0; k < KC; ++k) { fix[k] = act[k] < 0 ? lo[k] : (act[k] > 0 ? up[k] : 0.0); frd[k] = act[k] == 0 ? 1.0 : 0.0; }
        st.sync();
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const bool fr = act[k] == 0;
            // (the shuffles run with every lane enabled, none behind a condition: a disabled lane's value is not readable)
            const bool f1 = st.template at<1>(frd, k) != 0.0, f2 = st.template at<2>(frd, k) != 0.0, f3 = BW == 3 && st.template at<3>(frd, k) != 0.0;
            double s = q[k] * st.template at<1>(fix, k) + r[k] * st.template at<2>(fix, k);
            if constexpr (BW == 3) s += t[k] * st.template at<3>(fix, k);
            s += q_m1[k] * st.template at<-1>(fix, k);
            s += r_m2[k] * st.template at<-2>(fix, k);
            if constexpr (BW == 3) s += t_m3[k] * st.template at<-3>(fix, k);
            double coupled = -s;
            if constexpr (kLin) coupled = -lin[k] - s;
            rhs[k] = fr ? coupled : fix[k];
            pm[k] = fr ? p[k] : 1.0; qm[k] = (fr && f1) ? q[k] : 0.0; rm[k] = (fr && f2) ? r[k] : 0.0;
            if constexpr (BW == 3) tm[k] = (fr && f3) ? t[k] : 0.0;
        }
        band_ldl_solve<BW>(st, nq, pm, qm, rm, tm, rhs, x, sl.ldl);
        res.factors += 1;
        st.sync();
        Vec viol;
        st.bind(viol, sl.viol);
        double vloc = 0.0, sloc = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const double xk = x[k];
            const double g = band_gradient<BW, kLin>(st, k, x, p, q, r, t, q_m1, r_m2, t_m3, lin);
            double v = 0.0;
            if (real(k) && !pinned(k)) {
                if (act[k] == 0) v = fmax(fmax(lo[k] - xk, xk - up[k]), 0.0);
                else v = act[k] < 0 ? fmax(-g, 0.0) : fmax(g, 0.0);
            }
            if (real(k) && !(fabs(xk) <= 1e300 && fabs(g) <= 1e300)) nonfinite = true;
            viol[k] = v; vloc = fmax(vloc, v); sloc = fmax(sloc, real(k) ? fabs(xk) : 0.0);       // (S3: H's smallest eigenvalue is >= 1, a gradient that is off by tol moves the optimum by <= tol)
        }
        if (__ballot(nonfinite) != 0ull) { res.nonfinite = true; break; }
        const double vmax = wave_max(vloc), scale = 1.0 + wave_max(sloc);
        if (vmax <= tol * scale) { res.ok = true; break; }
        // (when the violation stops shrinking only the worst offenders move, as in the generic core's polish)
        if (vmax < 0.7 * best) { best = vmax; stall = 0; } else { stall += 1; }
        if (stall >= 3) conservative = true;
        const double thr = conservative ? fmax(tol * scale, loose(round) * vmax) : tol * scale;
#pragma unroll
        for (int k = 0; k < KC; ++k)
            if (real(k) && !pinned(k) && viol[k] >= thr && viol[k] > 0.0) {
                if (act[k] == 0) act[k] = (lo[k] - x[k] > x[k] - up[k]) ? -1 : 1;
                else act[k] = 0;
            }
    }
    return res;
}

// lane 0: a scenario's status, iters (0) and info (f[3] = interior-point iterations, f[5] = f[6] = factorisations)
__device__ __forceinline__ void sm_exact_report(int b, bool ok, bool nonfinite, int factors, int ipm_its, int32_t* status, int32_t* iters, double* info) {
    if (threadIdx.x != 0) return;
    status[b] = ok ? PQP_STATUS_SOLVED : (nonfinite ? PQP_STATUS_NUMERICAL : PQP_STATUS_MAX_ITER);
    if (iters) iters[b] = 0;
    if (info) { double* f = info + (size_t)b * PQP_INFO_STRIDE; for (int k = 0; k < PQP_INFO_STRIDE; ++k) f[k] = 0.0; f[3] = (double)ipm_its; f[4] = ok ? 1.0 : 0.0; f[5] = (double)factors; f[6] = (double)factors; }
}

// K: layers per lane (m <= 64 K; the host picks the smallest of 1, 2, 4, 6, 8, 12, 16: up to 1024 layers; 16: 19 spilled registers), or 0: any m,
// the arrays in the workspace `ws` (kPostExactArrays * 64 ceil(m / 64) doubles per scenario).
template <int K>
__global__ void __launch_bounds__(64) post_exact_kernel(int batch, int m, const int32_t* __restrict__ m_of, const double* __restrict__ ls,
                                                        const double* __restrict__ lb, const double* __restrict__ ub,
                                                        const double* __restrict__ vehicle_l, double tol, double* __restrict__ out_l,
                                                        int32_t* __restrict__ status, int32_t* __restrict__ iters, double* __restrict__ info,
                                                        signed char* __restrict__ act_io, int carry, double* ws) {
    typedef typename SmStoreOf<K>::type St;
    typedef typename St::Vec Vec;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= batch) return;
    int mq = m_of ? m_of[b] : m;
    mq = mq < 1 ? 1 : (mq > m ? m : mq);
    mq = __builtin_amdgcn_readfirstlane(mq);
    const size_t row = (size_t)b * m;
    const St st(lane, St::kHbm ? ws + (size_t)b * kPostExactArrays * (64 * ((m + 63) >> 6)) : nullptr, m);
    const int KC = St::kHbm ? st.chunks() : K;
    auto real = [&](int k) { return lane + 64 * k < mq; };
    // ---- the Hessian's three diagonals: p_i = H[i][i], q_i = H[i+1][i], r_i = H[i+2][i] -------------------------------------------------
    Vec sv, ih, wb, al, be, ga, p, q, r, lo, up, a, q_p1, r_p2;
    st.bind(sv, 0); st.bind(ih, 1); st.bind(wb, 2); st.bind(al, 3); st.bind(be, 4); st.bind(ga, 5); st.bind(p, 6); st.bind(q, 7); st.bind(r, 8); st.bind(lo, 9); st.bind(up, 10); st.bind(a, 11); st.bind(q_p1, 12); st.bind(r_p2, 13);
    typename St::ActVec act;
    st.bind(act, 14);
#pragma unroll
    for (int k = 0; k < KC; ++k) sv[k] = real(k) ? ls[row + lane + 64 * k] : 0.0;
    bool bad_s = false, bad_box = false;
    st.sync();
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int i = lane + 64 * k;
        const double s_next = st.template at<1>(sv, k);
        const bool has_b = i + 1 < mq;                   // l'_i exists for i <= mq - 2
        const double h = s_next - sv[k];
        bad_s = bad_s || (has_b && !(h > 0.0));
        const double ihk = has_b ? 1.0 / h : 0.0;
        ih[k] = ihk;
        double W = has_b ? 100.0 : 0.0;
        if (i + 2 == mq) W += 1000.0 / (h * h + 10.0);
        wb[k] = W * ihk * ihk;
    }
    if (__ballot(bad_s) != 0ull) {                       // abscissae that do not increase: the difference rows are singular
        for (int i = lane; i < m; i += 64) out_l[row + i] = 0.0;
        if (lane == 0) { status[b] = PQP_STATUS_NUMERICAL; if (iters) iters[b] = 0; }
        return;
    }
    st.sync();
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int i = lane + 64 * k;
        const bool has_c = i + 2 < mq;                   // l''_i for i <= mq - 3
        const double ih_next = st.template at<1>(ih, k), ihk = ih[k];
        al[k] = has_c ? ihk * ihk : 0.0; be[k] = has_c ? -(ih_next + ihk) * ihk : 0.0; ga[k] = has_c ? ih_next * ihk : 0.0;   // l''_i = al l_i + be l_{i+1} + ga l_{i+2}
    }
    st.sync();
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int i = lane + 64 * k;
        const double wb_p = st.template at<-1>(wb, k), be_p = st.template at<-1>(be, k), ga_p = st.template at<-1>(ga, k), ga_pp = st.template at<-2>(ga, k);
        const double alk = al[k];
        p[k] = 1.0 + wb_p + wb[k] + 1000.0 * (ga_pp * ga_pp + be_p * be_p + alk * alk);
        q[k] = -wb[k] + 1000.0 * (be_p * ga_p + alk * be[k]);
        r[k] = 1000.0 * alk * ga[k];
        double lok = -1e30, upk = 1e30;
        if (real(k)) { lok = i == 0 ? vehicle_l[b] : lb[row + i]; upk = i == 0 ? vehicle_l[b] : ub[row + i]; }
        lo[k] = lok; up[k] = upk;
        const bool pin = real(k) && lok == upk;
        bad_box = bad_box || (real(k) && lok > upk);
        // the first active set: OSQP's rule at the cold start (z = 0, y = 0) = the boxes that exclude 0
        int a0 = pin ? -1 : (lok > 0.0 ? -1 : (upk < 0.0 ? 1 : 0));
        // PQP_OPT_CARRY_CYCLES: the set this scenario's slot ended with in the handle's previous solve of the shape (the same corridor one planning
        // cycle earlier) - the rounds below then only have to confirm or repair it
        if (carry && real(k) && !pin) { const int v = act_io[row + i]; a0 = v < 0 ? -1 : (v > 0 ? 1 : 0); }
        act[k] = a0;
        a[k] = 0.0;
    }
    st.sync();
#pragma unroll
    for (int k = 0; k < KC; ++k) { q_p1[k] = st.template at<-1>(q, k); r_p2[k] = st.template at<-2>(r, k); }
    if (__ballot(bad_box) != 0ull) {                     // an inverted box: the rows l_i >= lb_i, l_i <= ub_i have no common point
        for (int i = lane; i < m; i += 64) out_l[row + i] = 0.0;
        if (lane == 0) { status[b] = PQP_STATUS_PRIMAL_INFEASIBLE; if (iters) iters[b] = 0; }
        return;
    }
    // (no linear term, no t: the dummies p, q are not read)
    const SmRounds rs = band_active_set_rounds<2, false>(st, mq, p, q, r, q, q_p1, r_p2, q_p1, p, lo, up, act, a, tol, 4 * mq + 24, false,
                                                         [](int) { return 0.9; }, SmRoundSlots{15, 16, 17, 18, 19, 20, -1, 21, 24});
    const bool ok = rs.ok, nonfinite = rs.nonfinite;
#pragma unroll
    for (int k = 0; k < KC; ++k) if (lane + 64 * k < m) out_l[row + lane + 64 * k] = (real(k) && !nonfinite) ? a[k] : 0.0;
    if (act_io && ok) {
#pragma unroll
        for (int k = 0; k < KC; ++k) if (real(k)) act_io[row + lane + 64 * k] = (signed char)act[k];
    }
    sm_exact_report(b, ok, nonfinite, rs.factors, 0, status, iters, info);
}

// ---- S2, exact: TensionSmoother's QP as a box QP in the lateral shifts alone, one wavefront per scenario --------------------------------
// The rows x_i - c_i d_i = X_i, y_i - s_i d_i = Y_i (c, s = cos, sin of phi + pi/2; X, Y = the raw points; tension_smoother.cpp:146-158) make x and
// y functions of d, which leaves  minimise 1/2 d^T (C H C + S H S + w_dev I) d + (C H X + S H Y)^T d  over the boxes on d,  H = the chain matrix
// of the second- and third-difference windows (:108-124), C = diag(c), S = diag(s): a heptadiagonal Hessian.  Same scheme as post_exact_kernel
// - primal-dual active-set rounds, each one LDL^T with the active shifts REMOVED from the system (not penalised: the Hessian's condition is
// ~1e8 and leaves no room for a penalty), the recursion down the lanes through v_readlane, the KKT test of the box QP - with three
// sub-diagonals and a linear term.  The generic core's 9 x 9-block formulation needs ~15 rounds of 20 barrier phases per level and holds 166
// points in a CU's LDS; this one holds 512 in registers (eight per lane; 96 of them spilled at that size), up to 1024 with twelve / sixteen per lane and
// 1.8 / 3.3 KB of scratch per lane, and any count with the arrays in HBM (K = 0: `ws`, kTensionExactArrays * 64 ceil(n / 64) doubles per scenario).
// Used for handles that ask for exact optima (polish = 1) and wherever the generic core cannot hold the QP.
__device__ __forceinline__ double tension_chain_entry(int j, int e, int nq, double w_k, double w_dk) {      // H[j + e][j], 0 <= e <= 3
    const double v2[3] = {1.0, -2.0, 1.0}, v3[4] = {-1.0, 3.0, -3.0, 1.0};
    double m = 0.0;
    if (j < 0 || j + e >= nq) return 0.0;
    for (int w = j + e - 2; w <= j; ++w)      // window start w covers w..w+2
        if (w >= 0 && w <= nq - 3 && e <= 2) m += w_k * v2[j - w] * v2[j + e - w];
    for (int w = j + e - 3; w <= j; ++w)
        if (w >= 0 && w <= nq - 4) m += w_dk * v3[j - w] * v3[j + e - w];
    return m;
}
template <int K>
__global__ void __launch_bounds__(64) tension_exact_kernel(int batch, int n, const int32_t* __restrict__ n_of, const double* __restrict__ xl,
                                                           const double* __restrict__ yl, const double* __restrict__ al, const double* __restrict__ clearance,
                                                           double w_k, double w_dk, double w_dev, double tol, double* __restrict__ ox, double* __restrict__ oy,
                                                           double* __restrict__ os, int32_t* __restrict__ status, int32_t* __restrict__ iters,
                                                           double* __restrict__ info, signed char* __restrict__ act_io, int carry, double* ws) {
    typedef typename SmStoreOf<K>::type St;
    typedef typename St::Vec Vec;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= batch) return;
    int nq = n_of ? n_of[b] : n;
    nq = nq < 4 ? 4 : (nq > n ? n : nq);
    nq = __builtin_amdgcn_readfirstlane(nq);
    const size_t row = (size_t)b * n;
    const St st(lane, St::kHbm ? ws + (size_t)b * kTensionExactArrays * (64 * ((n + 63) >> 6)) : nullptr, n);
    const int KC = St::kHbm ? st.chunks() : K;
    auto real = [&](int k) { return lane + 64 * k < nq; };
    Vec X, Y, cs, sn, h0, h1, h2, h3, p, q, r, t, lin, lo, up, d;
    st.bind(X, 0); st.bind(Y, 1); st.bind(cs, 2); st.bind(sn, 3); st.bind(h0, 4); st.bind(h1, 5); st.bind(h2, 6); st.bind(h3, 7); st.bind(p, 8); st.bind(q, 9); st.bind(r, 10); st.bind(t, 11); st.bind(lin, 12); st.bind(lo, 13); st.bind(up, 14); st.bind(d, 15);
    typename St::ActVec act;
    st.bind(act, 16);
    auto pinned = [&](int k) { return real(k) && lo[k] == up[k]; };
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int i = lane + 64 * k;
        X[k] = real(k) ? xl[row + i] : 0.0; Y[k] = real(k) ? yl[row + i] : 0.0;
        double sv = 0.0, cv = 1.0;
        if (real(k)) sincos(al[row + i] + kPi2, &sv, &cv);
        cs[k] = cv; sn[k] = sv;
        h0[k] = tension_chain_entry(i, 0, nq, w_k, w_dk); h1[k] = tension_chain_entry(i, 1, nq, w_k, w_dk);
        h2[k] = tension_chain_entry(i, 2, nq, w_k, w_dk); h3[k] = tension_chain_entry(i, 3, nq, w_k, w_dk);
        double c = real(k) ? fmin(clearance[row + i], 2.0) : 0.0;                 // tension_smoother.cpp:163-175
        lo[k] = -c; up[k] = c;
        if (i == 0) { lo[k] = 0.0; up[k] = 0.0; }                                 // :159-160
        if (i == nq - 1) { lo[k] = -0.5; up[k] = 0.5; }                           // :161-162
        if (!real(k)) { lo[k] = -1e30; up[k] = 1e30; }
        act[k] = pinned(k) ? -1 : (lo[k] > 0.0 ? -1 : (up[k] < 0.0 ? 1 : 0));
        // PQP_OPT_CARRY_CYCLES: the set this line's slot ended with in the handle's previous solve of the shape (the same line one planning cycle
        // earlier): from the cold start the rounds need 16-31 factorisations for ~15 active boxes, from the previous cycle's set 2-3
        if (carry && real(k) && !pinned(k)) { const int v = act_io[row + i]; act[k] = v < 0 ? -1 : (v > 0 ? 1 : 0); }
        d[k] = 0.0;
    }
    st.sync();
    bool bad_box = false;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        bad_box = bad_box || (real(k) && lo[k] > up[k]);
        const double c1 = st.template at<1>(cs, k), s1 = st.template at<1>(sn, k), c2 = st.template at<2>(cs, k), s2 = st.template at<2>(sn, k), c3 = st.template at<3>(cs, k), s3 = st.template at<3>(sn, k);
        p[k] = real(k) ? h0[k] + w_dev : 1.0;
        q[k] = h1[k] * (c1 * cs[k] + s1 * sn[k]);
        r[k] = h2[k] * (c2 * cs[k] + s2 * sn[k]);
        t[k] = h3[k] * (c3 * cs[k] + s3 * sn[k]);
        // gradient: c_i (H X)_i + s_i (H Y)_i; the rows of H annihilate constants, so the coordinates enter relative to point i
        double hx = 0.0, hy = 0.0;
        hx += h1[k] * (st.template at<1>(X, k) - X[k]) + h2[k] * (st.template at<2>(X, k) - X[k]) + h3[k] * (st.template at<3>(X, k) - X[k]);
        hy += h1[k] * (st.template at<1>(Y, k) - Y[k]) + h2[k] * (st.template at<2>(Y, k) - Y[k]) + h3[k] * (st.template at<3>(Y, k) - Y[k]);
        hx += st.template at<-1>(h1, k) * (st.template at<-1>(X, k) - X[k]) + st.template at<-2>(h2, k) * (st.template at<-2>(X, k) - X[k]) + st.template at<-3>(h3, k) * (st.template at<-3>(X, k) - X[k]);
        hy += st.template at<-1>(h1, k) * (st.template at<-1>(Y, k) - Y[k]) + st.template at<-2>(h2, k) * (st.template at<-2>(Y, k) - Y[k]) + st.template at<-3>(h3, k) * (st.template at<-3>(Y, k) - Y[k]);
        lin[k] = real(k) ? cs[k] * hx + sn[k] * hy : 0.0;
    }
    if (__ballot(bad_box) != 0ull) {                     // a negative clearance: the box on d is empty
        for (int i = lane; i < n; i += 64) { ox[row + i] = 0.0; oy[row + i] = 0.0; os[row + i] = 0.0; }
        if (lane == 0) { status[b] = PQP_STATUS_PRIMAL_INFEASIBLE; if (iters) iters[b] = 0; }
        return;
    }
    Vec q_m1, r_m2, t_m3;
    st.bind(q_m1, 17); st.bind(r_m2, 18); st.bind(t_m3, 19);
    st.sync();
#pragma unroll
    for (int k = 0; k < KC; ++k) { q_m1[k] = st.template at<-1>(q, k); r_m2[k] = st.template at<-2>(r, k); t_m3[k] = st.template at<-3>(t, k); }
    auto gradient = [&](int k) { return band_gradient<3, true>(st, k, d, p, q, r, t, q_m1, r_m2, t_m3, lin); };
    auto narrow = [&](int k) { return real(k) && !pinned(k) && up[k] - lo[k] < 1e-3; };
    int factors = 0, ipm_its = 0;
    // ---- the first active set, from the cold start: primal-dual interior-point iterations on the box QP ----------------------------------------
    // (round 2 started the active-set rounds from OSQP's cold-start rule - the boxes that exclude 0 - and needed 16 / 21 / 31 rounds on average at
    //  48 / 80 / 200 points, 39 / 67 / 52 on the slowest line of a batch of 1024, which is what a launch lasts.  The path to the optimum through the
    //  interior takes 10-12 iterations at every size - each the same LDL^T with the barrier's diagonal added, no row ever leaves the system - and
    //  ends so close to the optimum that the split "multiplier > slack" IS the optimal set on 9 lines in 10 and one or two boxes off on the rest:
    //  1-3 rounds of the exact iteration below confirm it.  Constants found with tools/active_set_sweep.py: centring 0.2 for two iterations then
    //  0.05, 0.995 of the way to the boundary, complementarity from 0.01 (more on rough lines) down to 1e-8 - at 1e-6 one line in 50 still needs 15-30 rounds.
    //  gam = the cost's scale relative to the reference's weights, so that the constants do not depend on the units of the weights.)
    // PQP_OPT_CARRY_CYCLES: attempt 0 = the rounds from the carried set, three of them at most (9 lines in 10 need one or two; the rest would take up to
    // 30 and a launch lasts as long as its slowest line); attempt 1 = the interior start, which is also the cold start.
    bool ok = false, nonfinite = false;
    for (int attempt = carry ? 0 : 1; attempt < 2 && !ok && !nonfinite; ++attempt) {
        if (attempt == 1) {
            const double gam = (6.0 * w_k + 20.0 * w_dk + w_dev) * (1.0 / 1006.0);
            Vec tl, tu, zl, zu, fre;
            st.bind(tl, 24); st.bind(tu, 25); st.bind(zl, 26); st.bind(zu, 27); st.bind(fre, 28);
            double cnt_loc = 0.0, tsum = 0.0, g0 = 0.0;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const double w = up[k] - lo[k];
                // boxes narrower than a millimetre stay at their centre (a barrier in them would stop every other shift's step) and are set by the gradient's sign
                const bool f = real(k) && !pinned(k) && !narrow(k);
                fre[k] = f ? 1.0 : 0.0; cnt_loc += fre[k];
                d[k] = real(k) ? (f ? fmin(fmax(0.0, lo[k] + 0.1 * w), up[k] - 0.1 * w) : 0.5 * (lo[k] + up[k])) : 0.0;
                tl[k] = f ? d[k] - lo[k] : 1.0; tu[k] = f ? up[k] - d[k] : 1.0;
                tsum += f ? fmin(tl[k], tu[k]) : 0.0;
            }
            st.sync();
#pragma unroll
            for (int k = 0; k < KC; ++k) { const double gk = gradient(k); g0 = fmax(g0, fre[k] != 0.0 ? fabs(gk) : 0.0); }       // (the shuffles inside run with every lane enabled)
            const double nfree = wave_sum(cnt_loc);
            // the first complementarity: 0.01 for lines like the reference's own (gradients of a few hundred at shifts of half a metre), more where the raw line is rough
            const double mu0 = fmax(0.01 * gam, nfree > 0.0 ? 3e-4 * wave_max(g0) * (wave_sum(tsum) / nfree) : 0.0);
#pragma unroll
            for (int k = 0; k < KC; ++k) { zl[k] = fre[k] != 0.0 ? mu0 * rcp(tl[k]) : 0.0; zu[k] = fre[k] != 0.0 ? mu0 * rcp(tu[k]) : 0.0; }
            for (int it = 0; nfree > 0.0 && it < 40; ++it) {
                Vec g;
                st.bind(g, 29);
                double cloc = 0.0, rloc = 0.0, gloc = 0.0;
                st.sync();
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const double gk = gradient(k);
                    g[k] = gk;
                    if (fre[k] != 0.0) { cloc += tl[k] * zl[k] + tu[k] * zu[k]; rloc = fmax(rloc, fabs(gk - zl[k] + zu[k])); }
                    if (real(k)) gloc = fmax(gloc, fabs(gk));
                }
                const double mu = wave_sum(cloc) / (2.0 * nfree), rmax = wave_max(rloc), gmax = wave_max(gloc);
                if (!(gmax <= 1e300)) break;
                if (mu < 1e-8 * gam && rmax < 1e-6 * (gam + gmax)) break;
                const double smu = (it < 2 ? 0.2 : 0.05) * mu;
                Vec itl, itu, pm, qm, rm, tm, rhs, dd;
                st.bind(itl, 30); st.bind(itu, 31); st.bind(pm, 32); st.bind(qm, 33); st.bind(rm, 34); st.bind(tm, 35); st.bind(rhs, 36); st.bind(dd, 37);
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const bool f = fre[k] != 0.0;
                    const bool f1 = st.template at<1>(fre, k) != 0.0, f2 = st.template at<2>(fre, k) != 0.0, f3 = st.template at<3>(fre, k) != 0.0;
                    const double il = rcp(tl[k]), iu = rcp(tu[k]);
                    itl[k] = il; itu[k] = iu;
                    pm[k] = f ? p[k] + zl[k] * il + zu[k] * iu : 1.0;
                    qm[k] = (f && f1) ? q[k] : 0.0; rm[k] = (f && f2) ? r[k] : 0.0; tm[k] = (f && f3) ? t[k] : 0.0;
                    rhs[k] = f ? -g[k] + smu * (il - iu) : 0.0;
                }
                band_ldl_solve<3>(st, nq, pm, qm, rm, tm, rhs, dd, 20);
                factors += 1; ipm_its += 1;
                Vec dzl, dzu;
                st.bind(dzl, 38); st.bind(dzu, 39);
                double aloc = 1e300;
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    if (fre[k] == 0.0) { dd[k] = 0.0; dzl[k] = 0.0; dzu[k] = 0.0; continue; }
                    const double ddk = dd[k];
                    const double dl = (smu - tl[k] * zl[k] - zl[k] * ddk) * itl[k];
                    const double du = (smu - tu[k] * zu[k] + zu[k] * ddk) * itu[k];
                    dzl[k] = dl; dzu[k] = du;
                    if (ddk < 0.0) aloc = fmin(aloc, -tl[k] / ddk);
                    if (ddk > 0.0) aloc = fmin(aloc, tu[k] / ddk);
                    if (dl < 0.0) aloc = fmin(aloc, -zl[k] / dl);
                    if (du < 0.0) aloc = fmin(aloc, -zu[k] / du);
                    if (!(fabs(ddk) <= 1e300)) aloc = -1.0;
                }
                const double amin = -wave_max(-aloc);
                if (!(amin > 0.0)) break;                       // a breakdown of the factorisation: the rounds below start from what there is
                const double alpha = fmin(1.0, 0.995 * amin);
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    if (fre[k] == 0.0) continue;
                    const double ddk = dd[k];
                    d[k] += alpha * ddk; tl[k] += alpha * ddk; tu[k] -= alpha * ddk;
                    zl[k] += alpha * dzl[k]; zu[k] += alpha * dzu[k];
                }
            }
            st.sync();
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const double gk = gradient(k);
                if (fre[k] != 0.0) act[k] = zl[k] > gam * tl[k] ? -1 : (zu[k] > gam * tu[k] ? 1 : 0);
                if (narrow(k)) act[k] = gk > 0.0 ? -1 : 1;
            }
        }
        // (after the interior start the set is a box or two off: moving only the worst offenders from the first round on ends in at most 4 rounds
        //  where the full moves the cold-start rule needs wander for 10-20 on one line in 3 500 - tools/active_set_sweep.py, tools/tension_fuzz.py)
        // (half of the largest violation, not the generic core's 0.9: the first solve - no box active, a Hessian of condition 1e8 - activates about four times the boxes
        //  the optimum holds, and releasing them one at a time took 20 / 28 / 55 rounds at 48 / 80 / 200 points where this takes 16 / 21 / 32; 0.25 cycles on 1 line in 100)
        // (1 line in 1000 cycles with 0.5 - tools/active_set_sweep.py -; from round 40 + n / 4 on, far beyond what a converging line needs, single moves end it)
        // (slots 32-36: the interior start's pm, qm, rm, tm, rhs, dead by now)
        const SmRounds rs = band_active_set_rounds<3, true>(st, nq, p, q, r, t, q_m1, r_m2, t_m3, lin, lo, up, act, d, tol, attempt == 0 ? 3 : 6 * nq + 40,
                                                            attempt == 1, [&](int round) { return (attempt == 1 || round >= 40 + nq / 4) ? 0.9 : 0.5; },
                                                            SmRoundSlots{40, 41, 36, 32, 33, 34, 35, 20, 42});
        ok = rs.ok; nonfinite = rs.nonfinite; factors += rs.factors;
    }
    // ---- x = X + c d, y = Y + s d, the chord lengths in the reference's order (tension_smoother.cpp:85-98); the tail repeats the last point
    Vec gx, gy, seg, sc;
    st.bind(gx, 32); st.bind(gy, 33); st.bind(seg, 34); st.bind(sc, 35);
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const double dd = (ok && real(k)) ? d[k] : 0.0;
        gx[k] = X[k] + cs[k] * dd; gy[k] = Y[k] + sn[k] * dd;
    }
    st.sync();
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const double px = st.template at<-1>(gx, k), py = st.template at<-1>(gy, k), cx = gx[k], cy = gy[k];
        const int i = lane + 64 * k;
        seg[k] = (i >= 1 && i < nq) ? sqrt((cx - px) * (cx - px) + (cy - py) * (cy - py)) : 0.0;
    }
    double acc = 0.0, lx = 0.0, ly = 0.0;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const double sk = seg[k], gxk = gx[k], gyk = gy[k];
        double sck = 0.0;
        const int cnt = nq - 64 * k < 64 ? nq - 64 * k : 64;
        for (int l = 0; l < cnt; ++l) {
            acc += readlane_f64(sk, l);
            if (lane == l) sck = acc;
            if (64 * k + l == nq - 1) { lx = readlane_f64(gxk, l); ly = readlane_f64(gyk, l); }
        }
        sc[k] = sck;
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int i = lane + 64 * k;
        if (i < n) { ox[row + i] = i < nq ? gx[k] : lx; oy[row + i] = i < nq ? gy[k] : ly; os[row + i] = i < nq ? sc[k] : acc; }
        if (act_io && ok && real(k)) act_io[row + i] = (signed char)act[k];
    }
    sm_exact_report(b, ok, nonfinite, factors, ipm_its, status, iters, info);
}

// result lists of the tension smoothers: x, y of the solution and the cumulative chord length
// (tension_smoother_2.cpp:57-70, tension_smoother.cpp:85-98); `stride` = variables per point (4 or 3)
// (n_of or nullptr: points of each scenario; the entries beyond them repeat the last point)
// One wavefront per scenario: the lanes copy the points and take the segment lengths (the square roots) in parallel, lane 0 adds them up
// in the reference's order (s_i = s_{i-1} + d_i), the lanes write the result.  (One LANE per scenario - 8 wavefronts for a batch of
// 512 - took 110 us at n = 200.)
__global__ void __launch_bounds__(64) tension_finish_kernel(int batch, int n, const int32_t* __restrict__ n_of, int nv, int stride,
                                                            const double* __restrict__ x, double* __restrict__ ox, double* __restrict__ oy,
                                                            double* __restrict__ os) {
    extern __shared__ __attribute__((aligned(16))) double fin_lds[];      // [n] segment lengths, then cumulative
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= batch) return;
    const double* xq = x + (size_t)b * nv;
    const int nq = n_of ? (n_of[b] < n ? (n_of[b] < 2 ? 2 : n_of[b]) : n) : n;
    for (int i = lane; i < n; i += 64) {
        const int j = i < nq ? i : nq - 1, jp = i == 0 ? 0 : (i - 1 < nq ? i - 1 : nq - 1);
        const double cx = xq[stride * j], cy = xq[stride * j + 1], px = xq[stride * jp], py = xq[stride * jp + 1];
        ox[(size_t)b * n + i] = cx; oy[(size_t)b * n + i] = cy;
        fin_lds[i] = i == 0 ? 0.0 : sqrt((cx - px) * (cx - px) + (cy - py) * (cy - py));
    }
    __syncthreads();
    if (lane == 0) {
        double s = 0.0;
        for (int i = 1; i < n; ++i) { s += fin_lds[i]; fin_lds[i] = s; }
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) os[(size_t)b * n + i] = fin_lds[i];
}
__global__ void post_finish_kernel(int batch, int m, const double* __restrict__ x, double* __restrict__ ol) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * m) return;
    const int b = idx / m, i = idx - b * m;
    ol[idx] = x[(size_t)b * 3 * m + 3 * i];
}

}  // namespace pqp
