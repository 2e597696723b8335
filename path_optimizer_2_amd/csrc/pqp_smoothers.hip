// pqp_smoothers.hip — the reference-line smoothing QPs of include/pqp.h: TensionSmoother2, TensionSmoother and
// the postSmooth QP.  Their kernels (pqp_smoother_kernels.inc, the generic banded core of pqp_banded_qp.hpp), launchers and entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "pqp_defaults.hpp"
#include "pqp_path_lane.hpp"
#include "pqp_banded_qp.hpp"
#include "pqp_wave.hpp"
#include "pqp_internal.hpp"

using namespace pqp_internal;

#include "pqp_smoother_kernels.inc"

// ---------------------------------------------------------------------------------------------------------
// smoother QPs, and the speed refine's QP on the same core (pqp_speed.hip)
// ---------------------------------------------------------------------------------------------------------
namespace {
enum { SM_TENSION2 = kBandedTension2, SM_TENSION = kBandedTension, SM_POST = kBandedPost, SM_REFINE = kBandedRefine };

struct SmShape { int nv, nc, bw, pbw, stride; };
SmShape sm_shape(int type, int n) {
    if (type == SM_TENSION2) return {4 * n - 1, 3 * (n - 1) + 2, 4, 4, 4};
    if (type == SM_TENSION) return {3 * n, 3 * n, 9, 9, 3};
    if (type == SM_REFINE) return {3 * n, 5 * n - 2, 3, 3, 3};
    return {3 * n, 3 * n - 2, 3, 0, 3};
}

// shared sparsity of a QP family in the interleaved variable order: integer host logic (like pqp_path_sizes)
int sm_upload_structure(pqp_handle* h, BandedGroup& g, int type, int n) {
    if (g.struct_type == type && g.struct_n == n) return PQP_OK;
    // a host -> device copy from vectors that go out of scope + a synchronise: not something a capturing stream may do.  The capture of
    // pqp_optimize_path_device is abandoned cleanly (the body fails, the call falls back to plain launches and never captures these arguments again:
    // a chain whose smoothers alternate between two structure types on the generic core uploads on every call)
    if (h->chain.capturing) return fail(PQP_ERR_INVALID, "smoother structure upload inside a graph capture");
    const SmShape sh = sm_shape(type, n);
    std::vector<int> acol((size_t)sh.nc * pqp::kRMax, -1), trow((size_t)sh.nv * pqp::kCMax, -1), tslot((size_t)sh.nv * pqp::kCMax, 0);
    auto row = [&](int r, int c0, int c1, int c2, int c3 = -1) { int* a = &acol[(size_t)r * pqp::kRMax]; a[0] = c0; a[1] = c1; a[2] = c2; a[3] = c3; };
    if (type == SM_TENSION2) {
        for (int i = 0; i < n - 1; ++i) {
            row(i, 4 * (i + 1), 4 * i, 4 * i + 2);
            row(n - 1 + i, 4 * (i + 1) + 1, 4 * i + 1, 4 * i + 2);
            row(2 * (n - 1) + i, 4 * (i + 1) + 2, 4 * i + 2, 4 * i + 3);
        }
        row(3 * (n - 1), 0, -1, -1);
        row(3 * (n - 1) + 1, 1, -1, -1);
    } else if (type == SM_TENSION) {
        for (int i = 0; i < n; ++i) { row(i, 3 * i, 3 * i + 2, -1); row(n + i, 3 * i + 1, 3 * i + 2, -1); row(2 * n + i, 3 * i + 2, -1, -1); }
    } else if (type == SM_REFINE) {
        // (s, v, a)_k -> 3k + {0, 1, 2}.  rows k, m + k, 2m + k: the boxes of s_k, v_k, a_k;  3m + k: s_{k+1} - s_k - dt v_k - dt^2/2 a_k;
        // 4m - 1 + k: v_{k+1} - v_k - dt a_k  (refine_assemble_kernel writes the values in this slot order)
        for (int k = 0; k < n; ++k) { row(k, 3 * k, -1, -1); row(n + k, 3 * k + 1, -1, -1); row(2 * n + k, 3 * k + 2, -1, -1); }
        for (int k = 0; k < n - 1; ++k) { row(3 * n + k, 3 * k, 3 * k + 1, 3 * k + 2, 3 * k + 3); row(4 * n - 1 + k, 3 * k + 1, 3 * k + 2, 3 * k + 4); }
    } else {
        for (int i = 0; i < n; ++i) row(i, 3 * i, -1, -1);
        for (int i = 0; i < n - 1; ++i) { row(n + i, 3 * (i + 1), 3 * i, 3 * i + 1); row(2 * n - 1 + i, 3 * (i + 1) + 1, 3 * i + 1, 3 * i + 2); }
    }
    std::vector<int> fill(sh.nv, 0);
    for (int r = 0; r < sh.nc; ++r)
        for (int s = 0; s < pqp::kRMax; ++s) {
            const int c = acol[(size_t)r * pqp::kRMax + s];
            if (c < 0) continue;
            if (fill[c] >= pqp::kCMax) return fail(PQP_ERR_INVALID, "smoother structure: column overflow");
            trow[(size_t)c * pqp::kCMax + fill[c]] = r; tslot[(size_t)c * pqp::kCMax + fill[c]] = s; ++fill[c];
        }
    int rc;
    if ((rc = g.acol.ensure(acol.size() * 4)) || (rc = g.trow.ensure(trow.size() * 4)) || (rc = g.tslot.ensure(tslot.size() * 4))) return rc;
    PQP_HIP(hipMemcpyAsync(g.acol.p, acol.data(), acol.size() * 4, hipMemcpyHostToDevice, h->stream));
    PQP_HIP(hipMemcpyAsync(g.trow.p, trow.data(), trow.size() * 4, hipMemcpyHostToDevice, h->stream));
    PQP_HIP(hipMemcpyAsync(g.tslot.p, tslot.data(), tslot.size() * 4, hipMemcpyHostToDevice, h->stream));
    PQP_HIP(hipStreamSynchronize(h->stream));      // the vectors go out of scope
    g.struct_type = type; g.struct_n = n;
    return PQP_OK;
}
}  // namespace

namespace pqp_internal {

// assemble (already enqueued by the caller into g.pband ...) -> banded ADMM solve.  All device pointers.  n_of: the counts the assemble
// kernel padded by (or nullptr)
int sm_solve(pqp_handle* h, BandedGroup& g, const pqp_params& prm, int type, int batch, int n, const int32_t* n_of, int32_t* status, int32_t* iters,
             double* info, bool timed) {
    const SmShape sh = sm_shape(type, n);
    pqp::BandedQpArgs a;
    std::memset(&a, 0, sizeof(a));
    a.batch = batch; a.nv = sh.nv; a.nc = sh.nc; a.bw = sh.bw; a.pbw = sh.pbw;
    a.pband = g.pband.as<double>(); a.q = g.q.as<double>(); a.acol = g.acol.as<int>(); a.aval = g.aval.as<double>();
    a.trow = g.trow.as<int>(); a.tslot = g.tslot.as<int>(); a.lo = g.lo.as<double>(); a.up = g.up.as<double>();
    a.x = g.x.as<double>(); a.y = g.y.as<double>(); a.status = status; a.iters = iters; a.info = info; a.prm = prm;
    a.n_of = n_of; a.n_pts = n; a.n_min = type == SM_TENSION2 ? 2 : (type == SM_TENSION ? 4 : 1); a.per_pt = sh.stride;      // (n_min: the assemble kernels' clamps)
    pqp::resolve_banded_params(&a.prm);
    // the row data of A, the index lists and q staged in LDS once per QP (256-lane kernels: always - two of them still share a CU's LDS up
    // to 80 KB each; 512-lane kernels: when it fits; 1024-lane kernels: never)
    const size_t lds0 = (size_t)pqp::BqLayout{sh.nv, sh.nc, sh.bw}.total(false) * 8, lds1 = (size_t)pqp::BqLayout{sh.nv, sh.nc, sh.bw}.total(true) * 8;
    const int nbb = pqp::BqLayout{sh.nv, sh.nc, sh.bw}.nbb();
    const int threads = 64 * ((nbb + 63) / 64);        // one lane per (padded) variable
    if (threads > 1024) return fail(PQP_ERR_CAPACITY, "smoother QP has more than 1024 variables");
    const bool stage = threads <= 512 && lds1 <= kLdsPerCu;
    const size_t lds = stage ? lds1 : lds0;
    const void* fn = nullptr;
#define PQP_BQ_PICK(BB) fn = (threads <= 256 && stage) ? (const void*)pqp::banded_solve_kernel<BB, 256, true> : threads <= 512 ? (stage ? (const void*)pqp::banded_solve_kernel<BB, 512, true> : (const void*)pqp::banded_solve_kernel<BB, 512, false>) : (const void*)pqp::banded_solve_kernel<BB, 1024, false>
    switch (sh.bw) {
        case 3: PQP_BQ_PICK(3); break;
        case 4: PQP_BQ_PICK(4); break;
        case 9: PQP_BQ_PICK(9); break;
        default: return fail(PQP_ERR_INVALID, "unsupported smoother block size");
    }
#undef PQP_BQ_PICK
    const int rc = lds_opt_in(fn, lds, "smoother QP too large for one CU's LDS");
    if (rc) return rc;
    const auto launch = [&]() -> int {
        void* kargs[] = {(void*)&a};
        PQP_HIP(hipLaunchKernel(fn, dim3(batch), dim3(threads), kargs, lds, h->stream));
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    };
    return timed ? h->launch_timed(launch) : launch();
}

bool sm_generic_fits(int type, int n) {
    const SmShape sh = sm_shape(type, n);
    const pqp::BqLayout lay{sh.nv, sh.nc, sh.bw};
    return (size_t)lay.total(false) * 8 <= kLdsPerCu && 64 * ((lay.nbb() + 63) / 64) <= 1024;
}

int sm_alloc(pqp_handle* h, BandedGroup& g, int type, int batch, int n) {
    const SmShape sh = sm_shape(type, n);
    int rc;
    if ((rc = g.pband.ensure((size_t)batch * (sh.pbw + 1) * sh.nv * 8)) || (rc = g.q.ensure((size_t)batch * sh.nv * 8)) ||
        (rc = g.aval.ensure((size_t)batch * sh.nc * pqp::kRMax * 8)) || (rc = g.lo.ensure((size_t)batch * sh.nc * 8)) ||
        (rc = g.up.ensure((size_t)batch * sh.nc * 8)) || (rc = g.x.ensure((size_t)batch * sh.nv * 8)) || (rc = g.y.ensure((size_t)batch * sh.nc * 8)))
        return rc;
    return sm_upload_structure(h, g, type, n);
}

}  // namespace pqp_internal

namespace {
// the smoothers' own group, under the handle's parameters
int sm_solve(pqp_handle* h, int type, int batch, int n, const int32_t* n_of, int32_t* status, int32_t* iters, double* info) {
    return sm_solve(h, h->sm, h->prm, type, batch, n, n_of, status, iters, info, true);
}
int sm_alloc(pqp_handle* h, int type, int batch, int n) { return sm_alloc(h, h->sm, type, batch, n); }
}  // namespace

extern "C" {

static bool tension2_ok(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list, const double* k_list,
                        const double* s_list, const double* out_x, const double* out_y, const double* out_s) {
    return h && x_list && y_list && angle_list && k_list && s_list && out_x && out_y && out_s && batch >= 1 && n >= 3;
}

// TensionSmoother2::osqpSmooth (tension_smoother_2.cpp:20-72), device pointers, all lists [batch][n]; n_of [batch] (device) or nullptr
static int smooth_tension2_impl(pqp_handle* h, int batch, int n, const int32_t* n_of, const double* x_list, const double* y_list,
                                const double* angle_list, const double* k_list, const double* s_list, double* out_x, double* out_y, double* out_s,
                                int32_t* status, int32_t* iters, double* info) {
    if (!tension2_ok(h, batch, n, x_list, y_list, angle_list, k_list, s_list, out_x, out_y, out_s))
        return fail(PQP_ERR_INVALID, "pqp_smooth_tension2: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    int rc;
    if (h->prm.polish != 0 || !sm_generic_fits(SM_TENSION2, n)) {
        // exact optima asked for (or more points than the generic core holds: 203, where its LDS ends - sm_generic_fits; tension_smoother_2.cpp:20-72 has
        // no cap): the QP has equality rows only - its optimum by one Riccati sweep per scenario (tension2_exact_kernel)
        if (!status) return fail(PQP_ERR_INVALID, "pqp_smooth_tension2: status is null");
        if ((rc = h->sm.pband.ensure((size_t)batch * n * 5 * 8)) || (rc = h->sm.aval.ensure((size_t)batch * n * 6 * 8))) return rc;
        hipLaunchKernelGGL(pqp::tension2_stage_kernel, dim3((batch * n + 255) / 256), dim3(256), 0, h->stream, batch, n, n_of, x_list, y_list, angle_list, k_list,
                           s_list, h->sm.aval.as<double>());
        PQP_HIP(hipGetLastError());
        return h->launch_timed([&]() -> int {
            hipLaunchKernelGGL(pqp::tension2_exact_kernel, dim3((batch + 63) / 64), dim3(64), 0, h->stream, batch, n, n_of, x_list, y_list,
                               h->prm.tension2_deviation_weight, h->prm.tension2_curvature_weight, h->prm.tension2_curvature_rate_weight, h->sm.aval.as<double>(),
                               h->sm.pband.as<double>(), out_x, out_y, out_s, status, iters, info);
            PQP_HIP(hipGetLastError());
            return PQP_OK;
        });
    }
    if ((rc = sm_alloc(h, SM_TENSION2, batch, n))) return rc;
    const int total = batch * n;
    hipLaunchKernelGGL(pqp::tension2_assemble_kernel, dim3((total + 255) / 256), dim3(256), 0, h->stream, batch, n, n_of, x_list, y_list, angle_list,
                       k_list, s_list, h->prm.tension2_deviation_weight, h->prm.tension2_curvature_weight, h->prm.tension2_curvature_rate_weight,
                       h->sm.pband.as<double>(), h->sm.q.as<double>(), h->sm.aval.as<double>(), h->sm.lo.as<double>(), h->sm.up.as<double>());
    PQP_HIP(hipGetLastError());
    if ((rc = sm_solve(h, SM_TENSION2, batch, n, n_of, status, iters, info))) return rc;
    hipLaunchKernelGGL(pqp::tension_finish_kernel, dim3(batch), dim3(64), (size_t)n * 8, h->stream, batch, n, n_of, 4 * n - 1, 4, h->sm.x.as<double>(), out_x, out_y, out_s);
    PQP_HIP(hipGetLastError());
    return PQP_OK;
}

int pqp_smooth_tension2_device(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list,
                               const double* k_list, const double* s_list, double* out_x, double* out_y, double* out_s, int32_t* status,
                               int32_t* iters, double* info) {
    return smooth_tension2_impl(h, batch, n, nullptr, x_list, y_list, angle_list, k_list, s_list, out_x, out_y, out_s, status, iters, info);
}

int pqp_smooth_tension2_var_device(pqp_handle* h, int batch, int n_max, const int32_t* n_of, const double* x_list, const double* y_list,
                                   const double* angle_list, const double* k_list, const double* s_list, double* out_x, double* out_y,
                                   double* out_s, int32_t* status, int32_t* iters, double* info) {
    if (!n_of) return fail(PQP_ERR_INVALID, "pqp_smooth_tension2_var: n_of is null");
    return smooth_tension2_impl(h, batch, n_max, n_of, x_list, y_list, angle_list, k_list, s_list, out_x, out_y, out_s, status, iters, info);
}

static bool tension_ok(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list, const double* clearance,
                       const double* out_x, const double* out_y, const double* out_s) {
    return h && x_list && y_list && angle_list && clearance && out_x && out_y && out_s && batch >= 1 && n >= 4;
}

// TensionSmoother::osqpSmooth (tension_smoother.cpp:49-100); clearance[batch][n] = Map::getObstacleDistance at each point; n_of [batch]
// (device) or nullptr
static int smooth_tension_impl(pqp_handle* h, int batch, int n, const int32_t* n_of, const double* x_list, const double* y_list, const double* angle_list,
                               const double* clearance, double* out_x, double* out_y, double* out_s, int32_t* status, int32_t* iters, double* info) {
    if (!tension_ok(h, batch, n, x_list, y_list, angle_list, clearance, out_x, out_y, out_s)) return fail(PQP_ERR_INVALID, "pqp_smooth_tension: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    int rc;
    // The generic block-cyclic-reduction core keeps a QP's vectors, factor rows and row data in one compute unit's LDS: in TensionSmoother's
    // 9 x 9 blocks that ends at 203 points (sm_generic_fits; S1 also at 203, postSmooth at 251 layers).  The reference has no such limit (tension_smoother.cpp:49-100; segmentRawReference gives a
    // point per metre of line).  Beyond it, also a handle in the reference's ADMM setting gets the exact kernel's optimum: a point with
    // zero residuals meets OSQP's termination test at any eps, so it IS a valid result of that setting (iters = 0; OSQP itself would
    // stop at a less accurate one).
    const bool generic_fits = sm_generic_fits(SM_TENSION, n);
    if (h->prm.polish == 1 || !generic_fits) {
        // exact optima asked for (or the only kernel that holds the QP): the box QP in the lateral shifts alone, one wavefront per scenario (tension_exact_kernel)
        if (!status) return fail(PQP_ERR_INVALID, "pqp_smooth_tension: status is null");
        const double wk = h->prm.cartesian_curvature_weight, wdk = h->prm.cartesian_curvature_rate_weight, wdev = h->prm.cartesian_deviation_weight, tol = h->prm.polish_tol;
        signed char* act_io;
        int carry;
        if ((rc = sm_carry_slot(h, 0, batch, n, act_io, carry))) return rc;
        // (any line longer than 1024 points - the reference has no cap: tension_smoother.cpp:49-100 - runs with its arrays in HBM)
        return sm_exact_launch(h, batch, n, pqp::kTensionExactArrays, [&](auto K, double* ws) {
            hipLaunchKernelGGL(pqp::tension_exact_kernel<K>, dim3(batch), dim3(64), 0, h->stream, batch, n, n_of, x_list, y_list, angle_list, clearance, wk, wdk,
                               wdev, tol, out_x, out_y, out_s, status, iters, info, act_io, carry, ws);
        });
    }
    if ((rc = sm_alloc(h, SM_TENSION, batch, n))) return rc;
    const int total = batch * n;
    hipLaunchKernelGGL(pqp::tension_assemble_kernel, dim3((total + 255) / 256), dim3(256), 0, h->stream, batch, n, n_of, x_list, y_list, angle_list, clearance,
                       h->prm.cartesian_curvature_weight, h->prm.cartesian_curvature_rate_weight, h->prm.cartesian_deviation_weight,
                       h->sm.pband.as<double>(), h->sm.q.as<double>(), h->sm.aval.as<double>(), h->sm.lo.as<double>(), h->sm.up.as<double>());
    PQP_HIP(hipGetLastError());
    if ((rc = sm_solve(h, SM_TENSION, batch, n, n_of, status, iters, info))) return rc;
    hipLaunchKernelGGL(pqp::tension_finish_kernel, dim3(batch), dim3(64), (size_t)n * 8, h->stream, batch, n, n_of, 3 * n, 3, h->sm.x.as<double>(), out_x, out_y, out_s);
    PQP_HIP(hipGetLastError());
    return PQP_OK;
}

int pqp_smooth_tension_device(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list,
                              const double* clearance, double* out_x, double* out_y, double* out_s, int32_t* status, int32_t* iters, double* info) {
    return smooth_tension_impl(h, batch, n, nullptr, x_list, y_list, angle_list, clearance, out_x, out_y, out_s, status, iters, info);
}

int pqp_smooth_tension_var_device(pqp_handle* h, int batch, int n_max, const int32_t* n_of, const double* x_list, const double* y_list,
                                  const double* angle_list, const double* clearance, double* out_x, double* out_y, double* out_s, int32_t* status,
                                  int32_t* iters, double* info) {
    if (!n_of) return fail(PQP_ERR_INVALID, "pqp_smooth_tension_var: n_of is null");
    return smooth_tension_impl(h, batch, n_max, n_of, x_list, y_list, angle_list, clearance, out_x, out_y, out_s, status, iters, info);
}

static bool post_smooth_ok(pqp_handle* h, int batch, int m, const double* layers_s, const double* lb, const double* ub, const double* vehicle_l,
                           const double* out_l) {
    return h && layers_s && lb && ub && vehicle_l && out_l && batch >= 1 && m >= 4;
}

// ReferencePathSmoother::postSmooth QP (reference_path_smoother.cpp:526-558): out_l[batch][m] = the lateral offsets l_i
static int post_smooth_impl(pqp_handle* h, int batch, int m, const int32_t* m_of, const double* layers_s, const double* lb, const double* ub,
                            const double* vehicle_l, double* out_l, int32_t* status, int32_t* iters, double* info) {
    if (!post_smooth_ok(h, batch, m, layers_s, lb, ub, vehicle_l, out_l)) return fail(PQP_ERR_INVALID, "pqp_post_smooth: bad argument (m >= 4, reference_path_smoother.cpp:528)");
    PQP_HIP(hipSetDevice(h->device));
    int rc;
    // (beyond what the generic core holds in a CU's LDS also a handle in the reference's ADMM setting gets the exact kernel's optimum, as in smooth_tension_impl)
    if (h->prm.polish == 1 || !sm_generic_fits(SM_POST, m)) {
        // exact optima asked for: the box QP in the offsets alone, one wavefront per scenario (post_exact_kernel)
        if (!status) return fail(PQP_ERR_INVALID, "pqp_post_smooth: status is null");
        const double tol = h->prm.polish_tol;
        signed char* act_io;
        int carry;
        if ((rc = sm_carry_slot(h, 1, batch, m, act_io, carry))) return rc;
        // (any corridor longer than 1024 layers - reference_path_smoother.cpp:526-580 has no cap - runs with its arrays in HBM)
        return sm_exact_launch(h, batch, m, pqp::kPostExactArrays, [&](auto K, double* ws) {
            hipLaunchKernelGGL(pqp::post_exact_kernel<K>, dim3(batch), dim3(64), 0, h->stream, batch, m, m_of, layers_s, lb, ub, vehicle_l, tol, out_l, status,
                               iters, info, act_io, carry, ws);
        });
    }
    if ((rc = sm_alloc(h, SM_POST, batch, m))) return rc;
    const int total = batch * m;
    hipLaunchKernelGGL(pqp::post_assemble_kernel, dim3((total + 255) / 256), dim3(256), 0, h->stream, batch, m, m_of, layers_s, lb, ub, vehicle_l,
                       h->sm.pband.as<double>(), h->sm.q.as<double>(), h->sm.aval.as<double>(), h->sm.lo.as<double>(), h->sm.up.as<double>());
    PQP_HIP(hipGetLastError());
    if ((rc = sm_solve(h, SM_POST, batch, m, m_of, status, iters, info))) return rc;
    hipLaunchKernelGGL(pqp::post_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, h->stream, batch, m, h->sm.x.as<double>(), out_l);
    PQP_HIP(hipGetLastError());
    return PQP_OK;
}

int pqp_post_smooth_device(pqp_handle* h, int batch, int m, const double* layers_s, const double* lb, const double* ub, const double* vehicle_l,
                           double* out_l, int32_t* status, int32_t* iters, double* info) {
    return post_smooth_impl(h, batch, m, nullptr, layers_s, lb, ub, vehicle_l, out_l, status, iters, info);
}

int pqp_post_smooth_var_device(pqp_handle* h, int batch, int m_max, const int32_t* m_of, const double* layers_s, const double* lb, const double* ub,
                               const double* vehicle_l, double* out_l, int32_t* status, int32_t* iters, double* info) {
    if (!m_of) return fail(PQP_ERR_INVALID, "pqp_post_smooth_var: m_of is null");
    return post_smooth_impl(h, batch, m_max, m_of, layers_s, lb, ub, vehicle_l, out_l, status, iters, info);
}

int pqp_smooth_tension2(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list, const double* k_list,
                        const double* s_list, double* out_x, double* out_y, double* out_s, int32_t* status, int32_t* iters) {
    if (!tension2_ok(h, batch, n, x_list, y_list, angle_list, k_list, s_list, out_x, out_y, out_s)) return fail(PQP_ERR_INVALID, "pqp_smooth_tension2: bad argument");
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double *d_x = st.in(x_list, bn), *d_y = st.in(y_list, bn), *d_angle = st.in(angle_list, bn), *d_k = st.in(k_list, bn), *d_s = st.in(s_list, bn);
    double *o_x = st.out(out_x, bn), *o_y = st.out(out_y, bn), *o_s = st.out(out_s, bn);
    int32_t *d_status = st.out(status, batch), *d_iters = st.out(iters, batch);
    return st.run([&]() -> int { return pqp_smooth_tension2_device(h, batch, n, d_x, d_y, d_angle, d_k, d_s, o_x, o_y, o_s, d_status, d_iters, nullptr); });
}

int pqp_smooth_tension(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list, const double* clearance,
                       double* out_x, double* out_y, double* out_s, int32_t* status, int32_t* iters) {
    if (!tension_ok(h, batch, n, x_list, y_list, angle_list, clearance, out_x, out_y, out_s)) return fail(PQP_ERR_INVALID, "pqp_smooth_tension: bad argument");
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double *d_x = st.in(x_list, bn), *d_y = st.in(y_list, bn), *d_angle = st.in(angle_list, bn), *d_clr = st.in(clearance, bn);
    double *o_x = st.out(out_x, bn), *o_y = st.out(out_y, bn), *o_s = st.out(out_s, bn);
    int32_t *d_status = st.out(status, batch), *d_iters = st.out(iters, batch);
    return st.run([&]() -> int { return pqp_smooth_tension_device(h, batch, n, d_x, d_y, d_angle, d_clr, o_x, o_y, o_s, d_status, d_iters, nullptr); });
}

int pqp_post_smooth(pqp_handle* h, int batch, int m, const double* layers_s, const double* lb, const double* ub, const double* vehicle_l, double* out_l,
                    int32_t* status, int32_t* iters) {
    if (!post_smooth_ok(h, batch, m, layers_s, lb, ub, vehicle_l, out_l)) return fail(PQP_ERR_INVALID, "pqp_post_smooth: bad argument");
    const size_t bm = (size_t)batch * m;
    Staging st(h);
    const double *d_s = st.in(layers_s, bm), *d_lb = st.in(lb, bm), *d_ub = st.in(ub, bm), *d_vl = st.in(vehicle_l, batch);
    double* o_l = st.out(out_l, bm);
    int32_t *d_status = st.out(status, batch), *d_iters = st.out(iters, batch);
    return st.run([&]() -> int { return pqp_post_smooth_device(h, batch, m, d_s, d_lb, d_ub, d_vl, o_l, d_status, d_iters, nullptr); });
}

}  // extern "C"
