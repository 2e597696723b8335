// pqp_chain.hip — PathOptimizer::solve (reference src/path_optimizer.cpp:34-71) for a batch of scenarios
// as ONE device-resident call: input points -> optimised paths, nothing copied to the host between the steps, every scenario with its
// own point / sample / layer / waypoint counts.
//
//   reference step                                                             here (all on the handles' streams, device pointers)
//   ReferencePathSmoother::bSpline               reference_path_smoother.cpp:490-521   pqp_bspline_resample_device
//   tk::spline::set_points (raw line)            :58-59                                pqp_spline_fit_var_device
//   segmentRawReference                          :48-85                                pqp_segment_raw_reference_device
//   TensionSmoother2::osqpSmooth                 tension_smoother_2.cpp:20-72          pqp_smooth_tension2_var_device   (smoother handle)
//   set_points (smoothed line), length + 3       tension_smoother.cpp:36-41            pqp_spline_fit_var_device, chain_length_kernel
//   graphSearchDp                                reference_path_smoother.cpp:142-295   pqp_dp_corridor_device
//   postSmooth QP (needs >= 4 layers)            :526-558                              pqp_post_smooth_var_device       (smoother handle)
//   postSmooth tail: offsets -> points, spline   :559-577                              pqp_offsets_to_points_device, pqp_spline_fit_var_device
//   processInitState, 75 degree test             path_optimizer.cpp:73-85,112-116      pqp_reference_states_device (init_err), chain_scal_kernel
//   setReferencePathLength                       :87-104                               pqp_reference_length_device
//   buildReferenceFromSpline(ds / 2, ds)         :119, reference_path_impl.cpp:314-338 pqp_reference_states_device
//   updateBounds                                 :120, reference_path_impl.cpp:177-312 pqp_corridor_bounds_device
//   optimizePath                                 :124-161                              pqp_path_solve_var_device (passes = 1)
//   ... or, second_pass = PQP_SECOND_PASS_BOUNDS_ON_STATES, the lines commented out there (:141-151):
//   BaseSolver::solve                            :142                                  pqp_path_solve_var_device (passes = 0)
//   updateBoundsOnInputStates                    :147, reference_path_impl.cpp:118-175 pqp_corridor_bounds_on_states_device, chain_scal_kernel
//   BaseSolver post_solver(..., *final_path).solve   :149-150                          chain_lin_kernel, pqp_path_solve_var_device (passes = 0, lin)
// The steps are the `_device` entry points of the other translation units; this one holds the chain's own small kernels and its graph capture.
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
#include "pqp_line_device.hpp"
#include "pqp_internal.hpp"
#include "pqp_chain_ws.hpp"

using namespace pqp_internal;

namespace pqp {

struct ChainScalArgs {
    int batch, n_max;
    const double* ref;          // [batch][n_max][5]
    const int32_t* count;       // [batch] reference states
    const int32_t* n_valid;     // [batch] waypoints before the road is blocked
    const double* init_err;     // [batch][2]
    const double* target;       // [batch][3]
    const double* start_k;      // [batch] or nullptr
    double max_steering_angle;
    double* scal;               // [batch][6]
};
// scal row of every scenario: what BaseSolver reads from VehicleState / ReferencePath (base_solver.cpp:216-220,254-258)
__global__ void chain_scal_kernel(const ChainScalArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    double* s = a.scal + (size_t)b * PQP_SCAL_STRIDE;
    s[0] = a.init_err[2 * b]; s[1] = a.init_err[2 * b + 1];
    s[2] = a.start_k ? a.start_k[b] : 0.0;                              // start_state.k (State's default: 0, data_struct.hpp:14-26)
    s[3] = a.target[3 * b + 2];
    s[4] = a.n_valid[b] < a.count[b] ? 1.0 : 0.0;                       // ReferencePath::isBlocked()
    s[5] = a.max_steering_angle;
}

struct ChainStatusArgs {
    int batch, n_max, raw_max, sample_max, layer_max, sample_min;     // sample_min: 3 (TensionSmoother2), 4 (TensionSmoother's kernels need the third-difference window)
    const int32_t *n_points, *raw_count, *sample_count, *sm_status, *layer_count, *ps_status, *ref_count, *n_valid, *qp_status;
    const double* init_err;
    int32_t* stage;             // [batch] where the scenario stopped (pqp_chain_stage), 0 = a path came out
    int32_t* status;            // [batch] pqp_status of the path QP, PQP_STATUS_UNSOLVED when the scenario never got there
    int32_t* n_out;             // [batch] waypoints of the path
};
__global__ void chain_status_kernel(const ChainStatusArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    int stage = PQP_CHAIN_OK;
    if (a.n_points[b] < 4) stage = PQP_CHAIN_FEW_POINTS;                                               // reference_path_smoother.cpp:33-36
    else if (a.raw_count[b] < 1) stage = PQP_CHAIN_FEW_POINTS;                                         // no raw line: more points than p_max, or not more than the B-spline's degree (pqp.h)
    else if (a.raw_count[b] > a.raw_max || a.sample_count[b] > a.sample_max || a.sample_count[b] < a.sample_min) stage = PQP_CHAIN_CAPACITY;
    else if (a.sm_status[b] != PQP_STATUS_SOLVED) stage = PQP_CHAIN_SMOOTHER_FAILED;                   // "Tension smoother failed!"
    else if (a.layer_count[b] < 0) stage = PQP_CHAIN_CAPACITY;
    else if (a.layer_count[b] == 0) stage = PQP_CHAIN_SEARCH_FAILED;                                   // graphSearchDp false
    else if (a.layer_count[b] < 4) stage = PQP_CHAIN_SHORT_REFERENCE;                                  // postSmooth: "Ref is short" (:528-531)
    else if (a.ps_status[b] != PQP_STATUS_SOLVED) stage = PQP_CHAIN_POST_SMOOTH_FAILED;
    else if (fabs(a.init_err[2 * b + 1]) > 75.0 * kPi / 180.0) stage = PQP_CHAIN_HEADING;                // path_optimizer.cpp:113-116
    else if (a.ref_count[b] > a.n_max) stage = PQP_CHAIN_CAPACITY;
    else if (a.n_valid[b] < 2) stage = PQP_CHAIN_BLOCKED;
    else if (a.qp_status[b] != PQP_STATUS_SOLVED) stage = PQP_CHAIN_PATH_QP_FAILED;                    // "Solving failed!" (:143-156)
    a.stage[b] = stage;
    a.status[b] = (stage == PQP_CHAIN_OK || stage == PQP_CHAIN_PATH_QP_FAILED) ? a.qp_status[b] : PQP_STATUS_UNSOLVED;
    a.n_out[b] = (stage == PQP_CHAIN_OK) ? a.n_valid[b] : 0;
}

// second_pass = BOUNDS_ON_STATES, between the bounds on the first path and the second solve: the post_solver's linearisation point (its
// input_path_ = the first path: l, d_heading, k at offsets 3, 4, 5 of `out`, base_solver.cpp:266-289) and its waypoint count - the new
// n_valid, or 0 where the first solve is not SOLVED ("Pre solving failed!": no second pass, path_optimizer.cpp:142-146)
__global__ void chain_lin_kernel(int batch, int n_max, const double* __restrict__ out, const int32_t* __restrict__ status1,
                                 const int32_t* __restrict__ n_valid2, double* __restrict__ lin, int32_t* __restrict__ n_of2) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * n_max) return;
    const double* o = out + (size_t)idx * PQP_OUT_STRIDE;
    double* l = lin + (size_t)idx * PQP_LIN_STRIDE;
    l[0] = o[3]; l[1] = o[4]; l[2] = o[5];
    const int b = idx / n_max;
    if (idx - b * n_max == 0) n_of2[b] = status1[b] == PQP_STATUS_SOLVED ? n_valid2[b] : 0;
}

// ... and after the second solve: what chain_status_kernel reads as the path QP's waypoint count and status - the first solve's where it
// failed, the second's otherwise - and the iterations of both solves (a QP either solve skipped counts 0 there)
__global__ void chain_second_pass_kernel(int batch, const int32_t* __restrict__ status1, const int32_t* __restrict__ n_valid1,
                                         const int32_t* __restrict__ status2, const int32_t* __restrict__ n_valid2, const int32_t* __restrict__ iters1,
                                         const int32_t* __restrict__ iters2, int32_t* __restrict__ status, int32_t* __restrict__ n_valid,
                                         int32_t* __restrict__ iters) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const bool first_ok = status1[b] == PQP_STATUS_SOLVED;
    status[b] = first_ok ? status2[b] : status1[b];
    n_valid[b] = first_ok ? n_valid2[b] : n_valid1[b];
    if (iters) iters[b] = iters1[b] + iters2[b];
}

// Map::getObstacleDistance at the points of the raw line: the clearance input of the TensionSmoother QP (tension_smoother.cpp:168;
// src/tools/Map.cpp:16-22).  One thread per point; the layer (<= 2 MB) is L2-resident.
__global__ void clearance_kernel(int batch, int n, const int32_t* __restrict__ n_of, const double* __restrict__ x, const double* __restrict__ y,
                                 const float* __restrict__ dist, const int32_t* __restrict__ map_of, pqp_grid_geometry g, double* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * n) return;
    const int b = idx / n;
    if (n_of && idx - b * n >= n_of[b]) { out[idx] = 0.0; return; }      // beyond the scenario's points: nothing to look up
    const float* layer = dist + (size_t)(map_of ? map_of[b] : 0) * g.rows * g.cols;
    out[idx] = obstacle_distance(layer, g, x[idx], y[idx]);
}

// counts clamped into what the next step can take (a scenario that overflowed a capacity is flagged by chain_status_kernel and must
// not make the next kernel read beyond its arrays).  With x / y / s (the raw line's lists, [batch][stride]): a scenario without a line
// (count 0: the step wrote none of its rows) gets the point (0, 0) at abscissa 0 as its first row - what the degenerate branch of the
// spline fit and gather_last_kernel read for it - so that the steps behind it run on a line of length 0 and not on what an earlier
// call left in the workspace
__global__ void chain_clamp_kernel(int batch, const int32_t* __restrict__ in, int lo, int hi, int32_t* __restrict__ out, int stride,
                                   double* __restrict__ x, double* __restrict__ y, double* __restrict__ s) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const int v = in[b];
    out[b] = v < lo ? lo : (v > hi ? hi : v);
    if (x && v < 1) { x[(size_t)b * stride] = 0.0; y[(size_t)b * stride] = 0.0; s[(size_t)b * stride] = 0.0; }
}

// dst[b] = src[b][count[b] - 1] + add: the length of a line from its abscissa list (the hand-over between the chain's steps)
__global__ void gather_last_kernel(int batch, int stride, const int32_t* __restrict__ count, const double* __restrict__ src, double add,
                                   double* __restrict__ dst) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    int c = count[b];
    c = c < 1 ? 1 : (c > stride ? stride : c);
    dst[b] = src[(size_t)b * stride + c - 1] + add;
}

}  // namespace pqp

extern "C" {

void pqp_chain_default_config(pqp_chain_config* c) {
    if (!c) return;
    c->raw_max = 160; c->sample_max = 128; c->layer_max = 96; c->n_max = 256;
    c->output_spacing = 0.3;                       // planning_flags.cpp:106
    c->dynamic_segmentation = 1;                   // :110
    c->max_steering_angle = 35.0 * 3.14159265358979323846 / 180.0;      // :22
    c->smoothed_length_margin = 3.0;               // tension_smoother.cpp:40
    c->smoothing_method = PQP_SMOOTHING_TENSION2;  // planning_flags.cpp:27
    c->second_pass = PQP_SECOND_PASS_RELINEARISE;  // path_optimizer.cpp:150 as it stands
    pqp_corridor_default_params(&c->corridor);
    pqp_dp_default_params(&c->dp);
}

int pqp_clearance_device(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const float* dist, const int32_t* map_of,
                         const pqp_grid_geometry* geom, double* clearance) {
    if (!h || !x_list || !y_list || !dist || !geometry_ok(geom) || !clearance || batch < 1 || n < 1) return fail(PQP_ERR_INVALID, "pqp_clearance: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    const int total = batch * n;
    hipLaunchKernelGGL(pqp::clearance_kernel, dim3((total + 255) / 256), dim3(256), 0, h->stream, batch, n, (const int32_t*)nullptr, x_list, y_list, dist, map_of, *geom, clearance);
    PQP_HIP(hipGetLastError());
    return PQP_OK;
}

// ordering between the two handles of the chain on events of their own (pqp_mark's slots 0..7 stay the caller's)
static int chain_mark(pqp_handle* h, int k) {
    PQP_HIP(hipSetDevice(h->device));
    PQP_HIP(hipEventRecord(h->marks[pqp_handle::kMarks + k], h->stream));
    return PQP_OK;
}
static int chain_wait(pqp_handle* h, pqp_handle* other, int k) {
    PQP_HIP(hipSetDevice(h->device));
    PQP_HIP(hipStreamWaitEvent(h->stream, other->marks[pqp_handle::kMarks + k], 0));
    return PQP_OK;
}

// the launches of the chain, enqueued on the two handles' streams (plainly, or into a stream capture: pqp_optimize_path_device below)
static int chain_body(pqp_handle* h, pqp_handle* hs, const pqp_chain_config& cfg, int batch, int p_max, const double* points,
                      const int32_t* n_points, const double* start, const double* target, const float* dist, const int32_t* map_of,
                      const pqp_grid_geometry* geom, const double* start_k, double* out, int32_t* n_out, int32_t* status, int32_t* stage,
                      int32_t* iters) {
    const int R = cfg.raw_max, S = cfg.sample_max, L = cfg.layer_max, N = cfg.n_max;
    int rc;
    // ---- workspace: measured and carved from the one list of its arrays (pqp_chain_ws.hpp) ------------------------------------------
    const bool second = cfg.second_pass == PQP_SECOND_PASS_BOUNDS_ON_STATES;
    const ChainDims dims{R, S, L, N, second};
    ChainWs w;
    const ChainWsSize need = carve(w, dims, (size_t)batch, nullptr, nullptr);
    if ((rc = h->chain.d.ensure(need.doubles * 8)) || (rc = h->chain.i.ensure(need.ints * 4))) return rc;
    carve(w, dims, (size_t)batch, h->chain.d.as<double>(), h->chain.i.as<int32_t>());
    const dim3 gb((batch + 255) / 256), tb(256);
    auto clamp = [&](const int32_t* in, int lo, int hi, int32_t* o, double* x = nullptr, double* y = nullptr, double* s = nullptr) {
        hipLaunchKernelGGL(pqp::chain_clamp_kernel, gb, tb, 0, h->stream, batch, in, lo, hi, o, hi, x, y, s);
    };
    auto last = [&](int stride, const int32_t* count, const double* src, double add, double* dst) {
        hipLaunchKernelGGL(pqp::gather_last_kernel, gb, tb, 0, h->stream, batch, stride, count, src, add, dst);
    };
    const bool two = hs != h;
    // ---- reference line smoothing (ReferencePathSmoother::solve) -------------------------------------------------------------------
    if ((rc = pqp_bspline_resample_device(h, batch, p_max, R, points, n_points, w.rx, w.ry, w.rs, w.raw_count))) return rc;
    clamp(w.raw_count, 0, R, w.raw_fit, w.rx, w.ry, w.rs);
    if ((rc = pqp_spline_fit_var_device(h, batch, R, w.raw_fit, w.rs, w.rx, w.ry, w.raw_tab, w.raw_ext))) return rc;
    last(R, w.raw_fit, w.rs, 0.0, w.raw_len);
    if ((rc = pqp_segment_raw_reference_device(h, batch, S, R, w.raw_tab, w.raw_ext, w.raw_len, 1.0, w.gx, w.gy, w.gs, w.ga, w.gk, w.sample_count))) return rc;
    clamp(w.sample_count, 0, S, w.sample_fit);
    if (two) { if ((rc = chain_mark(h, 1)) || (rc = chain_wait(hs, h, 1))) return rc; }
    if (cfg.smoothing_method == PQP_SMOOTHING_TENSION) {
        // TensionSmoother (ReferencePathSmoother::create, reference_path_smoother.cpp:20-24): the obstacle distance at the raw line's 1 m
        // samples bounds their lateral shift (tension_smoother.cpp:163-175)
        hipLaunchKernelGGL(pqp::clearance_kernel, dim3((batch * S + 255) / 256), dim3(256), 0, hs->stream, batch, S, w.sample_fit, w.gx, w.gy, dist, map_of, *geom, w.clr);
        PQP_HIP(hipGetLastError());
        if ((rc = pqp_smooth_tension_var_device(hs, batch, S, w.sample_fit, w.gx, w.gy, w.ga, w.clr, w.sx, w.sy, w.ss, w.sm_status, w.sm_iters, nullptr))) return rc;
    } else {
        if ((rc = pqp_smooth_tension2_var_device(hs, batch, S, w.sample_fit, w.gx, w.gy, w.ga, w.gk, w.gs, w.sx, w.sy, w.ss, w.sm_status, w.sm_iters, nullptr))) return rc;
    }
    if (two) { if ((rc = chain_mark(hs, 1)) || (rc = chain_wait(h, hs, 1))) return rc; }
    if ((rc = pqp_spline_fit_var_device(h, batch, S, w.sample_fit, w.ss, w.sx, w.sy, w.sm_tab, w.sm_ext))) return rc;
    last(S, w.sample_fit, w.ss, cfg.smoothed_length_margin, w.sm_len);
    if ((rc = pqp_dp_corridor_device(h, batch, S, L, w.sm_tab, w.sm_ext, w.sm_len, start, dist, map_of, geom, &cfg.dp, w.ls, w.lb, w.ub, w.layer_count, w.vl))) return rc;
    clamp(w.layer_count, 0, L, w.layer_fit);
    if (two) { if ((rc = chain_mark(h, 0)) || (rc = chain_wait(hs, h, 0))) return rc; }
    if ((rc = pqp_post_smooth_var_device(hs, batch, L, w.layer_fit, w.ls, w.lb, w.ub, w.vl, w.pl, w.ps_status, w.ps_iters, nullptr))) return rc;
    if (two) { if ((rc = chain_mark(hs, 0)) || (rc = chain_wait(h, hs, 0))) return rc; }
    if ((rc = pqp_offsets_to_points_device(h, batch, S, L, w.sm_tab, w.sm_ext, w.ls, w.pl, w.layer_fit, w.px, w.py, w.ps))) return rc;
    if ((rc = pqp_spline_fit_var_device(h, batch, L, w.layer_fit, w.ps, w.px, w.py, w.fin_tab, w.fin_ext))) return rc;
    last(L, w.layer_fit, w.ps, 0.0, w.fin_len);
    // ---- PathOptimizer::processReferencePath ----------------------------------------------------------------------------------------
    if ((rc = pqp_reference_length_device(h, batch, L, w.fin_tab, w.fin_ext, w.fin_len, target, w.max_s))) return rc;
    if ((rc = pqp_reference_states_device(h, batch, N, L, w.fin_tab, w.fin_ext, w.max_s, start, cfg.output_spacing / 2.0, cfg.output_spacing,
                                          cfg.dynamic_segmentation ? 1 : 0, w.ref, w.ref_count, w.err))) return rc;
    clamp(w.ref_count, 0, N, w.ref_fit);
    if ((rc = pqp_corridor_bounds_device(h, batch, N, L, w.ref, w.ref_fit, w.fin_tab, w.fin_ext, dist, map_of, geom, &cfg.corridor, w.bounds, w.n_valid))) return rc;
    pqp::ChainScalArgs sa{batch, N, w.ref, w.ref_fit, w.n_valid, w.err, target, start_k, cfg.max_steering_angle, w.scal};
    hipLaunchKernelGGL(pqp::chain_scal_kernel, gb, tb, 0, h->stream, sa);
    // ---- PathOptimizer::optimizePath ---------------------------------------------------------------------------------------------------
    const int32_t *qp_n = w.n_valid, *qp_st = w.qp_status;          // what chain_status_kernel reads
    if (!second) {
        if ((rc = pqp_path_solve_var_device(h, batch, N, w.n_valid, w.ref, nullptr, w.bounds, w.scal, /*passes=*/1, 0, out, w.qp_status, iters, nullptr))) return rc;
    } else {
        // solver.solve(final_path) (:142), cold
        if ((rc = pqp_path_solve_var_device(h, batch, N, w.n_valid, w.ref, nullptr, w.bounds, w.scal, /*passes=*/0, 0, out, w.qp_status, w.iters1, nullptr))) return rc;
        // reference_path_->updateBoundsOnInputStates(*grid_map_, *final_path) (:147) on the first path's states (its n_valid of them).  The
        // bounds of the first pass are no longer read: the new ones take their place
        if ((rc = pqp_corridor_bounds_on_states_device(h, batch, N, L, w.ref, w.n_valid, out, PQP_OUT_STRIDE, w.fin_tab, w.fin_ext, dist, map_of, geom,
                                                       &cfg.corridor, w.bounds, w.n_valid2))) return rc;
        // the post_solver reads isBlocked() again: with count = the reference states before either cut, n_valid2 < count holds when either
        // pass was blocked (n_valid2 <= n_valid <= count), which is blocked_bound_ never being reset (reference_path_impl.cpp:167,222)
        pqp::ChainScalArgs sa2{batch, N, w.ref, w.ref_fit, w.n_valid2, w.err, target, start_k, cfg.max_steering_angle, w.scal};
        hipLaunchKernelGGL(pqp::chain_scal_kernel, gb, tb, 0, h->stream, sa2);
        hipLaunchKernelGGL(pqp::chain_lin_kernel, dim3((batch * N + 255) / 256), tb, 0, h->stream, batch, N, (const double*)out, (const int32_t*)w.qp_status,
                           (const int32_t*)w.n_valid2, w.lin, w.n_of2);
        PQP_HIP(hipGetLastError());
        // BaseSolver post_solver(*reference_path_, *vehicle_state_, *final_path); post_solver.solve(final_path) (:149-150): a cold solve
        // around the first path, on the new bounds and the new n_valid waypoints (a scenario that keeps fewer than 2 is left alone: BLOCKED)
        if ((rc = pqp_path_solve_var_device(h, batch, N, w.n_of2, w.ref, w.lin, w.bounds, w.scal, /*passes=*/0, 0, out, w.qp_status2, w.iters2, nullptr))) return rc;
        hipLaunchKernelGGL(pqp::chain_second_pass_kernel, gb, tb, 0, h->stream, batch, (const int32_t*)w.qp_status, (const int32_t*)w.n_valid,
                           (const int32_t*)w.qp_status2, (const int32_t*)w.n_valid2, (const int32_t*)w.iters1, (const int32_t*)w.iters2, w.status_out,
                           w.n_valid_out, iters);
        PQP_HIP(hipGetLastError());
        qp_n = w.n_valid_out; qp_st = w.status_out;
    }
    pqp::ChainStatusArgs st{batch, N, R, S, L, cfg.smoothing_method == PQP_SMOOTHING_TENSION ? 4 : 3, n_points, w.raw_count, w.sample_count, w.sm_status, w.layer_count, w.ps_status, w.ref_count, qp_n, qp_st,
                            w.err, stage ? stage : w.ref_fit /* scratch */, status, n_out};
    hipLaunchKernelGGL(pqp::chain_status_kernel, gb, tb, 0, h->stream, st);
    PQP_HIP(hipGetLastError());
    return PQP_OK;
}

// Everything that decides what chain_body enqueues, as bytes: a captured graph is replayed only for the identical key.  The call's own
// arguments, the configuration, and of both handles the parameters, the options (whole) and what each group of host state says a captured
// launch depends on (its key(), pqp_internal.hpp); then the library's allocation generation (a graph holds device pointers of the
// handles' workspaces).
static Key chain_key(pqp_handle* h, pqp_handle* hs, const pqp_chain_config& cfg, int batch, int p_max, const void* const* ptrs, int n_ptrs,
                     const pqp_grid_geometry* geom) {
    Key k;
    k.v.reserve(1024);
    k.put(&h, sizeof(h)); k.put(&hs, sizeof(hs));
    k.put_int(batch); k.put_int(p_max);
    for (int i = 0; i < n_ptrs; ++i) k.put(&ptrs[i], sizeof(void*));
    k.bytes(*geom);
    // (pqp_chain_config has padding behind its int members: field by field; its sub-structs have none, pqp_internal.hpp)
    k.put_int(cfg.raw_max); k.put_int(cfg.sample_max); k.put_int(cfg.layer_max); k.put_int(cfg.n_max); k.put(&cfg.output_spacing, 8); k.put_int(cfg.dynamic_segmentation);
    k.put(&cfg.max_steering_angle, 8); k.put(&cfg.smoothed_length_margin, 8); k.put_int(cfg.smoothing_method); k.put_int(cfg.second_pass);
    k.bytes(cfg.corridor); k.bytes(cfg.dp);
    for (const pqp_handle* x : {h, hs}) {
        k.bytes(x->prm);
        k.bytes(x->opt);
        x->lane.key(k); x->strm.key(k); x->sm.key(k);
    }
    k.put_int((long long)g_alloc_generation.load(std::memory_order_relaxed));
    return k;
}

int pqp_optimize_path_device(pqp_handle* h, pqp_handle* hs, const pqp_chain_config* cfg_in, int batch, int p_max, const double* points,
                             const int32_t* n_points, const double* start, const double* target, const float* dist, const int32_t* map_of,
                             const pqp_grid_geometry* geom, const double* start_k, double* out, int32_t* n_out, int32_t* status, int32_t* stage,
                             int32_t* iters) {
    if (!h || !points || !n_points || !start || !target || !dist || !geom || !out || !n_out || !status || batch < 1 || p_max < 4)
        return fail(PQP_ERR_INVALID, "pqp_optimize_path: bad argument");
    pqp_chain_config cfg;
    if (cfg_in) cfg = *cfg_in; else pqp_chain_default_config(&cfg);
    const int R = cfg.raw_max, S = cfg.sample_max, L = cfg.layer_max, N = cfg.n_max;
    if (cfg.smoothing_method != PQP_SMOOTHING_TENSION2 && cfg.smoothing_method != PQP_SMOOTHING_TENSION)
        return fail(PQP_ERR_INVALID, "pqp_optimize_path: smoothing_method is neither TENSION2 nor TENSION (\"No such smoother!\", reference_path_smoother.cpp:25-28)");
    if (cfg.second_pass != PQP_SECOND_PASS_RELINEARISE && cfg.second_pass != PQP_SECOND_PASS_BOUNDS_ON_STATES)
        return fail(PQP_ERR_INVALID, "pqp_optimize_path: second_pass is neither RELINEARISE nor BOUNDS_ON_STATES");
    // (the reference's post_solver would see s = 0 on every input state - getOptimizedPath never sets s, base_solver.cpp:266-289 - and so
    //  another precise-planning count than the one the path solve computes from the reference states: pqp.h, pqp_second_pass)
    if (cfg.second_pass == PQP_SECOND_PASS_BOUNDS_ON_STATES && h->prm.rough_constraints_far_away)
        return fail(PQP_ERR_INVALID, "pqp_optimize_path: second_pass = BOUNDS_ON_STATES with rough_constraints_far_away on the path handle");
    // (no upper bounds here - the reference has none: every step below checks what it can hold, the smoother QPs and the path QP of any size go
    //  to the kernels that keep their state in HBM; the steps that stage a line's spline table in a CU's LDS take lines of any length with
    //  PQP_OPT_LONG_LINES on the path handle, where they all run)
    if (R < 8 || S < 4 || L < 4 || N < 2) return fail(PQP_ERR_CAPACITY, "pqp_optimize_path: capacities out of range (raw_max >= 8, sample_max >= 4, layer_max >= 4, n_max >= 2)");
    if (!hs) hs = h;
    if (hs->device != h->device) return fail(PQP_ERR_INVALID, "pqp_optimize_path: the smoother handle lives on another device than the path handle");
    PQP_HIP(hipSetDevice(h->device));
    auto body = [&]() { return chain_body(h, hs, cfg, batch, p_max, points, n_points, start, target, dist, map_of, geom, start_k, out, n_out, status, stage, iters); };
    if (!h->opt.chain_graph) return body();
    // ---- PQP_OPT_CHAIN_GRAPH: the first call with a key runs plain (it sizes every workspace and uploads what is uploaded once), the second call
    //      with that key is captured and launched, later ones are replays.  The key holds the launch parity of the path handle's cost-order double
    //      buffer, so a caller sees: plain, plain (other parity), capture, capture (other parity), replays - two graphs per argument set ----
    const void* ptrs[] = {points, n_points, start, target, dist, map_of, start_k, out, n_out, status, stage, iters};
    const Key key = chain_key(h, hs, cfg, batch, p_max, ptrs, (int)(sizeof(ptrs) / sizeof(ptrs[0])), geom);
    pqp_handle::ChainGraph* g = nullptr;
    for (auto& e : h->chain.graphs) if (e.key == key) { g = &e; break; }
    auto after_replay = [&](const pqp_handle::ChainGraph& e) {
        h->lane.replayed(e.replay);
        // no timing events inside a graph: pqp_last_kernel_ms / pqp_kernel_ms_history have nothing newer than the last plain launch to report
        h->timing.timed = false; hs->timing.timed = false;
    };
    // A replay runs as one unit on the path handle's stream; the smoother handle's stream is not part of it.  So that it stays ordered with
    // what the caller enqueues on that stream before and after - as the plain launches are, some of which run there - the graph waits for
    // the smoother stream's earlier work and the smoother stream's later work waits for the graph.
    // (The two fences cost 3.6 % of a replay, profiles/r04n_chain_fence.txt.  Option value 2: no fences - the caller guarantees that the
    //  smoother handle's stream carries no other work while chains are in flight.)
    const bool fenced = hs != h && h->opt.chain_graph != 2;
    auto launch = [&](hipGraphExec_t exec) -> int {
        if (fenced) { int r; if ((r = chain_mark(hs, 1)) || (r = chain_wait(h, hs, 1))) return r; }
        PQP_HIP(hipGraphLaunch(exec, h->stream));
        if (fenced) { int r; if ((r = chain_mark(h, 1)) || (r = chain_wait(hs, h, 1))) return r; }
        return PQP_OK;
    };
    if (g && g->exec) {
        const int rl = launch(g->exec);
        if (rl != PQP_OK) return rl;
        after_replay(*g);
        return PQP_OK;
    }
    if (!g) {
        if (h->chain.graphs.size() >= 16) {          // (a caller that keeps changing its buffers: stop collecting)
            for (auto& e : h->chain.graphs) if (e.exec) (void)hipGraphExecDestroy(e.exec);
            h->chain.graphs.clear();
        }
        h->chain.graphs.emplace_back();
        h->chain.graphs.back().key = key;
        return body();
    }
    if (g->failed) return body();
    // capture: the smoother handle's stream joins through the chain's own events and is joined back before the end
    const pqp_handle::LanePath::Mark before = h->lane.mark();
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) { g->failed = true; return body(); }
    h->chain.capturing = true; hs->chain.capturing = true;
    const int rc = body();
    h->chain.capturing = false; hs->chain.capturing = false;
    e = hipStreamEndCapture(h->stream, &graph);
    hipGraphExec_t exec = nullptr;
    if (rc == PQP_OK && e == hipSuccess && graph) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (rc != PQP_OK || e != hipSuccess || !exec) {
        // nothing of the captured body has run: undo its host-side bookkeeping and run it plainly
        (void)hipGetLastError();
        g->failed = true;
        h->lane.rewind(before);
        return body();
    }
    g->exec = exec;
    g->replay = h->lane.captured(before);           // (the capture counted launches that only happen now, with every replay)
    const int rl = launch(g->exec);
    if (rl != PQP_OK) return rl;
    after_replay(*g);
    return PQP_OK;
}

}  // extern "C"
