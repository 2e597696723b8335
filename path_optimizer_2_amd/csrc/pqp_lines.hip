// pqp_lines.hip — the line-geometry entry points of include/pqp.h: corridor bounds (on reference states and on the states of a solved path),
// reference states and raw-reference segmentation, offsets to points, reference length, B-spline resampling, spline fit, the layered DP
// corridor search, and the projection of points onto a line.  Their kernels in the LDS and the long form (pqp_corridor_kernels.inc with its
// pqp_*_body.inc, pqp_project_kernels.inc), launchers and entry points.
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
#include "pqp_wave.hpp"
#include "pqp_line_device.hpp"
#include "pqp_internal.hpp"

using namespace pqp_internal;

#include "pqp_corridor_kernels.inc"
#include "pqp_project_kernels.inc"

extern "C" {

// ---- corridor bounds from the distance map -----------------------------------------------------------
void pqp_corridor_default_params(pqp_corridor_params* p) {
    if (!p) return;
    p->front_length = 3.9; p->rear_length = -1.0;       // planning_flags.cpp:20,18
    p->car_width = 2.0; p->safety_margin = 0.3;         // planning_flags.cpp:10,14
    p->epsilon = 1e-6;                                  // planning_flags.cpp:108
    p->search_radius = 0.5; p->delta_s = 0.3; p->smaller_ds = 0.05; p->search_range = 6.0; p->min_space = 0.2;   // reference_path_impl.cpp:238-304
    p->projection_window = 5.0;                         // reference_path_impl.cpp:194
}

static bool corridor_ok(pqp_handle* h, int batch, int n, int m, const double* ref, const double* spline, const double* spline_ext, const float* dist,
                        const pqp_grid_geometry* geom, const pqp_corridor_params* prm, const double* bounds, const int32_t* n_valid) {
    return h && ref && spline && spline_ext && dist && prm && bounds && n_valid && batch >= 1 && n >= 1 && m >= 3 && geometry_ok(geom) &&
           prm->delta_s > 0.0 && prm->smaller_ds > 0.0;
}

// the waypoints kernel `fn` (corridor_bounds_kernel / states_bounds_kernel) holds in LDS at a time: a whole scenario's probes when they fit
// (9 m + 33 n doubles), tiles of waypoints otherwise: any path length.  Sets *lds to the dynamic LDS of that tile and opts in to it.
static int corridor_tile(const void* fn, int m, int n, int* tile, size_t* lds, const char* who) {
    *tile = n;
    size_t fixed = 0;
    if (const int rc = static_lds(fn, &fixed)) return rc;
    if (pqp::CorridorLds{m, n}.total_bytes() > kLdsPerCu - fixed) {
        const long long room = (long long)(kLdsPerCu - fixed) - (long long)pqp::CorridorLds{m, 0}.total_bytes(), per_waypoint = (long long)(pqp::CorridorLds{m, 1}.total_bytes() - pqp::CorridorLds{m, 0}.total_bytes());
        if (room < 16 * per_waypoint) return fail(PQP_ERR_CAPACITY, std::string(who) + ": the line's spline table (9 m doubles) does not leave room for the probes in one CU's LDS");
        *tile = (int)(room / per_waypoint);
    }
    *lds = pqp::CorridorLds{m, *tile}.total_bytes();
    return lds_opt_in(fn, *lds, (std::string(who) + ": scenario too large for one CU's LDS (about 9 m + 31 n doubles)").c_str());
}

// PQP_OPT_LONG_LINES on a corridor launch: the long kernel `long_fn` (the table in HBM, tiles of probes in LDS) where `fn` would refuse
// the line's table (1) or always (2); *fn_out and the tile / LDS of the launch accordingly
static int corridor_pick(int opt, const void* fn, const void* long_fn, int m, int n, const void** fn_out, int* tile, size_t* lds, const char* who) {
    // (what corridor_tile refuses: the table and the fewest probes `fn` runs on, a tile of 16 waypoints or all n, exceed one CU's LDS)
    bool go_long = false;
    if (const int rc = long_form(opt, fn, pqp::CorridorLds{m, n < 16 ? n : 16}.total_bytes(), &go_long)) return rc;
    *fn_out = go_long ? long_fn : fn;
    return corridor_tile(*fn_out, go_long ? 0 : m, n, tile, lds, who);
}

// the sample loops are strided; 512 lanes per scenario keep the most gathers in flight per CU (measured at batch 1024 x n = 80: 1024 lanes
// 142 us - two scenarios per CU -, 512: 121, 256: 120, 128: 146)
constexpr int kCorridorThreads = 512;

int pqp_corridor_bounds_device(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* spline,
                               const double* spline_ext, const float* dist, const int32_t* map_of, const pqp_grid_geometry* geom,
                               const pqp_corridor_params* prm, double* bounds, int32_t* n_valid) {
    if (!corridor_ok(h, batch, n, m, ref, spline, spline_ext, dist, geom, prm, bounds, n_valid))
        return fail(PQP_ERR_INVALID, "pqp_corridor_bounds: bad argument (m >= 3 knots: spline.cpp:164; a map layer of 2 x 2 to 2^30 cells)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::CorridorArgs a;
    a.batch = batch; a.n = n; a.m = m; a.ref = ref; a.spl = spline; a.spl_ext = spline_ext; a.dist = dist; a.map_of = map_of; a.n_of = n_of;
    a.g = *geom; a.p = *prm; a.bounds = bounds; a.n_valid = n_valid;
    size_t lds = 0;
    const void* fn = nullptr;
    if (const int rc = corridor_pick(h->opt.long_lines, (const void*)pqp::corridor_bounds_kernel, (const void*)pqp::long_corridor_kernel, m, n, &fn, &a.tile, &lds,
                                     "pqp_corridor_bounds")) return rc;
    return h->launch_timed([&]() -> int {
        if (fn == (const void*)pqp::long_corridor_kernel) hipLaunchKernelGGL(pqp::long_corridor_kernel, dim3(batch), dim3(kCorridorThreads), lds, h->stream, a);
        else hipLaunchKernelGGL(pqp::corridor_bounds_kernel, dim3(batch), dim3(kCorridorThreads), lds, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_corridor_bounds(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* spline,
                        const double* spline_ext, const float* dist, int n_maps, const int32_t* map_of, const pqp_grid_geometry* geom,
                        const pqp_corridor_params* prm, double* bounds, int32_t* n_valid) {
    if (!corridor_ok(h, batch, n, m, ref, spline, spline_ext, dist, geom, prm, bounds, n_valid) || n_maps < 1)
        return fail(PQP_ERR_INVALID, "pqp_corridor_bounds: bad argument");
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_ref = st.in(ref, bn * PQP_REF_STRIDE);
    const int32_t* d_n_of = st.in(n_of, batch);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4);
    const float* d_dist = st.in(dist, (size_t)n_maps * geom->rows * geom->cols);
    const int32_t* d_map_of = st.in(map_of, batch);
    double* d_bounds = st.out(bounds, bn * PQP_BOUNDS_STRIDE);
    int32_t* d_n_valid = st.out(n_valid, batch);
    return st.run([&]() -> int { return pqp_corridor_bounds_device(h, batch, n, m, d_ref, d_n_of, d_spl, d_ext, d_dist, d_map_of, geom, prm, d_bounds, d_n_valid); });
}

// ---- corridor bounds on the states of a solved path (ReferencePathImpl::updateBoundsOnInputStates) ----------------------------------
static bool corridor_states_ok(pqp_handle* h, int batch, int n, int m, const double* ref, const double* states, int stride, const double* spline,
                               const double* spline_ext, const float* dist, const pqp_grid_geometry* geom, const pqp_corridor_params* prm,
                               const double* bounds, const int32_t* n_valid) {
    return corridor_ok(h, batch, n, m, ref, spline, spline_ext, dist, geom, prm, bounds, n_valid) && states && stride >= 5;
}

int pqp_corridor_bounds_on_states_device(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* states,
                                         int stride, const double* spline, const double* spline_ext, const float* dist, const int32_t* map_of,
                                         const pqp_grid_geometry* geom, const pqp_corridor_params* prm, double* bounds, int32_t* n_valid) {
    if (!corridor_states_ok(h, batch, n, m, ref, states, stride, spline, spline_ext, dist, geom, prm, bounds, n_valid))
        return fail(PQP_ERR_INVALID, "pqp_corridor_bounds_on_states: bad argument (stride >= 5; m >= 3 knots; a map layer of 2 x 2 to 2^30 cells)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::CorridorArgs a;
    a.batch = batch; a.n = n; a.m = m; a.ref = ref; a.spl = spline; a.spl_ext = spline_ext; a.dist = dist; a.map_of = map_of; a.n_of = n_of;
    a.g = *geom; a.p = *prm; a.bounds = bounds; a.n_valid = n_valid;
    size_t lds = 0;
    const void* fn = nullptr;
    if (const int rc = corridor_pick(h->opt.long_lines, (const void*)pqp::states_bounds_kernel, (const void*)pqp::long_states_kernel, m, n, &fn, &a.tile, &lds,
                                     "pqp_corridor_bounds_on_states")) return rc;
    return h->launch_timed([&]() -> int {
        if (fn == (const void*)pqp::long_states_kernel) hipLaunchKernelGGL(pqp::long_states_kernel, dim3(batch), dim3(kCorridorThreads), lds, h->stream, a, states, stride);
        else hipLaunchKernelGGL(pqp::states_bounds_kernel, dim3(batch), dim3(kCorridorThreads), lds, h->stream, a, states, stride);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_corridor_bounds_on_states(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* states, int stride,
                                  const double* spline, const double* spline_ext, const float* dist, int n_maps, const int32_t* map_of,
                                  const pqp_grid_geometry* geom, const pqp_corridor_params* prm, double* bounds, int32_t* n_valid) {
    if (!corridor_states_ok(h, batch, n, m, ref, states, stride, spline, spline_ext, dist, geom, prm, bounds, n_valid) || n_maps < 1)
        return fail(PQP_ERR_INVALID, "pqp_corridor_bounds_on_states: bad argument");
    if (map_of)
        for (int b = 0; b < batch; ++b)
            if (map_of[b] < 0 || map_of[b] >= n_maps) return fail(PQP_ERR_INVALID, "pqp_corridor_bounds_on_states: map_of outside [0, n_maps)");
    if (n_of)       // CHECK_LE(input_sl_states.size(), reference_states_.size()) (reference_path_impl.cpp:119)
        for (int b = 0; b < batch; ++b)
            if (n_of[b] < 0 || n_of[b] > n) return fail(PQP_ERR_INVALID, "pqp_corridor_bounds_on_states: n_of outside [0, n] (more states than reference states)");
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_ref = st.in(ref, bn * PQP_REF_STRIDE);
    const int32_t* d_n_of = st.in(n_of, batch);
    const double* d_states = st.in(states, bn * stride);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4);
    const float* d_dist = st.in(dist, (size_t)n_maps * geom->rows * geom->cols);
    const int32_t* d_map_of = st.in(map_of, batch);
    double* d_bounds = st.out(bounds, bn * PQP_BOUNDS_STRIDE, n_of ? 0 : -1);      // (rows beyond a scenario's states are not written)
    int32_t* d_n_valid = st.out(n_valid, batch);
    return st.run([&]() -> int {
        return pqp_corridor_bounds_on_states_device(h, batch, n, m, d_ref, d_n_of, d_states, stride, d_spl, d_ext, d_dist, d_map_of, geom, prm, d_bounds, d_n_valid);
    });
}

// ---- points onto their reference line: Cartesian to Frenet (getProjection + global2Local, tools.cpp:57-126) -------------------------------
static const char* const kProjectBad =
    "pqp_project_points: bad argument (batch >= 1, m >= 2, 1 <= q_max <= 256 * 65535, stride >= 2, stride >= 3 with has_heading)";

static bool project_ok(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length, int q_max, int stride,
                       int has_heading, const double* points, const double* proj, const int32_t* flags) {
    return h && spline && spline_ext && length && points && proj && flags && batch >= 1 && m >= 2 && q_max >= 1 &&
           q_max <= pqp::kProjectThreads * 65535 && stride >= (has_heading ? 3 : 2);
}

int pqp_project_points_device(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length, int q_max,
                              int stride, int has_heading, const double* points, const int32_t* q_of, double* proj, int32_t* flags) {
    if (!project_ok(h, batch, m, spline, spline_ext, length, q_max, stride, has_heading, points, proj, flags)) return fail(PQP_ERR_INVALID, kProjectBad);
    PQP_HIP(hipSetDevice(h->device));
    pqp::ProjectArgs a;
    a.batch = batch; a.m = m; a.q_max = q_max; a.stride = stride; a.has_heading = has_heading ? 1 : 0; a.spl = spline; a.spl_ext = spline_ext;
    a.length = length; a.points = points; a.q_of = q_of; a.proj = proj; a.flags = flags;
    const dim3 grid((unsigned)batch, (unsigned)((q_max + pqp::kProjectThreads - 1) / pqp::kProjectThreads));
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::project_points_kernel, grid, dim3(pqp::kProjectThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_project_points(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length, int q_max,
                       int stride, int has_heading, const double* points, const int32_t* q_of, double* proj, int32_t* flags) {
    if (!project_ok(h, batch, m, spline, spline_ext, length, q_max, stride, has_heading, points, proj, flags)) return fail(PQP_ERR_INVALID, kProjectBad);
    const size_t rows = (size_t)batch * q_max;
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4), *d_length = st.in(length, batch);
    const double* d_points = st.in(points, rows * stride);
    const int32_t* d_q_of = st.in(q_of, batch);
    double* d_proj = st.out(proj, rows * PQP_PROJ_STRIDE);
    int32_t* d_flags = st.out(flags, rows);
    return st.run([&]() -> int {
        return pqp_project_points_device(h, batch, m, d_spl, d_ext, d_length, q_max, stride, has_heading, d_points, d_q_of, d_proj, d_flags);
    });
}

// ---- reference states + initial error ----------------------------------------------------------------
static bool reference_states_ok(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext, const double* max_s,
                                const double* start, double ds_small, double ds_large, const double* ref, const int32_t* count, const double* init_err) {
    return h && spline && spline_ext && max_s && ref && count && batch >= 1 && n_max >= 1 && m >= 3 && ds_small > 0.0 && ds_large >= ds_small &&
           (!init_err || start);
}

int pqp_reference_states_device(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext,
                                const double* max_s, const double* start, double ds_small, double ds_large, int dynamic, double* ref,
                                int32_t* count, double* init_err) {
    if (!reference_states_ok(h, batch, n_max, m, spline, spline_ext, max_s, start, ds_small, ds_large, ref, count, init_err))
        return fail(PQP_ERR_INVALID, "pqp_reference_states: bad argument (0 < ds_small <= ds_large: reference_path_impl.cpp:315)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::RefStatesArgs a;
    a.batch = batch; a.n_max = n_max; a.m = m; a.spl = spline; a.spl_ext = spline_ext; a.max_s = max_s; a.start = start;
    a.ds_small = ds_small; a.ds_large = ds_large; a.dynamic = dynamic ? 1 : 0; a.ref = ref; a.count = count; a.init_err = init_err;
    a.lx = a.ly = a.ls = a.langle = a.lk = nullptr;
    const size_t lds = ((size_t)9 * m + n_max) * 8;
    return line_launch(h, (const void*)pqp::reference_states_kernel, lds, "pqp_reference_states: 9 m + n_max doubles exceed one CU's LDS", 0,
                       [&](auto go_long, double*) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_ref_states_kernel, dim3(batch), dim3(64), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::reference_states_kernel, dim3(batch), dim3(64), lds, h->stream, a);
    });
}

// ---- raw reference line -> the smoother QPs' input lists (ReferencePathSmoother::segmentRawReference) ------------------------------
static bool segment_ok(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext, const double* max_s, double delta_s,
                       const double* x, const double* y, const double* s, const double* angle, const double* k, const int32_t* count) {
    return h && spline && spline_ext && max_s && x && y && s && angle && k && count && batch >= 1 && n_max >= 1 && m >= 3 && delta_s > 0.0;
}

int pqp_segment_raw_reference_device(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext,
                                     const double* max_s, double delta_s, double* x, double* y, double* s, double* angle, double* k,
                                     int32_t* count) {
    if (!segment_ok(h, batch, n_max, m, spline, spline_ext, max_s, delta_s, x, y, s, angle, k, count))
        return fail(PQP_ERR_INVALID, "pqp_segment_raw_reference: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    pqp::RefStatesArgs a;
    a.batch = batch; a.n_max = n_max; a.m = m; a.spl = spline; a.spl_ext = spline_ext; a.max_s = max_s; a.start = nullptr;
    a.ds_small = delta_s; a.ds_large = delta_s; a.dynamic = 2; a.ref = nullptr; a.count = count; a.init_err = nullptr;
    a.lx = x; a.ly = y; a.ls = s; a.langle = angle; a.lk = k;
    const size_t lds = ((size_t)9 * m + n_max) * 8;
    return line_launch(h, (const void*)pqp::reference_states_kernel, lds, "pqp_segment_raw_reference: 9 m + n_max doubles exceed one CU's LDS", 0,
                       [&](auto go_long, double*) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_ref_states_kernel, dim3(batch), dim3(64), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::reference_states_kernel, dim3(batch), dim3(64), lds, h->stream, a);
    });
}

int pqp_segment_raw_reference(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext, const double* max_s,
                              double delta_s, double* x, double* y, double* s, double* angle, double* k, int32_t* count) {
    if (!segment_ok(h, batch, n_max, m, spline, spline_ext, max_s, delta_s, x, y, s, angle, k, count))
        return fail(PQP_ERR_INVALID, "pqp_segment_raw_reference: bad argument");
    const size_t bn = (size_t)batch * n_max;
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4), *d_max_s = st.in(max_s, batch);
    double *d_x = st.out(x, bn, 0), *d_y = st.out(y, bn, 0), *d_s = st.out(s, bn, 0), *d_angle = st.out(angle, bn, 0), *d_k = st.out(k, bn, 0);
    int32_t* d_count = st.out(count, batch);
    return st.run([&]() -> int { return pqp_segment_raw_reference_device(h, batch, n_max, m, d_spl, d_ext, d_max_s, delta_s, d_x, d_y, d_s, d_angle, d_k, d_count); });
}

int pqp_reference_states(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext, const double* max_s,
                         const double* start, double ds_small, double ds_large, int dynamic, double* ref, int32_t* count,
                         double* init_err) {
    if (!reference_states_ok(h, batch, n_max, m, spline, spline_ext, max_s, start, ds_small, ds_large, ref, count, init_err))
        return fail(PQP_ERR_INVALID, "pqp_reference_states: bad argument");
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4), *d_max_s = st.in(max_s, batch);
    const double* d_start = st.in(start, (size_t)batch * 3);
    double* d_ref = st.out(ref, (size_t)batch * n_max * PQP_REF_STRIDE, 0);
    int32_t* d_count = st.out(count, batch);
    double* d_err = init_err ? st.out(init_err, (size_t)batch * 2) : nullptr;
    return st.run([&]() -> int {
        return pqp_reference_states_device(h, batch, n_max, m, d_spl, d_ext, d_max_s, d_start, ds_small, ds_large, dynamic, d_ref, d_count, d_err);
    });
}

// ---- lateral offsets on a line -> points with chord-length abscissae (tail of ReferencePathSmoother::postSmooth) ---------------------
static bool offsets_ok(pqp_handle* h, int batch, int m_spline, int m, const double* spline, const double* spline_ext, const double* at_s, const double* l,
                       const double* x, const double* y, const double* s) {
    return h && spline && spline_ext && at_s && l && x && y && s && batch >= 1 && m_spline >= 3 && m >= 1;
}

int pqp_offsets_to_points_device(pqp_handle* h, int batch, int m_spline, int m, const double* spline, const double* spline_ext, const double* at_s,
                                 const double* l, const int32_t* m_of, double* x, double* y, double* s) {
    if (!offsets_ok(h, batch, m_spline, m, spline, spline_ext, at_s, l, x, y, s)) return fail(PQP_ERR_INVALID, "pqp_offsets_to_points: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    pqp::OffsetsArgs a;
    a.batch = batch; a.m_spl = m_spline; a.m = m; a.spl = spline; a.spl_ext = spline_ext; a.at_s = at_s; a.l = l; a.m_of = m_of;
    a.x = x; a.y = y; a.s = s;
    const size_t lds = ((size_t)9 * m_spline + 2 * (size_t)m) * 8;
    return line_launch(h, (const void*)pqp::offsets_to_points_kernel, lds, "pqp_offsets_to_points: 9 m_spline + 2 m doubles exceed one CU's LDS", 0,
                       [&](auto go_long, double*) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_offsets_kernel, dim3(batch), dim3(64), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::offsets_to_points_kernel, dim3(batch), dim3(64), lds, h->stream, a);
    });
}

int pqp_offsets_to_points(pqp_handle* h, int batch, int m_spline, int m, const double* spline, const double* spline_ext, const double* at_s,
                          const double* l, const int32_t* m_of, double* x, double* y, double* s) {
    if (!offsets_ok(h, batch, m_spline, m, spline, spline_ext, at_s, l, x, y, s)) return fail(PQP_ERR_INVALID, "pqp_offsets_to_points: bad argument");
    const size_t bm = (size_t)batch * m;
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m_spline), *d_ext = st.in(spline_ext, (size_t)batch * 4);
    const double *d_at_s = st.in(at_s, bm), *d_l = st.in(l, bm);
    const int32_t* d_m_of = st.in(m_of, batch);
    double *d_x = st.out(x, bm, 0), *d_y = st.out(y, bm, 0), *d_s = st.out(s, bm, 0);
    return st.run([&]() -> int { return pqp_offsets_to_points_device(h, batch, m_spline, m, d_spl, d_ext, d_at_s, d_l, d_m_of, d_x, d_y, d_s); });
}

// ---- length of the reference line up to the target state (PathOptimizer::setReferencePathLength) ---------------------------------
static bool reference_length_ok(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length, const double* target,
                                const double* length_out) {
    return h && spline && spline_ext && length && target && length_out && batch >= 1 && m >= 3;
}

int pqp_reference_length_device(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length,
                                const double* target, double* length_out) {
    if (!reference_length_ok(h, batch, m, spline, spline_ext, length, target, length_out)) return fail(PQP_ERR_INVALID, "pqp_reference_length: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    pqp::RefLengthArgs a;
    a.batch = batch; a.m = m; a.spl = spline; a.spl_ext = spline_ext; a.length = length; a.target = target; a.length_out = length_out;
    const size_t lds = (size_t)9 * m * 8;
    return line_launch(h, (const void*)pqp::reference_length_kernel, lds, "pqp_reference_length: 9 m doubles exceed one CU's LDS", 0,
                       [&](auto go_long, double*) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_ref_length_kernel, dim3(batch), dim3(64), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::reference_length_kernel, dim3(batch), dim3(64), lds, h->stream, a);
    });
}

int pqp_reference_length(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length,
                         const double* target, double* length_out) {
    if (!reference_length_ok(h, batch, m, spline, spline_ext, length, target, length_out)) return fail(PQP_ERR_INVALID, "pqp_reference_length: bad argument");
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4);
    const double *d_length = st.in(length, batch), *d_target = st.in(target, (size_t)batch * 3);
    double* d_out = st.out(length_out, batch);
    return st.run([&]() -> int { return pqp_reference_length_device(h, batch, m, d_spl, d_ext, d_length, d_target, d_out); });
}

// ---- input points -> dense raw reference line (ReferencePathSmoother::bSpline) --------------------------------------------------
static bool bspline_ok(pqp_handle* h, int batch, int p_max, int n_max, const double* points, const int32_t* n_points, const double* x, const double* y,
                       const double* s, const int32_t* count) {
    return h && points && n_points && x && y && s && count && batch >= 1 && p_max >= 4 && n_max >= 2;
}

int pqp_bspline_resample_device(pqp_handle* h, int batch, int p_max, int n_max, const double* points, const int32_t* n_points, double* x,
                                double* y, double* s, int32_t* count) {
    if (!bspline_ok(h, batch, p_max, n_max, points, n_points, x, y, s, count))
        return fail(PQP_ERR_INVALID, "pqp_bspline_resample: bad argument (at least 4 input points: reference_path_smoother.cpp:33)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::BsplineArgs a;
    a.batch = batch; a.p_max = p_max; a.n_max = n_max; a.pts = points; a.n_pts = n_points; a.x = x; a.y = y; a.s = s; a.count = count;
    const size_t lds = ((size_t)3 * p_max + 6 + (size_t)3 * n_max) * 8;
    return line_launch(h, (const void*)pqp::bspline_resample_kernel, lds, "pqp_bspline_resample: 3 p_max + 3 n_max doubles exceed one CU's LDS", (size_t)batch * (p_max + 6) * 8,
                       [&](auto go_long, double* ws) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_bspline_kernel, dim3(batch), dim3(64), 0, h->stream, a, ws);
        else hipLaunchKernelGGL(pqp::bspline_resample_kernel, dim3(batch), dim3(64), lds, h->stream, a);
    });
}

int pqp_bspline_resample(pqp_handle* h, int batch, int p_max, int n_max, const double* points, const int32_t* n_points, double* x, double* y,
                         double* s, int32_t* count) {
    if (!bspline_ok(h, batch, p_max, n_max, points, n_points, x, y, s, count)) return fail(PQP_ERR_INVALID, "pqp_bspline_resample: bad argument");
    const size_t bn = (size_t)batch * n_max;
    Staging st(h);
    const double* d_pts = st.in(points, (size_t)batch * p_max * 2);
    const int32_t* d_n_pts = st.in(n_points, batch);
    double *d_x = st.out(x, bn, 0), *d_y = st.out(y, bn, 0), *d_s = st.out(s, bn, 0);
    int32_t* d_count = st.out(count, batch);
    return st.run([&]() -> int { return pqp_bspline_resample_device(h, batch, p_max, n_max, d_pts, d_n_pts, d_x, d_y, d_s, d_count); });
}

// ---- spline fit ---------------------------------------------------------------------------------------
static bool spline_fit_ok(pqp_handle* h, int batch, int m, const double* s, const double* x, const double* y, const double* spline, const double* spline_ext) {
    return h && s && x && y && spline && spline_ext && batch >= 1 && m >= 3;
}

static int spline_fit_impl(pqp_handle* h, int batch, int m, const int32_t* m_of, const double* s, const double* x, const double* y, double* spline,
                           double* spline_ext) {
    if (!spline_fit_ok(h, batch, m, s, x, y, spline, spline_ext)) return fail(PQP_ERR_INVALID, "pqp_spline_fit: bad argument (m >= 3: spline.cpp:164)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::SplineFitArgs a;
    a.m_of = m_of;
    a.batch = batch; a.m = m; a.s = s; a.vx = x; a.vy = y; a.spl = spline; a.spl_ext = spline_ext;
    const size_t lds = (size_t)7 * m * 8;
    return line_launch(h, (const void*)pqp::spline_fit_kernel, lds, "pqp_spline_fit: 7 m doubles exceed one CU's LDS", (size_t)2 * batch * lds,
                       [&](auto go_long, double* ws) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_fit_kernel, dim3(2 * batch), dim3(64), 0, h->stream, a, ws);
        else hipLaunchKernelGGL(pqp::spline_fit_kernel, dim3(2 * batch), dim3(64), lds, h->stream, a);
    });
}

int pqp_spline_fit_device(pqp_handle* h, int batch, int m, const double* s, const double* x, const double* y, double* spline,
                          double* spline_ext) {
    return spline_fit_impl(h, batch, m, nullptr, s, x, y, spline, spline_ext);
}

int pqp_spline_fit_var_device(pqp_handle* h, int batch, int m_max, const int32_t* m_of, const double* s, const double* x, const double* y,
                              double* spline, double* spline_ext) {
    if (!m_of) return fail(PQP_ERR_INVALID, "pqp_spline_fit_var: m_of is null");
    return spline_fit_impl(h, batch, m_max, m_of, s, x, y, spline, spline_ext);
}

int pqp_spline_fit(pqp_handle* h, int batch, int m, const double* s, const double* x, const double* y, double* spline, double* spline_ext) {
    if (!spline_fit_ok(h, batch, m, s, x, y, spline, spline_ext)) return fail(PQP_ERR_INVALID, "pqp_spline_fit: bad argument");
    const size_t bm = (size_t)batch * m;
    Staging st(h);
    const double *d_s = st.in(s, bm), *d_x = st.in(x, bm), *d_y = st.in(y, bm);
    double *d_spl = st.out(spline, 9 * bm), *d_ext = st.out(spline_ext, (size_t)batch * 4);
    return st.run([&]() -> int { return pqp_spline_fit_device(h, batch, m, d_s, d_x, d_y, d_spl, d_ext); });
}

// ---- layered DP corridor search ------------------------------------------------------------------------
void pqp_dp_default_params(pqp_dp_params* p) {
    if (!p) return;
    p->lateral_range = 10.0; p->longitudinal_spacing = 1.5; p->lateral_spacing = 0.6; p->car_width = 2.0;      // planning_flags.cpp:38-42,10
}

static bool dp_ok(pqp_handle* h, int batch, int m, int max_layers, const double* spline, const double* spline_ext, const double* length, const double* start,
                  const float* dist, const pqp_grid_geometry* geom, const pqp_dp_params* prm, const double* layers_s, const double* lb, const double* ub,
                  const int32_t* count, const double* vehicle_l) {
    return h && spline && spline_ext && length && start && dist && prm && layers_s && lb && ub && count && vehicle_l && batch >= 1 && m >= 3 &&
           max_layers >= 2 && geometry_ok(geom) && prm->lateral_spacing > 0.0 && prm->longitudinal_spacing > 0.0 &&
           !(2.0 * prm->lateral_range / prm->lateral_spacing + 1.0 > 64.0);
}

int pqp_dp_corridor_device(pqp_handle* h, int batch, int m, int max_layers, const double* spline, const double* spline_ext,
                           const double* length, const double* start, const float* dist, const int32_t* map_of,
                           const pqp_grid_geometry* geom, const pqp_dp_params* prm, double* layers_s, double* lb, double* ub,
                           int32_t* count, double* vehicle_l) {
    if (!dp_ok(h, batch, m, max_layers, spline, spline_ext, length, start, dist, geom, prm, layers_s, lb, ub, count, vehicle_l))
        return fail(PQP_ERR_INVALID, "pqp_dp_corridor: bad argument (at most 64 lateral samples per layer)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::DpArgs a;
    a.batch = batch; a.m = m; a.max_layers = max_layers; a.spl = spline; a.spl_ext = spline_ext; a.length = length; a.start = start;
    a.dist = dist; a.map_of = map_of; a.g = *geom; a.p = *prm; a.layers_s = layers_s; a.lb = lb; a.ub = ub; a.count = count; a.vehicle_l = vehicle_l;
    const int nlat = pqp::dp_lateral_samples(prm->lateral_range, prm->lateral_spacing);
    const size_t lds = pqp::DpBlock<true, true>{m, max_layers, nlat}.total_bytes();
    const size_t lds_long = pqp::DpBlock<false, true>{m, max_layers, nlat}.total_bytes();
    return line_launch(h, (const void*)pqp::dp_corridor_kernel, lds, "pqp_dp_corridor: 9 m + 17 max_layers doubles (+ the edge table) exceed one CU's LDS",
                       (size_t)batch * pqp::DpBlock<true, false>{m, max_layers, nlat}.doubles() * 8, [&](auto go_long, double* ws) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_dp_kernel, dim3(batch), dim3(pqp::kDpThreads), lds_long, h->stream, a, ws);
        else hipLaunchKernelGGL(pqp::dp_corridor_kernel, dim3(batch), dim3(pqp::kDpThreads), lds, h->stream, a);
    }, (const void*)pqp::long_dp_kernel, lds_long, "pqp_dp_corridor: the long form's cost tables exceed one CU's LDS");
}

int pqp_dp_corridor(pqp_handle* h, int batch, int m, int max_layers, const double* spline, const double* spline_ext, const double* length,
                    const double* start, const float* dist, int n_maps, const int32_t* map_of, const pqp_grid_geometry* geom,
                    const pqp_dp_params* prm, double* layers_s, double* lb, double* ub, int32_t* count, double* vehicle_l) {
    if (!dp_ok(h, batch, m, max_layers, spline, spline_ext, length, start, dist, geom, prm, layers_s, lb, ub, count, vehicle_l) || n_maps < 1)
        return fail(PQP_ERR_INVALID, "pqp_dp_corridor: bad argument");
    const size_t bl = (size_t)batch * max_layers;
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4);
    const double *d_length = st.in(length, batch), *d_start = st.in(start, (size_t)batch * 3);
    const float* d_dist = st.in(dist, (size_t)n_maps * geom->rows * geom->cols);
    const int32_t* d_map_of = st.in(map_of, batch);
    double *d_ls = st.out(layers_s, bl, 0), *d_lb = st.out(lb, bl, 0), *d_ub = st.out(ub, bl, 0);
    int32_t* d_count = st.out(count, batch);
    double* d_vl = st.out(vehicle_l, batch);
    return st.run([&]() -> int {
        return pqp_dp_corridor_device(h, batch, m, max_layers, d_spl, d_ext, d_length, d_start, d_dist, d_map_of, geom, prm, d_ls, d_lb, d_ub, d_count, d_vl);
    });
}

}  // extern "C"
