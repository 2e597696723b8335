// pqp_maps.hip — the entry points of include/pqp.h around the obstacle distance map and the planned paths: the distance layer from an
// occupancy grid (pqp_distance_kernels.inc), vehicle footprints against it (pqp_footprint_kernels.inc), scores of candidate paths and each
// group's best (pqp_select_kernels.inc), speed profiles along them (pqp_speed_kernels.inc), samples of those trajectories on a time grid
// (pqp_sample_kernels.inc), those samples against predicted moving agents (pqp_agents_kernels.inc), standing agents laid over the distance
// layers (pqp_overlay_kernels.inc), those agents' rows from their tracks
// (pqp_predict_kernels.inc), speeds that pass those agents in
// the path-time plane (pqp_search_kernels.inc), the speed QP that makes such a plan drivable (pqp_refine_kernels.inc; its solve is the
// banded core's, launched from pqp_smoothers.hip), those plans on a fine time step (pqp_plan_kernels.inc), scores of the finished
// trajectories and each group's best (pqp_rank_kernels.inc).  Their kernels, launchers and entry points.
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
#include "pqp_driven_path.hpp"
#include "pqp_line_device.hpp"
#include "pqp_internal.hpp"

using namespace pqp_internal;

#include "pqp_distance_kernels.inc"
#include "pqp_footprint_kernels.inc"
#include "pqp_select_kernels.inc"
#include "pqp_speed_kernels.inc"
#include "pqp_sample_kernels.inc"
#include "pqp_agents_kernels.inc"
#include "pqp_overlay_kernels.inc"
#include "pqp_predict_kernels.inc"
#include "pqp_search_kernels.inc"
#include "pqp_refine_kernels.inc"
#include "pqp_plan_kernels.inc"
#include "pqp_rank_kernels.inc"

// ---- what the entry points below share ------------------------------------------------------------------------------------------------
// the grid of a kernel that gives every item a wavefront, threads / 64 of them to a workgroup
static dim3 wave_grid(long long items, int threads) {
    const int per_block = threads / 64;
    return dim3((unsigned)((items + per_block - 1) / per_block));
}

// an optional index array of a host form: every entry inside [0, count), or the refusal `what`
static int index_range(const int32_t* of, int batch, int count, const char* what) {
    if (of)
        for (int b = 0; b < batch; ++b)
            if (of[b] < 0 || of[b] >= count) return fail(PQP_ERR_INVALID, what);
    return PQP_OK;
}

// the car's circles as the kernels take them
static int car_circles_of(const pqp_car_geometry* car, pqp::CarCircles* c) {
    double circles[7][3];
    if (const int rc = pqp_car_circles(car, &circles[0][0])) return rc;
    for (int k = 0; k < 7; ++k) { c->cx[k] = circles[k][0]; c->cy[k] = circles[k][1]; c->cr[k] = circles[k][2]; }
    // the reference's own bounding circle (circles[6][2]) does not contain the corner circles: the broad phase takes the radius that does
    c->rb = 0.0;
    for (int k = 0; k < 6; ++k) c->rb = std::max(c->rb, std::hypot(c->cx[k] - c->cx[6], c->cy[k] - c->cy[6]) + c->cr[k]);
    return PQP_OK;
}

// agent_frames_kernel over every (scene, agent, step) row, inside a launch_timed
static int launch_agent_frames(pqp_handle* h, int n_scenes, int a_max, int m, const double* agents, double* frames) {
    const pqp::AgentFramesArgs fa = {(long long)n_scenes * a_max * m, agents, frames};
    if (fa.rows == 0) return PQP_OK;
    hipLaunchKernelGGL(pqp::agent_frames_kernel, dim3((unsigned)((fa.rows + pqp::kAgentsThreads - 1) / pqp::kAgentsThreads)),
                       dim3(pqp::kAgentsThreads), 0, h->stream, fa);
    PQP_HIP(hipGetLastError());
    return PQP_OK;
}

extern "C" {

// ---- the obstacle distance layer from an occupancy grid (src/test/demo.cpp:104-113) ------------------------------------------------
static bool distance_layer_ok(pqp_handle* h, int n_maps, const pqp_grid_geometry* geom, const uint8_t* grid, const float* dist) {
    return h && grid && dist && n_maps >= 1 && geometry_ok(geom);
}

int pqp_distance_layer_device(pqp_handle* h, int n_maps, const pqp_grid_geometry* geom, const uint8_t* grid, float* dist) {
    if (!distance_layer_ok(h, n_maps, geom, grid, dist))
        return fail(PQP_ERR_INVALID, "pqp_distance_layer: bad argument (n_maps >= 1; a map of 2 x 2 to 2^30 cells, resolution > 0)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::DistanceArgs a;
    a.grid = grid; a.out = reinterpret_cast<int32_t*>(dist); a.n_maps = n_maps; a.rows = geom->rows; a.cols = geom->cols;
    const pqp::edt::Shape sh = pqp::edt::shape_of(geom->rows, geom->cols);
    a.site_bits = sh.site_bits; a.empty_d2 = sh.empty_d2; a.res = (float)geom->resolution;
    const long long lines = (long long)n_maps * geom->cols, lanes = (long long)n_maps * geom->rows;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::distance_lines_kernel, dim3((unsigned)std::min((lines + 3) / 4, 1ll << 20)), dim3(256), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        const unsigned blocks = (unsigned)std::min((lanes + 63) / 64, 1ll << 20);
        if (sh.wide) hipLaunchKernelGGL(pqp::distance_envelope_kernel<int64_t>, dim3(blocks), dim3(64), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::distance_envelope_kernel<int32_t>, dim3(blocks), dim3(64), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_distance_layer(pqp_handle* h, int n_maps, const pqp_grid_geometry* geom, const uint8_t* grid, float* dist) {
    if (!distance_layer_ok(h, n_maps, geom, grid, dist))
        return fail(PQP_ERR_INVALID, "pqp_distance_layer: bad argument (n_maps >= 1; a map of 2 x 2 to 2^30 cells, resolution > 0)");
    const size_t cells = (size_t)n_maps * geom->rows * geom->cols;
    Staging st(h);
    const uint8_t* d_grid = st.in(grid, cells);
    float* d_dist = st.out(dist, cells);
    return st.run([&]() -> int { return pqp_distance_layer_device(h, n_maps, geom, d_grid, d_dist); });
}

// ---- vehicle footprints against the distance layer (collision_checker.cpp:17-58, car_geometry.cpp:38-72) ----------------------------
void pqp_car_default_geometry(pqp_car_geometry* c) {
    if (!c) return;
    c->width = 2.0;                 // planning_flags.cpp:10
    c->rear_length = -1.0;          // :18
    c->front_length = 3.9;          // :20
}

static bool car_ok(const pqp_car_geometry* c) {
    return c && std::isfinite(c->width) && std::isfinite(c->rear_length) && std::isfinite(c->front_length);
}

int pqp_car_circles(const pqp_car_geometry* c, double* circles) {
    if (!car_ok(c) || !circles) return fail(PQP_ERR_INVALID, "pqp_car_circles: bad argument (a finite car geometry)");
    // CollisionChecker's car_(FLAGS_car_width, fabs(FLAGS_rear_length), FLAGS_front_length) -> CarGeometry(width, back_length, front_length)
    const double width = c->width, back_length = std::fabs(c->rear_length), front_length = c->front_length;
    const double length = front_length + back_length;
    const double fl_x = front_length, fl_y = width / 2.0, fr_x = front_length, fr_y = -width / 2.0;
    const double rl_x = -back_length, rl_y = width / 2.0, rr_x = -back_length, rr_y = -width / 2.0;
    // CarGeometry::setCircles, car_geometry.cpp:38-57, term by term
    const double bounding_x = (front_length - back_length) / 2.0;
    const double bounding_r = std::sqrt(std::pow(length / 2, 2) + std::pow(width / 2, 2));
    const double small_circle_shift = width / 4.0;
    const double small_circle_radius = std::sqrt(2 * std::pow(small_circle_shift, 2));
    const double large_circle_radius = std::sqrt(std::pow(width, 2) + std::pow((length - width) / 2.0, 2)) / 2;
    const double v[7][3] = {{rr_x + small_circle_shift, rr_y + small_circle_shift, small_circle_radius},
                            {rl_x + small_circle_shift, rl_y - small_circle_shift, small_circle_radius},
                            {fr_x - small_circle_shift, fr_y + small_circle_shift, small_circle_radius},
                            {fl_x - small_circle_shift, fl_y - small_circle_shift, small_circle_radius},
                            {bounding_x + (length - width) / 4, 0, large_circle_radius},
                            {bounding_x - (length - width) / 4, 0, large_circle_radius},
                            {bounding_x, 0, bounding_r}};
    std::memcpy(circles, v, sizeof(v));
    return PQP_OK;
}

static bool footprint_ok(pqp_handle* h, int batch, int n, int stride, const double* states, const float* dist, const pqp_grid_geometry* geom,
                         const pqp_car_geometry* car, int mode, const uint8_t* free_out, const int32_t* first_collision) {
    return h && states && dist && free_out && first_collision && batch >= 1 && n >= 1 && n <= (1 << 30) && stride >= 3 && geometry_ok(geom) &&
           car_ok(car) && (mode == PQP_FOOTPRINT_CIRCLES || mode == PQP_FOOTPRINT_BOUNDING_FIRST);
}

int pqp_footprint_check_device(pqp_handle* h, int batch, int n, int stride, const double* states, const int32_t* n_of, const float* dist,
                               const int32_t* map_of, const pqp_grid_geometry* geom, const pqp_car_geometry* car, int mode, uint8_t* free_out,
                               int32_t* first_collision, double* margin) {
    if (!footprint_ok(h, batch, n, stride, states, dist, geom, car, mode, free_out, first_collision))
        return fail(PQP_ERR_INVALID, "pqp_footprint_check: bad argument (stride >= 3; a finite car geometry; mode CIRCLES or BOUNDING_FIRST; "
                                     "a map layer of 2 x 2 to 2^30 cells)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::FootprintArgs a;
    if (const int rc = car_circles_of(car, &a.car)) return rc;
    a.batch = batch; a.n = n; a.stride = stride; a.states = states; a.n_of = n_of; a.dist = dist; a.map_of = map_of; a.g = *geom;
    a.free_out = free_out; a.first_collision = first_collision; a.margin = margin;
    return h->launch_timed([&]() -> int {
        if (mode == PQP_FOOTPRINT_CIRCLES)
            hipLaunchKernelGGL(pqp::footprint_check_kernel<PQP_FOOTPRINT_CIRCLES>, dim3(batch), dim3(pqp::kFootprintThreads), 0, h->stream, a);
        else
            hipLaunchKernelGGL(pqp::footprint_check_kernel<PQP_FOOTPRINT_BOUNDING_FIRST>, dim3(batch), dim3(pqp::kFootprintThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_footprint_check(pqp_handle* h, int batch, int n, int stride, const double* states, const int32_t* n_of, const float* dist, int n_maps,
                        const int32_t* map_of, const pqp_grid_geometry* geom, const pqp_car_geometry* car, int mode, uint8_t* free_out,
                        int32_t* first_collision, double* margin) {
    if (!footprint_ok(h, batch, n, stride, states, dist, geom, car, mode, free_out, first_collision) || n_maps < 1)
        return fail(PQP_ERR_INVALID, "pqp_footprint_check: bad argument");
    if (const int rc = index_range(map_of, batch, n_maps, "pqp_footprint_check: map_of outside [0, n_maps)")) return rc;
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_states = st.in(states, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const float* d_dist = st.in(dist, (size_t)n_maps * geom->rows * geom->cols);
    const int32_t* d_map_of = st.in(map_of, batch);
    uint8_t* d_free = st.out(free_out, bn);
    int32_t* d_first = st.out(first_collision, batch);
    double* d_margin = margin ? st.out(margin, bn) : nullptr;
    return st.run([&]() -> int {
        return pqp_footprint_check_device(h, batch, n, stride, d_states, d_n_of, d_dist, d_map_of, geom, car, mode, d_free, d_first, d_margin);
    });
}

// ---- scores of candidate paths and each group's best ----------------------------------------------------------------------------------
void pqp_select_default_params(pqp_select_params* p) {
    if (!p) return;
    pqp_params d;
    pqp::default_params(&d);
    p->weight_kappa = d.weight_kappa;          // base_solver.cpp:124
    p->weight_dkappa = d.weight_dkappa;        // :125
    p->weight_offset = 0.0;                    // :123: weight_l is 0
    p->weight_length = 0.0;
    p->weight_clearance = 0.0;
    p->clearance_want = d.expected_safety_margin;      // FLAGS_expected_safety_margin, planning_flags.cpp:95
    p->per_waypoint = 0;
    p->require_free = 1;
}

static bool select_ok(pqp_handle* h, const pqp_select_params* prm, int batch, int n, int stride, const double* paths, int groups,
                      const int32_t* group_start, const double* terms, const int32_t* best, const double* best_paths, const int32_t* best_n) {
    return h && prm && paths && group_start && terms && best && batch >= 1 && n >= 1 && n <= (1 << 30) && stride >= 7 && groups >= 0 &&
           (best_paths != nullptr) == (best_n != nullptr);
}

int pqp_select_paths_device(pqp_handle* h, const pqp_select_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                            const int32_t* status, const int32_t* stage, const int32_t* first_collision, const double* margin, int groups,
                            const int32_t* group_start, double* terms, int32_t* best, double* best_paths, int32_t* best_n) {
    if (!select_ok(h, prm, batch, n, stride, paths, groups, group_start, terms, best, best_paths, best_n))
        return fail(PQP_ERR_INVALID, "pqp_select_paths: bad argument (stride >= 7; groups >= 0; best_paths and best_n both or neither)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::SelectArgs a;
    a.batch = batch; a.n = n; a.stride = stride; a.groups = groups; a.paths = paths; a.n_of = n_of; a.status = status; a.stage = stage;
    a.first_collision = first_collision; a.margin = margin; a.group_start = group_start; a.prm = *prm; a.terms = terms; a.best = best;
    a.best_paths = best_paths; a.best_n = best_n;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::path_score_kernel, wave_grid(batch, pqp::kSelectThreads), dim3(pqp::kSelectThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        if (groups > 0) {
            hipLaunchKernelGGL(pqp::group_select_kernel, wave_grid(groups, pqp::kSelectThreads), dim3(pqp::kSelectThreads), 0, h->stream, a);
            PQP_HIP(hipGetLastError());
        }
        return PQP_OK;
    });
}

int pqp_select_paths(pqp_handle* h, const pqp_select_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                     const int32_t* status, const int32_t* stage, const int32_t* first_collision, const double* margin, int groups,
                     const int32_t* group_start, double* terms, int32_t* best, double* best_paths, int32_t* best_n) {
    if (!select_ok(h, prm, batch, n, stride, paths, groups, group_start, terms, best, best_paths, best_n))
        return fail(PQP_ERR_INVALID, "pqp_select_paths: bad argument (stride >= 7; groups >= 0; best_paths and best_n both or neither)");
    for (const double v : {prm->weight_kappa, prm->weight_dkappa, prm->weight_offset, prm->weight_length, prm->weight_clearance, prm->clearance_want})
        if (!std::isfinite(v)) return fail(PQP_ERR_INVALID, "pqp_select_paths: a parameter that is not finite");
    if (group_start[0] != 0 || group_start[groups] != batch) return fail(PQP_ERR_INVALID, "pqp_select_paths: group_start must run from 0 to batch");
    for (int g = 0; g < groups; ++g)
        if (group_start[g + 1] < group_start[g]) return fail(PQP_ERR_INVALID, "pqp_select_paths: group_start must be ascending");
    // (from here on groups >= 1: group_start runs from 0 to batch >= 1)
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_status = st.in(status, batch);
    const int32_t* d_stage = st.in(stage, batch);
    const int32_t* d_first = st.in(first_collision, batch);
    const double* d_margin = st.in(margin, bn);
    const int32_t* d_start = st.in(group_start, (size_t)groups + 1);
    double* d_terms = st.out(terms, (size_t)batch * PQP_SCORE_STRIDE);
    int32_t* d_best = st.out(best, groups);
    double* d_best_paths = best_paths ? st.out(best_paths, (size_t)groups * n * 7) : nullptr;
    int32_t* d_best_n = best_n ? st.out(best_n, groups) : nullptr;
    return st.run([&]() -> int {
        return pqp_select_paths_device(h, prm, batch, n, stride, d_paths, d_n_of, d_status, d_stage, d_first, d_margin, groups, d_start, d_terms,
                                       d_best, d_best_paths, d_best_n);
    });
}

// ---- planned paths to trajectories: s, v, a, t ---------------------------------------------------------------------------------------------
void pqp_speed_default_params(pqp_speed_params* p) {
    if (!p) return;
    // this library's choice: the reference plans geometry only and has no such flags
    p->v_max = 10.0;
    p->a_max = 1.5;
    p->d_max = 3.0;
    p->a_lat_max = 2.0;
}

static const char* const kSpeedRefusal =
    "pqp_speed_profile: bad argument (batch >= 1; n >= 1; stride >= 6; v_max finite and >= 0; a_max and d_max finite and > 0; a_lat_max > 0)";

static bool speed_ok(pqp_handle* h, const pqp_speed_params* prm, int batch, int n, int stride, const double* paths, const double* v_start,
                     const double* profile, const int32_t* flags) {
    return h && prm && paths && v_start && profile && flags && batch >= 1 && n >= 1 && stride >= 6 && std::isfinite(prm->v_max) &&
           prm->v_max >= 0.0 && std::isfinite(prm->a_max) && prm->a_max > 0.0 && std::isfinite(prm->d_max) && prm->d_max > 0.0 &&
           prm->a_lat_max > 0.0;
}

int pqp_speed_profile_device(pqp_handle* h, const pqp_speed_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                             const int32_t* stop_before, const double* v_limit, const double* v_start, const double* v_end, double* profile,
                             int32_t* flags) {
    if (!speed_ok(h, prm, batch, n, stride, paths, v_start, profile, flags)) return fail(PQP_ERR_INVALID, kSpeedRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::SpeedArgs a;
    a.batch = batch; a.n = n; a.stride = stride; a.paths = paths; a.n_of = n_of; a.stop_before = stop_before; a.v_limit = v_limit;
    a.v_start = v_start; a.v_end = v_end; a.prm = *prm; a.profile = profile; a.flags = flags;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::speed_profile_kernel, wave_grid(batch, pqp::kSpeedThreads), dim3(pqp::kSpeedThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_speed_profile(pqp_handle* h, const pqp_speed_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                      const int32_t* stop_before, const double* v_limit, const double* v_start, const double* v_end, double* profile,
                      int32_t* flags) {
    if (!speed_ok(h, prm, batch, n, stride, paths, v_start, profile, flags)) return fail(PQP_ERR_INVALID, kSpeedRefusal);
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_stop = st.in(stop_before, batch);
    const double* d_limit = st.in(v_limit, bn);
    const double* d_start = st.in(v_start, batch);
    const double* d_end = st.in(v_end, batch);
    double* d_profile = st.out(profile, bn * PQP_SPEED_STRIDE);
    int32_t* d_flags = st.out(flags, batch);
    return st.run([&]() -> int {
        return pqp_speed_profile_device(h, prm, batch, n, stride, d_paths, d_n_of, d_stop, d_limit, d_start, d_end, d_profile, d_flags);
    });
}

// ---- time-stamped trajectories at a fixed time step ------------------------------------------------------------------------------------------
void pqp_sample_default_params(pqp_sample_params* p) {
    if (!p) return;
    // this library's choice, as pqp_speed_default_params: the reference has no time axis
    p->dt = 0.1;
    p->hold_last = 0;
}

static const char* const kSampleRefusal =
    "pqp_sample_trajectory: bad argument (batch >= 1; n >= 1; m >= 1; stride >= 6; dt finite and > 0; hold_last 0 or 1)";

static bool sample_ok(pqp_handle* h, const pqp_sample_params* prm, int batch, int n, int stride, const double* paths, const double* profile, int m,
                      const double* traj, const int32_t* m_of, const int32_t* flags) {
    return h && prm && paths && profile && traj && m_of && flags && batch >= 1 && n >= 1 && m >= 1 && stride >= 6 && std::isfinite(prm->dt) &&
           prm->dt > 0.0 && (prm->hold_last == 0 || prm->hold_last == 1);
}

int pqp_sample_trajectory_device(pqp_handle* h, const pqp_sample_params* prm, int batch, int n, int stride, const double* paths,
                                 const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* t0, int m, double* traj,
                                 int32_t* m_of, int32_t* flags) {
    if (!sample_ok(h, prm, batch, n, stride, paths, profile, m, traj, m_of, flags)) return fail(PQP_ERR_INVALID, kSampleRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::SampleArgs a;
    a.batch = batch; a.n = n; a.stride = stride; a.m = m; a.paths = paths; a.n_of = n_of; a.stop_before = stop_before; a.profile = profile;
    a.t0 = t0; a.prm = *prm; a.traj = traj; a.m_of = m_of; a.flags = flags;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::sample_trajectory_kernel, wave_grid(batch, pqp::kSampleThreads), dim3(pqp::kSampleThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_sample_trajectory(pqp_handle* h, const pqp_sample_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                          const int32_t* stop_before, const double* profile, const double* t0, int m, double* traj, int32_t* m_of,
                          int32_t* flags) {
    if (!sample_ok(h, prm, batch, n, stride, paths, profile, m, traj, m_of, flags)) return fail(PQP_ERR_INVALID, kSampleRefusal);
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_stop = st.in(stop_before, batch);
    const double* d_profile = st.in(profile, bn * PQP_SPEED_STRIDE);
    const double* d_t0 = st.in(t0, batch);
    double* d_traj = st.out(traj, (size_t)batch * m * PQP_TRAJ_STRIDE);
    int32_t* d_m_of = st.out(m_of, batch);
    int32_t* d_flags = st.out(flags, batch);
    return st.run([&]() -> int {
        return pqp_sample_trajectory_device(h, prm, batch, n, stride, d_paths, d_n_of, d_stop, d_profile, d_t0, m, d_traj, d_m_of, d_flags);
    });
}

// ---- sampled trajectories against predicted moving agents -------------------------------------------------------------------------------------
void pqp_agents_default_params(double* margin) {
    if (!margin) return;
    *margin = 0.0;                  // touching is no hit; this library's choice, the reference has no moving obstacles
}

static const char* const kAgentsRefusal =
    "pqp_agents_check: bad argument (batch >= 1; m >= 1; stride >= 3; n_scenes >= 1; a_max >= 0; n_scenes * a_max * m <= 2^38; margin finite and >= 0; "
    "a finite car geometry)";

static bool agents_ok(pqp_handle* h, double margin, const pqp_car_geometry* car, int batch, int m, int stride, const double* traj,
                      int n_scenes, int a_max, const double* agents, const int32_t* first_hit, const int32_t* hit_agent) {
    // (the frames' launch is one block per 256 rows in x: 2^38 rows are 2^30 blocks, and 16 TiB of frames)
    return h && traj && first_hit && hit_agent && batch >= 1 && m >= 1 && stride >= 3 && n_scenes >= 1 && a_max >= 0 &&
           (long long)n_scenes * a_max <= (1ll << 38) / m && (agents || a_max == 0) && std::isfinite(margin) && margin >= 0.0 && car_ok(car);
}

int pqp_agents_check_device(pqp_handle* h, double margin, const pqp_car_geometry* car, int batch, int m, int stride,
                            const double* traj, const int32_t* m_of, int n_scenes, int a_max, const double* agents, const int32_t* a_of,
                            const int32_t* scene_of, double* frames, int32_t* first_hit, int32_t* hit_agent, double* clearance) {
    if (!agents_ok(h, margin, car, batch, m, stride, traj, n_scenes, a_max, agents, first_hit, hit_agent) || (!frames && a_max > 0))
        return fail(PQP_ERR_INVALID, kAgentsRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::AgentsArgs a;
    if (const int rc = car_circles_of(car, &a.car)) return rc;
    a.batch = batch; a.m = m; a.stride = stride; a.n_scenes = n_scenes; a.a_max = a_max; a.traj = traj; a.m_of = m_of;
    a.a_of = a_of; a.scene_of = scene_of; a.margin = margin; a.frames = frames; a.first_hit = first_hit; a.hit_agent = hit_agent;
    a.clearance = clearance;
    return h->launch_timed([&]() -> int {
        if (const int rc = launch_agent_frames(h, n_scenes, a_max, m, agents, frames)) return rc;
        const dim3 grid = wave_grid(batch, pqp::kAgentsThreads);
        if (clearance) hipLaunchKernelGGL(pqp::agents_check_kernel<true>, grid, dim3(pqp::kAgentsThreads), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::agents_check_kernel<false>, grid, dim3(pqp::kAgentsThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_agents_check(pqp_handle* h, double margin, const pqp_car_geometry* car, int batch, int m, int stride,
                     const double* traj, const int32_t* m_of, int n_scenes, int a_max, const double* agents, const int32_t* a_of,
                     const int32_t* scene_of, int32_t* first_hit, int32_t* hit_agent, double* clearance) {
    if (!agents_ok(h, margin, car, batch, m, stride, traj, n_scenes, a_max, agents, first_hit, hit_agent)) return fail(PQP_ERR_INVALID, kAgentsRefusal);
    if (const int rc = index_range(scene_of, batch, n_scenes, "pqp_agents_check: scene_of outside [0, n_scenes)")) return rc;
    const size_t bm = (size_t)batch * m, rows = (size_t)n_scenes * a_max * m;
    Staging st(h);
    const double* d_traj = st.in(traj, bm * stride);
    const int32_t* d_m_of = st.in(m_of, batch);
    const double* d_agents = rows ? st.in(agents, rows * PQP_AGENT_STRIDE) : nullptr;
    const int32_t* d_a_of = st.in(a_of, n_scenes);
    const int32_t* d_scene_of = st.in(scene_of, batch);
    double* d_frames = rows ? st.out((double*)nullptr, rows * PQP_AGENT_FRAME_STRIDE) : nullptr;
    int32_t* d_first = st.out(first_hit, batch);
    int32_t* d_who = st.out(hit_agent, batch);
    double* d_clear = clearance ? st.out(clearance, bm) : nullptr;
    return st.run([&]() -> int {
        return pqp_agents_check_device(h, margin, car, batch, m, stride, d_traj, d_m_of, n_scenes, a_max, d_agents, d_a_of, d_scene_of, d_frames,
                                       d_first, d_who, d_clear);
    });
}

// ---- tracked agents to predicted rows, on the layers' steps and on fine steps -----------------------------------------------------------------
void pqp_predict_default_params(double* prm) {
    if (!prm) return;
    // this library's choice: the reference has no moving obstacles
    prm[PQP_PREDICT_V_CAP] = 40.0;
    prm[PQP_PREDICT_GROW] = 0.0;
    prm[PQP_PREDICT_L_MAX] = 3.0;
}

static const char* const kPredictRefusal =
    "pqp_predict_agents: bad argument (n_scenes >= 1; a_max >= 0; m >= 1; r >= 1; (m - 1) * r + 1 <= INT_MAX; n_scenes * a_max * ((m - 1) * r + 1) <= "
    "2^38; t0 finite and >= 0; dt finite and > 0; v_cap, grow and l_max finite and >= 0; n_lanes >= 0; with n_lanes > 0 lane_m >= 2 and the three "
    "lane arrays)";

static bool predict_ok(pqp_handle* h, const double* prm, double t0, double dt, int m, int r, int n_scenes, int a_max, const double* tracks,
                       int n_lanes, int lane_m, const double* lane_spline, const double* lane_ext, const double* lane_length, const double* agents,
                       const int32_t* flags) {
    if (!(h && prm && n_scenes >= 1 && a_max >= 0 && m >= 1 && r >= 1 && n_lanes >= 0)) return false;
    const long long M = (long long)(m - 1) * r + 1;
    if (M > INT_MAX || (long long)n_scenes * a_max > (1ll << 38) / M) return false;
    if (a_max > 0 && !(tracks && agents && flags)) return false;
    if (!(std::isfinite(t0) && t0 >= 0.0 && std::isfinite(dt) && dt > 0.0)) return false;
    for (int k = 0; k < PQP_PREDICT_PARAMS; ++k)
        if (!(std::isfinite(prm[k]) && prm[k] >= 0.0)) return false;
    return n_lanes == 0 || (lane_m >= 2 && lane_spline && lane_ext && lane_length);
}

int pqp_predict_agents_device(pqp_handle* h, const double* prm, double t0, double dt, int m, int r, int n_scenes, int a_max, const double* tracks,
                              const int32_t* a_of, const int32_t* lane_of, int n_lanes, int lane_m, const double* lane_spline,
                              const double* lane_ext, const double* lane_length, double* agents, double* anchor, int32_t* flags) {
    if (!predict_ok(h, prm, t0, dt, m, r, n_scenes, a_max, tracks, n_lanes, lane_m, lane_spline, lane_ext, lane_length, agents, flags))
        return fail(PQP_ERR_INVALID, kPredictRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::PredictArgs a;
    a.n_scenes = n_scenes; a.a_max = a_max; a.m = m; a.r = r; a.n_lanes = n_lanes; a.lane_m = lane_m; a.t0 = t0; a.dt = dt;
    a.v_cap = prm[PQP_PREDICT_V_CAP]; a.grow = prm[PQP_PREDICT_GROW]; a.l_max = prm[PQP_PREDICT_L_MAX];
    a.tracks = tracks; a.a_of = a_of; a.lane_of = lane_of; a.lane_spl = lane_spline; a.lane_ext = lane_ext; a.lane_len = lane_length;
    a.agents = agents; a.anchor = anchor; a.flags = flags;
    const long long slots = (long long)n_scenes * a_max;
    return h->launch_timed([&]() -> int {
        if (slots == 0) return PQP_OK;
        const long long blocks = (slots + pqp::kPredictThreads / 64 - 1) / (pqp::kPredictThreads / 64);
        hipLaunchKernelGGL(pqp::predict_agents_kernel, dim3((unsigned)std::min(blocks, pqp::kPredictMaxBlocks)), dim3(pqp::kPredictThreads), 0,
                           h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_predict_agents(pqp_handle* h, const double* prm, double t0, double dt, int m, int r, int n_scenes, int a_max, const double* tracks,
                       const int32_t* a_of, const int32_t* lane_of, int n_lanes, int lane_m, const double* lane_spline, const double* lane_ext,
                       const double* lane_length, double* agents, double* anchor, int32_t* flags) {
    if (!predict_ok(h, prm, t0, dt, m, r, n_scenes, a_max, tracks, n_lanes, lane_m, lane_spline, lane_ext, lane_length, agents, flags))
        return fail(PQP_ERR_INVALID, kPredictRefusal);
    const size_t slots = (size_t)n_scenes * a_max, M = (size_t)(m - 1) * r + 1;
    if (lane_of)
        for (size_t k = 0; k < slots; ++k)
            if (lane_of[k] >= n_lanes) return fail(PQP_ERR_INVALID, "pqp_predict_agents: lane_of at or above n_lanes");
    if (slots == 0) return PQP_OK;
    Staging st(h);
    const double* d_tracks = st.in(tracks, slots * PQP_TRACK_STRIDE);
    const int32_t* d_a_of = st.in(a_of, n_scenes);
    const int32_t* d_lane_of = st.in(lane_of, slots);
    const double* d_spl = n_lanes ? st.in(lane_spline, (size_t)n_lanes * 9 * lane_m) : nullptr;
    const double* d_ext = n_lanes ? st.in(lane_ext, (size_t)n_lanes * 4) : nullptr;
    const double* d_len = n_lanes ? st.in(lane_length, n_lanes) : nullptr;
    double* d_agents = st.out(agents, slots * M * PQP_AGENT_STRIDE);
    double* d_anchor = anchor ? st.out(anchor, slots * PQP_ANCHOR_STRIDE) : nullptr;
    int32_t* d_flags = st.out(flags, slots);
    return st.run([&]() -> int {
        return pqp_predict_agents_device(h, prm, t0, dt, m, r, n_scenes, a_max, d_tracks, d_a_of, d_lane_of, n_lanes, lane_m, d_spl, d_ext, d_len,
                                         d_agents, d_anchor, d_flags);
    });
}

// ---- standing agents laid over the distance layers, one layer per scene ---------------------------------------------------------------------
void pqp_overlay_default_params(double* inflate) {
    if (!inflate) return;
    *inflate = 0.0;                 // the corridor and the footprint check add the car's circles and the safety margin themselves
}

static const char* const kOverlayRefusal =
    "pqp_overlay_agents: bad argument (n_maps >= 1; n_scenes >= 1; a_max >= 0; a finite map geometry of 2 x 2 to 2^30 cells, resolution > 0; "
    "n_scenes * rows * cols <= 2^38; inflate finite and >= 0; base_of = NULL needs n_maps = 1 or n_scenes = n_maps; dist_out = dist needs "
    "base_of = NULL and n_scenes = n_maps)";

static bool overlay_ok(pqp_handle* h, double inflate, int n_maps, const pqp_grid_geometry* geom, const float* dist, int n_scenes, int a_max,
                       const double* agents, const int32_t* base_of, const float* dist_out, const int32_t* flags) {
    if (!(h && dist && dist_out && flags && n_maps >= 1 && n_scenes >= 1 && a_max >= 0 && (agents || a_max == 0) && geometry_ok(geom))) return false;
    if (!(std::isfinite(geom->resolution) && std::isfinite(geom->length_x) && std::isfinite(geom->length_y) && std::isfinite(geom->pos_x) &&
          std::isfinite(geom->pos_y) && std::isfinite(inflate) && inflate >= 0.0))
        return false;
    if ((long long)n_scenes > (1ll << 38) / ((long long)geom->rows * geom->cols)) return false;
    const bool own_layer = !base_of && n_scenes == n_maps;               // every scene reads the layer of its own index alone
    if (!base_of && n_maps != 1 && !own_layer) return false;
    return dist_out != dist || own_layer;
}

int pqp_overlay_agents_device(pqp_handle* h, double inflate, int n_maps, const pqp_grid_geometry* geom, const float* dist, int n_scenes,
                              int a_max, const double* agents, const int32_t* a_of, const int32_t* base_of, double* frames, float* dist_out,
                              int32_t* flags) {
    if (!overlay_ok(h, inflate, n_maps, geom, dist, n_scenes, a_max, agents, base_of, dist_out, flags) || (!frames && a_max > 0))
        return fail(PQP_ERR_INVALID, kOverlayRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::OverlayArgs a;
    a.n_maps = n_maps; a.n_scenes = n_scenes; a.a_max = a_max; a.g = *geom; a.inflate = inflate; a.dist = dist; a.a_of = a_of;
    a.base_of = base_of; a.frames = frames; a.out = dist_out; a.flags = flags;
    a.tiles_i = ((unsigned)geom->rows + 63) / 64;
    a.tiles_j = ((unsigned)geom->cols + pqp::kOverlayCols - 1) / pqp::kOverlayCols;
    // (rows * cols < 2^30: at most 2^26 tiles of a scene; the scenes go over y and z, 65535 to a row)
    a.scenes_y = (unsigned)std::min(n_scenes, 65535);
    const unsigned per_block = pqp::kOverlayThreads / 64;
    const dim3 grid((a.tiles_i * a.tiles_j + per_block - 1) / per_block, a.scenes_y, ((unsigned)n_scenes + a.scenes_y - 1) / a.scenes_y);
    return h->launch_timed([&]() -> int {
        if (const int rc = launch_agent_frames(h, n_scenes, a_max, 1, agents, frames)) return rc;
        hipLaunchKernelGGL(pqp::overlay_kernel, grid, dim3(pqp::kOverlayThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_overlay_agents(pqp_handle* h, double inflate, int n_maps, const pqp_grid_geometry* geom, const float* dist, int n_scenes, int a_max,
                       const double* agents, const int32_t* a_of, const int32_t* base_of, float* dist_out, int32_t* flags) {
    if (!overlay_ok(h, inflate, n_maps, geom, dist, n_scenes, a_max, agents, base_of, dist_out, flags)) return fail(PQP_ERR_INVALID, kOverlayRefusal);
    if (const int rc = index_range(base_of, n_scenes, n_maps, "pqp_overlay_agents: base_of outside [0, n_maps)")) return rc;
    const size_t cells = (size_t)geom->rows * geom->cols, rows = (size_t)n_scenes * a_max;
    Staging st(h);
    // (dist_out = dist: the device form then runs on two arrays, and by the definition gives what it gives in place)
    const float* d_dist = st.in(dist, (size_t)n_maps * cells);
    const double* d_agents = rows ? st.in(agents, rows * PQP_AGENT_STRIDE) : nullptr;
    const int32_t* d_a_of = st.in(a_of, n_scenes);
    const int32_t* d_base_of = st.in(base_of, n_scenes);
    double* d_frames = rows ? st.out((double*)nullptr, rows * PQP_AGENT_FRAME_STRIDE) : nullptr;
    float* d_out = st.out(dist_out, (size_t)n_scenes * cells);
    int32_t* d_flags = st.out(flags, n_scenes);
    return st.run([&]() -> int {
        return pqp_overlay_agents_device(h, inflate, n_maps, geom, d_dist, n_scenes, a_max, d_agents, d_a_of, d_base_of, d_frames, d_out, d_flags);
    });
}

// ---- speeds past predicted agents: a search in the path-time plane ---------------------------------------------------------------------------
int pqp_search_params_from_speed(const pqp_speed_params* sp, double dt, double ds, pqp_search_params* p) {
    if (!sp || !p || !(std::isfinite(dt) && dt > 0.0) || !(std::isfinite(ds) && ds > 0.0))
        return fail(PQP_ERR_INVALID, "pqp_search_params_from_speed: bad argument (dt and ds finite and > 0)");
    // this library's choice, as pqp_speed_default_params: the reference has no time axis
    const double q_max = std::floor(sp->v_max * dt / ds), q_up = std::floor(sp->a_max * (dt * dt) / ds), q_down = std::floor(sp->d_max * (dt * dt) / ds);
    if (!(q_max >= 0.0 && q_max <= 63.0)) return fail(PQP_ERR_INVALID, "pqp_search_params_from_speed: floor(v_max dt / ds) outside 0 .. 63");
    p->dt = dt;
    p->ds = ds;
    p->w_slow = 1.0;
    p->w_accel = 1.0;
    p->margin = 0.0;
    p->stations = 128;
    p->q_max = (int32_t)q_max;
    p->q_up = (int32_t)std::fmin(std::fmax(q_up, 1.0), 63.0);
    p->q_down = (int32_t)std::fmin(std::fmax(q_down, 1.0), 63.0);
    return PQP_OK;
}

void pqp_search_default_params(pqp_search_params* p) {
    if (!p) return;
    pqp_speed_params sp;
    pqp_speed_default_params(&sp);
    (void)pqp_search_params_from_speed(&sp, 1.0, 0.5, p);
}

static const char* const kSearchRefusal =
    "pqp_speed_search: bad argument (batch >= 1; n >= 1; m >= 1; stride >= 6; dt and ds finite and > 0; w_slow, w_accel and margin finite and >= 0; "
    "stations >= 1; 0 <= q_max <= 63; q_up, q_down >= 0; stations * (q_max + 1) <= 4096; n_scenes >= 1; a_max >= 0; n_scenes * a_max * m <= 2^38; "
    "a finite car geometry)";

static bool search_ok(pqp_handle* h, const pqp_search_params* prm, const pqp_car_geometry* car, int batch, int n, int stride, const double* paths,
                      const double* profile, const double* v_start, int m, int n_scenes, int a_max, const double* agents, const int32_t* steps,
                      const double* traj, const double* cost, const int32_t* reached, const int32_t* flags) {
    if (!(h && prm && paths && profile && v_start && steps && traj && cost && reached && flags && batch >= 1 && n >= 1 && m >= 1 && stride >= 6))
        return false;
    const auto price = [](double v) { return std::isfinite(v) && v >= 0.0; };
    if (!(std::isfinite(prm->dt) && prm->dt > 0.0 && std::isfinite(prm->ds) && prm->ds > 0.0 && price(prm->w_slow) && price(prm->w_accel))) return false;
    if (!(prm->stations >= 1 && prm->q_max >= 0 && prm->q_max <= 63 && prm->q_up >= 0 && prm->q_down >= 0 &&
          (long long)prm->stations * (prm->q_max + 1) <= PQP_SEARCH_MAX_STATES))
        return false;
    return n_scenes >= 1 && a_max >= 0 && (long long)n_scenes * a_max <= (1ll << 38) / m && (agents || a_max == 0) && price(prm->margin) && car_ok(car);
}

int pqp_speed_search_device(pqp_handle* h, const pqp_search_params* prm, const pqp_car_geometry* car, int batch, int n, int stride,
                            const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start,
                            int m, int n_scenes, int a_max, const double* agents, const int32_t* a_of, const int32_t* scene_of, double* frames,
                            int32_t* blocked, uint8_t* parents, int32_t* steps, double* traj, double* cost, int32_t* reached, int32_t* flags) {
    if (!search_ok(h, prm, car, batch, n, stride, paths, profile, v_start, m, n_scenes, a_max, agents, steps, traj, cost, reached, flags) ||
        !blocked || !parents || (!frames && a_max > 0))
        return fail(PQP_ERR_INVALID, kSearchRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::SearchArgs a;
    if (const int rc = car_circles_of(car, &a.car)) return rc;
    a.batch = batch; a.n = n; a.stride = stride; a.m = m; a.n_scenes = n_scenes; a.a_max = a_max; a.paths = paths; a.n_of = n_of;
    a.stop_before = stop_before; a.profile = profile; a.v_start = v_start; a.a_of = a_of; a.scene_of = scene_of; a.prm = *prm; a.frames = frames;
    a.blocked = blocked; a.parents = parents; a.steps = steps; a.traj = traj; a.cost = cost; a.reached = reached; a.flags = flags;
    const long long waves = (long long)batch * ((prm->stations + 63) / 64);
    return h->launch_timed([&]() -> int {
        if (const int rc = launch_agent_frames(h, n_scenes, a_max, m, agents, frames)) return rc;
        hipLaunchKernelGGL(pqp::st_occupancy_kernel, wave_grid(waves, pqp::kAgentsThreads), dim3(pqp::kAgentsThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        hipLaunchKernelGGL(pqp::st_search_kernel, dim3((unsigned)batch), dim3(pqp::kSearchThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_speed_search(pqp_handle* h, const pqp_search_params* prm, const pqp_car_geometry* car, int batch, int n, int stride,
                     const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start, int m,
                     int n_scenes, int a_max, const double* agents, const int32_t* a_of, const int32_t* scene_of, int32_t* blocked,
                     int32_t* steps, double* traj, double* cost, int32_t* reached, int32_t* flags) {
    if (!search_ok(h, prm, car, batch, n, stride, paths, profile, v_start, m, n_scenes, a_max, agents, steps, traj, cost, reached, flags))
        return fail(PQP_ERR_INVALID, kSearchRefusal);
    if (const int rc = index_range(scene_of, batch, n_scenes, "pqp_speed_search: scene_of outside [0, n_scenes)")) return rc;
    const size_t bn = (size_t)batch * n, bm = (size_t)batch * m, rows = (size_t)n_scenes * a_max * m;
    const size_t words = (size_t)(prm->stations + 31) / 32, states = (size_t)prm->stations * (prm->q_max + 1);
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_stop = st.in(stop_before, batch);
    const double* d_profile = st.in(profile, bn * PQP_SPEED_STRIDE);
    const double* d_start = st.in(v_start, batch);
    const double* d_agents = rows ? st.in(agents, rows * PQP_AGENT_STRIDE) : nullptr;
    const int32_t* d_a_of = st.in(a_of, n_scenes);
    const int32_t* d_scene_of = st.in(scene_of, batch);
    double* d_frames = rows ? st.out((double*)nullptr, rows * PQP_AGENT_FRAME_STRIDE) : nullptr;
    int32_t* d_blocked = st.out(blocked, bm * words);
    uint8_t* d_parents = st.out((uint8_t*)nullptr, bm * states);
    int32_t* d_steps = st.out(steps, bm * 2);
    double* d_traj = st.out(traj, bm * PQP_TRAJ_STRIDE);
    double* d_cost = st.out(cost, batch);
    int32_t* d_reached = st.out(reached, batch);
    int32_t* d_flags = st.out(flags, batch);
    return st.run([&]() -> int {
        return pqp_speed_search_device(h, prm, car, batch, n, stride, d_paths, d_n_of, d_stop, d_profile, d_start, m, n_scenes, a_max, d_agents,
                                       d_a_of, d_scene_of, d_frames, d_blocked, d_parents, d_steps, d_traj, d_cost, d_reached, d_flags);
    });
}

// ---- searched speed plans made drivable: a jerk-limited speed QP ---------------------------------------------------------------------------
void pqp_refine_default_params(double* prm, int* window) {
    if (prm) {
        pqp_speed_params sp;
        pqp_speed_default_params(&sp);
        prm[PQP_REFINE_W_REF] = prm[PQP_REFINE_W_ACCEL] = prm[PQP_REFINE_W_JERK] = 1.0;
        prm[PQP_REFINE_A_MAX] = sp.a_max;
        prm[PQP_REFINE_D_MAX] = sp.d_max;
    }
    if (window) *window = 4;
}

static const char* const kRefineRefusal =
    "pqp_speed_refine: bad argument (batch >= 1; n >= 1; m >= 1; stride >= 6; dt and ds finite and > 0; 1 <= stations <= 4096; the three weights "
    "finite and >= 0, w_ref + w_accel > 0; a_max and d_max finite and > 0; window >= 0)";

static bool refine_ok(pqp_handle* h, const pqp_search_params* grid, const double* prm, int window, int batch, int n, int stride, const double* paths,
                      const double* profile, const double* v_start, int m, const int32_t* blocked, const int32_t* steps, const int32_t* reached,
                      const double* search_traj, const double* traj, const double* cost, const int32_t* status, const int32_t* iters,
                      const int32_t* flags) {
    if (!(h && grid && prm && paths && profile && v_start && blocked && steps && reached && search_traj && traj && cost && status && iters && flags &&
          batch >= 1 && n >= 1 && m >= 1 && stride >= 6 && window >= 0))
        return false;
    const auto weight = [](double v) { return std::isfinite(v) && v >= 0.0; };
    const auto limit = [](double v) { return std::isfinite(v) && v > 0.0; };
    return limit(grid->dt) && limit(grid->ds) && grid->stations >= 1 && grid->stations <= PQP_SEARCH_MAX_STATES && weight(prm[PQP_REFINE_W_REF]) &&
           weight(prm[PQP_REFINE_W_ACCEL]) && weight(prm[PQP_REFINE_W_JERK]) && prm[PQP_REFINE_W_REF] + prm[PQP_REFINE_W_ACCEL] > 0.0 &&
           limit(prm[PQP_REFINE_A_MAX]) && limit(prm[PQP_REFINE_D_MAX]);
}

// the layers the banded core holds in one CU's LDS: sm_generic_fits is monotone in m
static bool refine_fits(int m) { return m < 2 || sm_generic_fits(kBandedRefine, m); }

int pqp_speed_refine_device(pqp_handle* h, const pqp_search_params* grid, const double* prm, int window, int batch, int n, int stride,
                            const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start,
                            int m, const int32_t* blocked, const int32_t* steps, const int32_t* reached, const double* search_traj,
                            double* traj, double* bounds, double* cost, double* excess, int32_t* status, int32_t* iters, int32_t* flags) {
    if (!refine_ok(h, grid, prm, window, batch, n, stride, paths, profile, v_start, m, blocked, steps, reached, search_traj, traj, cost, status, iters, flags))
        return fail(PQP_ERR_INVALID, kRefineRefusal);
    if (!refine_fits(m)) return fail(PQP_ERR_CAPACITY, "pqp_speed_refine: the QP of m layers is beyond what the banded core holds in one CU's LDS");
    PQP_HIP(hipSetDevice(h->device));
    const bool solve = m >= 2;               // m = 1: every path is kept, there is no QP to assemble or solve
    int rc;
    if ((rc = h->rf.bounds.ensure((size_t)batch * m * 3 * 8))) return rc;
    if (solve && (rc = sm_alloc(h, h->rf, kBandedRefine, batch, m))) return rc;
    pqp::RefineArgs a;
    a.batch = batch; a.n = n; a.stride = stride; a.m = m; a.stations = grid->stations; a.window = window;
    a.dt = grid->dt; a.ds = grid->ds; a.w_ref = prm[PQP_REFINE_W_REF]; a.w_accel = prm[PQP_REFINE_W_ACCEL]; a.w_jerk = prm[PQP_REFINE_W_JERK];
    a.a_max = prm[PQP_REFINE_A_MAX]; a.d_max = prm[PQP_REFINE_D_MAX];
    a.paths = paths; a.n_of = n_of; a.stop_before = stop_before; a.profile = profile; a.v_start = v_start; a.blocked = blocked; a.steps = steps;
    a.reached = reached; a.search_traj = search_traj; a.corridor = h->rf.bounds.as<double>();
    a.pband = h->rf.pband.as<double>(); a.q = h->rf.q.as<double>(); a.aval = h->rf.aval.as<double>(); a.lo = h->rf.lo.as<double>();
    a.up = h->rf.up.as<double>(); a.x = h->rf.x.as<double>();
    a.traj = traj; a.bounds = bounds; a.cost = cost; a.excess = excess; a.status = status; a.iters = iters; a.flags = flags;
    // always the exact optimum: the production tolerances with the KKT-verified polish, whatever the handle's path-QP setting
    pqp_params exact;
    pqp::production_params(&exact);
    exact.polish = 1;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::st_corridor_kernel, dim3((unsigned)batch), dim3(pqp::kRefineThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        if (solve) {
            const long long total = (long long)batch * m;
            hipLaunchKernelGGL(pqp::refine_assemble_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, a);
            PQP_HIP(hipGetLastError());
            if (const int rc2 = sm_solve(h, h->rf, exact, kBandedRefine, batch, m, nullptr, status, iters, nullptr, false)) return rc2;
        }
        hipLaunchKernelGGL(pqp::refine_finish_kernel, dim3((unsigned)batch), dim3(pqp::kRefineThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_speed_refine(pqp_handle* h, const pqp_search_params* grid, const double* prm, int window, int batch, int n, int stride,
                     const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start, int m,
                     const int32_t* blocked, const int32_t* steps, const int32_t* reached, const double* search_traj, double* traj,
                     double* bounds, double* cost, double* excess, int32_t* status, int32_t* iters, int32_t* flags) {
    if (!refine_ok(h, grid, prm, window, batch, n, stride, paths, profile, v_start, m, blocked, steps, reached, search_traj, traj, cost, status, iters, flags))
        return fail(PQP_ERR_INVALID, kRefineRefusal);
    if (!refine_fits(m)) return fail(PQP_ERR_CAPACITY, "pqp_speed_refine: the QP of m layers is beyond what the banded core holds in one CU's LDS");
    const size_t bn = (size_t)batch * n, bm = (size_t)batch * m, words = (size_t)(grid->stations + 31) / 32;
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_stop = st.in(stop_before, batch);
    const double* d_profile = st.in(profile, bn * PQP_SPEED_STRIDE);
    const double* d_start = st.in(v_start, batch);
    const int32_t* d_blocked = st.in(blocked, bm * words);
    const int32_t* d_steps = st.in(steps, bm * 2);
    const int32_t* d_reached = st.in(reached, batch);
    const double* d_from = st.in(search_traj, bm * PQP_TRAJ_STRIDE);
    double* d_traj = st.out(traj, bm * PQP_TRAJ_STRIDE);
    double* d_bounds = bounds ? st.out(bounds, bm * 3) : nullptr;
    double* d_cost = st.out(cost, batch);
    double* d_excess = excess ? st.out(excess, batch) : nullptr;
    int32_t* d_status = st.out(status, batch);
    int32_t* d_iters = st.out(iters, batch);
    int32_t* d_flags = st.out(flags, batch);
    return st.run([&]() -> int {
        return pqp_speed_refine_device(h, grid, prm, window, batch, n, stride, d_paths, d_n_of, d_stop, d_profile, d_start, m, d_blocked, d_steps,
                                       d_reached, d_from, d_traj, d_bounds, d_cost, d_excess, d_status, d_iters, d_flags);
    });
}

// ---- speed plans on a fine time step --------------------------------------------------------------------------------------------------------
static const char* const kPlanRefusal =
    "pqp_sample_plan: bad argument (batch >= 1; n >= 1; m >= 1; r >= 1; stride >= 6; dt finite and > 0; linear 0 or 1; (m - 1) * r + 1 <= INT_MAX)";

static bool plan_ok(pqp_handle* h, double dt, int r, int linear, int batch, int n, int stride, const double* paths, const double* profile, int m,
                    const double* plan, const double* fine, const int32_t* m_of, const int32_t* flags) {
    return h && paths && profile && plan && fine && m_of && flags && batch >= 1 && n >= 1 && m >= 1 && r >= 1 && stride >= 6 && std::isfinite(dt) &&
           dt > 0.0 && (linear == 0 || linear == 1) && (long long)(m - 1) * r + 1 <= INT_MAX;
}

int pqp_sample_plan_device(pqp_handle* h, double dt, int r, int linear, int batch, int n, int stride, const double* paths,
                           const int32_t* n_of, const int32_t* stop_before, const double* profile, int m, const double* plan,
                           const int32_t* count_of, const int32_t* refine_flags, double* fine, int32_t* m_of, double* defect,
                           double* excess, int32_t* flags) {
    if (!plan_ok(h, dt, r, linear, batch, n, stride, paths, profile, m, plan, fine, m_of, flags)) return fail(PQP_ERR_INVALID, kPlanRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::PlanArgs a;
    a.batch = batch; a.n = n; a.stride = stride; a.m = m; a.r = r; a.linear = linear; a.dt = dt; a.paths = paths; a.n_of = n_of;
    a.stop_before = stop_before; a.profile = profile; a.plan = plan; a.count_of = count_of; a.refine_flags = refine_flags; a.fine = fine;
    a.m_of = m_of; a.defect = defect; a.excess = excess; a.flags = flags;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::plan_sample_kernel, wave_grid(batch, pqp::kPlanThreads), dim3(pqp::kPlanThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_sample_plan(pqp_handle* h, double dt, int r, int linear, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                    const int32_t* stop_before, const double* profile, int m, const double* plan, const int32_t* count_of,
                    const int32_t* refine_flags, double* fine, int32_t* m_of, double* defect, double* excess, int32_t* flags) {
    if (!plan_ok(h, dt, r, linear, batch, n, stride, paths, profile, m, plan, fine, m_of, flags)) return fail(PQP_ERR_INVALID, kPlanRefusal);
    const size_t bn = (size_t)batch * n, fine_rows = (size_t)batch * ((size_t)(m - 1) * r + 1);
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_stop = st.in(stop_before, batch);
    const double* d_profile = st.in(profile, bn * PQP_SPEED_STRIDE);
    const double* d_plan = st.in(plan, (size_t)batch * m * PQP_TRAJ_STRIDE);
    const int32_t* d_count = st.in(count_of, batch);
    const int32_t* d_rflags = st.in(refine_flags, batch);
    double* d_fine = st.out(fine, fine_rows * PQP_TRAJ_STRIDE);
    int32_t* d_m_of = st.out(m_of, batch);
    double* d_defect = defect ? st.out(defect, batch) : nullptr;
    double* d_excess = excess ? st.out(excess, batch) : nullptr;
    int32_t* d_flags = st.out(flags, batch);
    return st.run([&]() -> int {
        return pqp_sample_plan_device(h, dt, r, linear, batch, n, stride, d_paths, d_n_of, d_stop, d_profile, m, d_plan, d_count, d_rflags, d_fine,
                                      d_m_of, d_defect, d_excess, d_flags);
    });
}

// ---- scores of finished trajectories and each group's best ---------------------------------------------------------------------------------
void pqp_rank_default_params(double* prm, int* require_free) {
    if (prm) {
        pqp_select_params sel;
        pqp_select_default_params(&sel);
        // this library's choice: the reference has no speed plan to weigh against its path
        prm[PQP_RANK_W_PATH] = prm[PQP_RANK_W_PROGRESS] = prm[PQP_RANK_W_ACCEL] = prm[PQP_RANK_W_JUMP] = prm[PQP_RANK_W_LATERAL] = 1.0;
        prm[PQP_RANK_W_CLEARANCE] = 0.0;
        prm[PQP_RANK_CLEARANCE_WANT] = sel.clearance_want;
    }
    if (require_free) *require_free = 1;
}

static const char* const kRankRefusal =
    "pqp_select_plans: bad argument (batch >= 1; m >= 1; stride >= 8; with paths n >= 1 and path_stride >= 7; groups >= 0; best_traj and best_m "
    "both or neither; best_paths and best_n both or neither, and only with paths; every parameter finite; require_free 0 or 1)";

static bool rank_ok(pqp_handle* h, const double* prm, int require_free, int batch, int m, int stride, const double* traj, int n, int path_stride,
                    const double* paths, int groups, const int32_t* group_start, const double* terms, const int32_t* best, const double* best_traj,
                    const int32_t* best_m, const double* best_paths, const int32_t* best_n) {
    if (!(h && prm && traj && group_start && terms && best && batch >= 1 && m >= 1 && stride >= PQP_TRAJ_STRIDE && groups >= 0)) return false;
    if (paths && !(n >= 1 && n <= (1 << 30) && path_stride >= 7)) return false;
    if ((best_traj != nullptr) != (best_m != nullptr) || (best_paths != nullptr) != (best_n != nullptr) || (best_paths && !paths)) return false;
    for (int k = 0; k < PQP_RANK_PARAMS; ++k)
        if (!std::isfinite(prm[k])) return false;
    return require_free == 0 || require_free == 1;
}

int pqp_select_plans_device(pqp_handle* h, const double* prm, int require_free, int batch, int m, int stride, const double* traj,
                            const int32_t* m_of, const double* path_terms, const int32_t* search_flags, const int32_t* first_hit,
                            const double* clearance, int n, int path_stride, const double* paths, const int32_t* n_of, int groups,
                            const int32_t* group_start, double* terms, int32_t* best, double* best_traj, int32_t* best_m, double* best_paths,
                            int32_t* best_n) {
    if (!rank_ok(h, prm, require_free, batch, m, stride, traj, n, path_stride, paths, groups, group_start, terms, best, best_traj, best_m, best_paths, best_n))
        return fail(PQP_ERR_INVALID, kRankRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::RankArgs a;
    a.batch = batch; a.m = m; a.stride = stride; a.n = n; a.path_stride = path_stride; a.groups = groups; a.require_free = require_free;
    a.traj = traj; a.m_of = m_of; a.path_terms = path_terms; a.search_flags = search_flags; a.first_hit = first_hit; a.clearance = clearance;
    a.paths = paths; a.n_of = n_of; a.group_start = group_start;
    for (int k = 0; k < PQP_RANK_PARAMS; ++k) a.prm[k] = prm[k];
    a.terms = terms; a.best = best; a.best_traj = best_traj; a.best_m = best_m; a.best_paths = best_paths; a.best_n = best_n;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::plan_score_kernel, wave_grid(batch, pqp::kRankThreads), dim3(pqp::kRankThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        if (groups > 0) {
            hipLaunchKernelGGL(pqp::plan_group_kernel, wave_grid(groups, pqp::kRankThreads), dim3(pqp::kRankThreads), 0, h->stream, a);
            PQP_HIP(hipGetLastError());
        }
        return PQP_OK;
    });
}

int pqp_select_plans(pqp_handle* h, const double* prm, int require_free, int batch, int m, int stride, const double* traj, const int32_t* m_of,
                     const double* path_terms, const int32_t* search_flags, const int32_t* first_hit, const double* clearance, int n,
                     int path_stride, const double* paths, const int32_t* n_of, int groups, const int32_t* group_start, double* terms,
                     int32_t* best, double* best_traj, int32_t* best_m, double* best_paths, int32_t* best_n) {
    if (!rank_ok(h, prm, require_free, batch, m, stride, traj, n, path_stride, paths, groups, group_start, terms, best, best_traj, best_m, best_paths, best_n))
        return fail(PQP_ERR_INVALID, kRankRefusal);
    if (group_start[0] != 0 || group_start[groups] != batch) return fail(PQP_ERR_INVALID, "pqp_select_plans: group_start must run from 0 to batch");
    for (int g = 0; g < groups; ++g)
        if (group_start[g + 1] < group_start[g]) return fail(PQP_ERR_INVALID, "pqp_select_plans: group_start must be ascending");
    // (from here on groups >= 1: group_start runs from 0 to batch >= 1)
    const size_t bm = (size_t)batch * m;
    Staging st(h);
    const double* d_traj = st.in(traj, bm * stride);
    const int32_t* d_m_of = st.in(m_of, batch);
    const double* d_path_terms = st.in(path_terms, (size_t)batch * PQP_SCORE_STRIDE);
    const int32_t* d_sflags = st.in(search_flags, batch);
    const int32_t* d_first = st.in(first_hit, batch);
    const double* d_clear = st.in(clearance, bm);
    const double* d_paths = paths ? st.in(paths, (size_t)batch * n * path_stride) : nullptr;
    const int32_t* d_n_of = paths ? st.in(n_of, batch) : nullptr;
    const int32_t* d_start = st.in(group_start, (size_t)groups + 1);
    double* d_terms = st.out(terms, (size_t)batch * PQP_PLAN_SCORE_STRIDE);
    int32_t* d_best = st.out(best, groups);
    double* d_best_traj = best_traj ? st.out(best_traj, (size_t)groups * m * PQP_TRAJ_STRIDE) : nullptr;
    int32_t* d_best_m = best_m ? st.out(best_m, groups) : nullptr;
    double* d_best_paths = best_paths ? st.out(best_paths, (size_t)groups * n * 7) : nullptr;
    int32_t* d_best_n = best_n ? st.out(best_n, groups) : nullptr;
    return st.run([&]() -> int {
        return pqp_select_plans_device(h, prm, require_free, batch, m, stride, d_traj, d_m_of, d_path_terms, d_sflags, d_first, d_clear, n, path_stride,
                                       d_paths, d_n_of, groups, d_start, d_terms, d_best, d_best_traj, d_best_m, d_best_paths, d_best_n);
    });
}

}  // extern "C"
