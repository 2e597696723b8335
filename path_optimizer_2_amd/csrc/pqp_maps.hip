// pqp_maps.hip — the entry points of include/pqp.h around the obstacle distance map: the distance layer from an occupancy grid
// (pqp_distance_kernels.inc), vehicle footprints against it (pqp_footprint_kernels.inc) and standing agents laid over the layers
// (pqp_overlay_kernels.inc).  Their kernels, launchers and entry points, and the car's circles on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "pqp_internal.hpp"

using namespace pqp_internal;

#include "pqp_distance_kernels.inc"
#include "pqp_footprint_kernels.inc"
#include "pqp_overlay_kernels.inc"

int pqp_internal::car_circles_of(const pqp_car_geometry* car, pqp::CarCircles* c) {
    double circles[7][3];
    if (const int rc = pqp_car_circles(car, &circles[0][0])) return rc;
    for (int k = 0; k < 7; ++k) { c->cx[k] = circles[k][0]; c->cy[k] = circles[k][1]; c->cr[k] = circles[k][2]; }
    // the reference's own bounding circle (circles[6][2]) does not contain the corner circles: the broad phase takes the radius that does
    c->rb = 0.0;
    for (int k = 0; k < 6; ++k) c->rb = std::max(c->rb, std::hypot(c->cx[k] - c->cx[6], c->cy[k] - c->cy[6]) + c->cr[k]);
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
    if (!(h && dist && dist_out && flags && n_maps >= 1 && agent_rows_ok(n_scenes, a_max, 1, agents) && geometry_ok(geom))) return false;
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
    const size_t cells = (size_t)geom->rows * geom->cols;
    Staging st(h);
    // (dist_out = dist: the device form then runs on two arrays, and by the definition gives what it gives in place)
    const float* d_dist = st.in(dist, (size_t)n_maps * cells);
    const AgentArrays d = stage_agents(st, n_scenes, a_max, 1, agents, a_of, base_of, n_scenes);
    float* d_out = st.out(dist_out, (size_t)n_scenes * cells);
    int32_t* d_flags = st.out(flags, n_scenes);
    return st.run([&]() -> int {
        return pqp_overlay_agents_device(h, inflate, n_maps, geom, d_dist, n_scenes, a_max, d.agents, d.a_of, d.of, d.frames, d_out, d_flags);
    });
}

}  // extern "C"
