// pqp_footprint_kernels.inc — instantiated by pqp_maps.hip; includes pqp_car_circles.hpp (the circles and their placement),
// pqp_driven_path.hpp (clamped_count) and pqp_line_device.hpp (obstacle_distance).  Vehicle footprints of planned states against the
// obstacle distance layer (pqp_footprint_check):
//   CollisionChecker::isSingleStateCollisionFree          src/tools/collision_checker.cpp:17-39
//   CollisionChecker::isSingleStateCollisionFreeImproved  src/tools/collision_checker.cpp:41-58
//   CarGeometry::getCircles / getBoundingCircle           src/tools/car_geometry.cpp:59-72 (the circles themselves: pqp_car_circles, host)
//   local2Global                                          src/tools/tools.cpp:50-55 (local_to_global of pqp_car_circles.hpp)
//   Map::getObstacleDistance / isInside                   src/tools/Map.cpp:16-26   (obstacle_distance of pqp_corridor_kernels.inc)
// One workgroup of 256 lanes per scenario, one state per lane, striding over the scenario's states.  A state takes one sincos and six
// map samples; the six samples' 24 cell loads are independent of each other, so they are in flight together (the layer, <= a few MB,
// sits in L2).  first_collision: one ballot per wavefront and stride step, then the least of the four wavefronts' indices through LDS -
// no atomics, the same answer every run, any n.

#include "pqp_car_circles.hpp"
#include "pqp_driven_path.hpp"
#include "pqp_line_device.hpp"

namespace pqp {

constexpr int kFootprintThreads = 256;

struct FootprintArgs {
    int batch, n, stride;
    const double* states;            // [batch][n][stride]  x, y, heading at offsets 0, 1, 2
    const int32_t* n_of;             // [batch] states per scenario (<= n), or nullptr: all have n
    const float* dist;               // [n_maps][cols][rows]  as for CorridorArgs
    const int32_t* map_of;           // [batch] or nullptr: map 0
    pqp_grid_geometry g;
    CarCircles car;
    uint8_t* free_out;               // [batch][n]
    int32_t* first_collision;        // [batch]
    double* margin;                  // [batch][n] or nullptr
};

// GridMap::isInside (checkIfPositionWithinMap), the test obstacle_distance opens with
__device__ __forceinline__ bool map_is_inside(const pqp_grid_geometry& g, double px, double py) {
#pragma clang fp contract(off)
    const double tx = -(px - g.pos_x - 0.5 * g.length_x), ty = -(py - g.pos_y - 0.5 * g.length_y);
    return tx >= 0.0 && ty >= 0.0 && tx < g.length_x && ty < g.length_y;
}

// MODE: pqp_footprint_mode.  In BOUNDING_FIRST mode the six samples are taken only where the bounding circle is not clear (or where the
// margin is asked for): lanes of one wavefront diverge there.
template <int MODE>
__global__ void __launch_bounds__(kFootprintThreads) footprint_check_kernel(const FootprintArgs a) {
#pragma clang fp contract(off)
    __shared__ int wave_first[kFootprintThreads / 64];
    const int b = blockIdx.x, wave = threadIdx.x >> 6;
    const int nb = clamped_count(a.n_of, b, a.n);
    const float* __restrict__ dist = a.dist + (size_t)(a.map_of ? a.map_of[b] : 0) * a.g.rows * a.g.cols;
    const double* st = a.states + (size_t)b * a.n * a.stride;
    int first = INT_MAX;                                                     // wave-uniform: the wavefront's first colliding index
    for (int base = 0; base < a.n; base += kFootprintThreads) {
        const int i = base + (int)threadIdx.x;
        bool collide = false;
        double mg = 0.0;
        if (i < nb) {
            const double x = st[(size_t)i * a.stride], y = st[(size_t)i * a.stride + 1], heading = st[(size_t)i * a.stride + 2];
            double sh, ch;
            sincos(heading, &sh, &ch);
            const auto place = [&](int k) { return local_to_global(a.car.cx[k], a.car.cy[k], sh, ch, x, y); };      // a circle where it is asked for
            bool bound_in = true, exact = true;
            if (MODE == PQP_FOOTPRINT_BOUNDING_FIRST) {
                const Point2 bp = place(6);
                bound_in = map_is_inside(a.g, bp.x, bp.y);
                exact = bound_in && obstacle_distance(dist, a.g, bp.x, bp.y) < a.car.cr[6];  // :49-53: the big circle is not clear
            }
            bool six = false;
            if (exact || a.margin) {
                double d[6];
                bool in[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const Point2 pk = place(k);
                    in[k] = map_is_inside(a.g, pk.x, pk.y);
                    d[k] = obstacle_distance(dist, a.g, pk.x, pk.y);                         // Map::getObstacleDistance: 0 outside
                }
                mg = d[0] - a.car.cr[0];
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    six = six || !in[k] || d[k] < a.car.cr[k];                                // :28-35
                    const double v = d[k] - a.car.cr[k];
                    mg = v < mg ? v : mg;
                }
            }
            collide = MODE == PQP_FOOTPRINT_BOUNDING_FIRST ? (!bound_in || (exact && six)) : six;
        }
        if (i < a.n) {
            a.free_out[(size_t)b * a.n + i] = (i < nb && !collide) ? 1 : 0;
            if (a.margin) a.margin[(size_t)b * a.n + i] = mg;
        }
        const uint64_t hit = __ballot(collide);
        if (hit && first == INT_MAX) first = base + wave * 64 + __builtin_ctzll(hit);
    }
    if ((threadIdx.x & 63) == 0) wave_first[wave] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        int f = nb;
#pragma unroll
        for (int w = 0; w < kFootprintThreads / 64; ++w) f = min(f, wave_first[w]);
        a.first_collision[b] = f;
    }
}

}  // namespace pqp
