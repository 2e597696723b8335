// pqp_distance_kernels.inc — instantiated by pqp_maps.hip; includes pqp_distance_layer.hpp.  The obstacle distance layer from an occupancy grid (pqp_distance_layer):
//   cv::distanceTransform(obstacle, dist, CV_DIST_L2, CV_DIST_MASK_PRECISE); dist *= resolution     src/test/demo.cpp:104-113
// Two launches on the handle's stream, the per-line routines of pqp_distance_layer.hpp:
//   distance_lines_kernel      phase A: one wavefront per column line (rows contiguous bytes): one byte per lane and a ballot per block of
//                              64 cells; g(r, c) goes to the dist buffer as int32, 4-byte stores of consecutive lanes.
//   distance_envelope_kernel   phase B: one lane per (map, r); consecutive lanes hold consecutive r, so the walk across the columns
//                              (stride rows) reads and writes 256 contiguous bytes per wavefront and column.

#include "pqp_distance_layer.hpp"

namespace pqp {

struct DistanceArgs {
    const uint8_t* grid;             // [n_maps][cols][rows]  0 = obstacle
    int32_t* out;                    // [n_maps][cols][rows]  g (phase A), then the float layer (phase B)
    long long n_maps;
    int rows, cols, site_bits;
    uint64_t empty_d2;               // rows^2 + cols^2
    float res;
};

__global__ void __launch_bounds__(256) distance_lines_kernel(DistanceArgs a) {
    const int lane = threadIdx.x & 63;
    const long long lines = a.n_maps * a.cols, waves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long line = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); line < lines; line += waves) {
        const uint8_t* src = a.grid + line * a.rows;
        int32_t* dst = a.out + line * a.rows;
        const int rows = a.rows;
        auto mask_at = [&](int base) -> uint64_t {
            const bool obstacle = base + lane < rows && src[base + lane] == 0;
            return __ballot(obstacle);
        };
        auto emit = [&](int base, uint64_t mask, int prev, int next) {
            if (base + lane < rows) dst[base + lane] = edt::cell_g(rows, base, lane, mask, prev, next);
        };
        edt::obstacle_line(rows, mask_at, emit);
    }
}

template <class D>
__global__ void __launch_bounds__(64) distance_envelope_kernel(DistanceArgs a) {
    const long long lanes = a.n_maps * a.rows, stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < lanes; i += stride) {
        const long long m = i / a.rows, r = i - m * a.rows;
        edt::envelope_line<D>(a.out + m * a.rows * a.cols + r, a.rows, a.cols, a.site_bits, a.empty_d2, a.res);
    }
}

}  // namespace pqp
