// Host build of pqp_distance_layer (path_optimizer_2_amd/csrc/pqp_distance_layer.hpp): both phases of every map run the device per-line
// routines on the CPU, phase A with the 64 lanes of a wavefront's ballot looped over.  TEST INFRASTRUCTURE: it lets
// tests/test_distance_layer.py check the algorithm bit for bit in a container without a GPU; nothing in the product links it.
#include <cstdint>
#include <cstring>

#include "../../path_optimizer_2_amd/csrc/pqp_distance_layer.hpp"

extern "C" {

// grid [n_maps][cols][rows] uint8 (0 = obstacle) -> dist [n_maps][cols][rows] float; the same dispatch as pqp_distance_layer_device
int pqp_emu_distance_layer(int n_maps, int rows, int cols, double resolution, const uint8_t* grid, float* dist) {
    using namespace pqp::edt;
    if (n_maps < 1 || rows < 2 || cols < 2 || (long long)rows * cols >= (1ll << 30) || !(resolution > 0.0)) return -1;
    int32_t* out = reinterpret_cast<int32_t*>(dist);
    const long long lines = (long long)n_maps * cols;
    for (long long line = 0; line < lines; ++line) {
        const uint8_t* src = grid + line * rows;
        int32_t* dst = out + line * rows;
        auto mask_at = [&](int base) {
            uint64_t m = 0;
            for (int lane = 0; lane < 64; ++lane)
                if (base + lane < rows && src[base + lane] == 0) m |= 1ull << lane;
            return m;
        };
        auto emit = [&](int base, uint64_t mask, int prev, int next) {
            for (int lane = 0; lane < 64 && base + lane < rows; ++lane) dst[base + lane] = cell_g(rows, base, lane, mask, prev, next);
        };
        obstacle_line(rows, mask_at, emit);
    }
    const Shape sh = shape_of(rows, cols);
    for (long long m = 0; m < n_maps; ++m)
        for (int r = 0; r < rows; ++r) {
            int32_t* line = out + m * rows * cols + r;
            if (sh.wide) envelope_line<int64_t>(line, rows, cols, sh.site_bits, sh.empty_d2, (float)resolution);
            else envelope_line<int32_t>(line, rows, cols, sh.site_bits, sh.empty_d2, (float)resolution);
        }
    return 0;
}

// 1 when this build takes the 64-bit path for the map (pqp_distance_layer_device's choice)
int pqp_emu_distance_wide(int rows, int cols) { return pqp::edt::shape_of(rows, cols).wide ? 1 : 0; }

float pqp_emu_sqrt_rn(uint64_t d2) { return pqp::edt::sqrt_rn(d2); }

}  // extern "C"
