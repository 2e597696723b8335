// PathOptimizationNS::FootprintChecker (include/pqp_footprint_checker.hpp) from C++ (tests/test_cpp_footprint.py).  Reads a binary file:
//   int32 rows, cols, n_maps, n_paths; double resolution, length_x, length_y, pos_x, pos_y; float layers [n_maps][cols][rows];
//   per path: int32 n, map; double [n][3] x, y, heading
// and prints, per path: "path <first collision, CIRCLES> <first collision, BOUNDING_FIRST>" from two checkPaths calls, then one line per state
// "<isSingleStateCollisionFree> <isSingleStateCollisionFreeImproved> <free from checkPaths, CIRCLES>".  Exit 1 without a usable GPU.
#include <cstdio>
#include <vector>

#include "../../include/pqp_footprint_checker.hpp"

using PathOptimizationNS::FootprintChecker;
using PathOptimizationNS::SlState;
using PathOptimizationNS::State;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: footprint_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    int32_t hdr[4];
    double gd[5];
    if (std::fread(hdr, 4, 4, f) != 4 || std::fread(gd, 8, 5, f) != 5) return 2;
    const pqp_grid_geometry geom{hdr[0], hdr[1], gd[0], gd[1], gd[2], gd[3], gd[4]};
    const int n_maps = hdr[2], n_paths = hdr[3];
    std::vector<float> layers((size_t)n_maps * geom.rows * geom.cols);
    if (std::fread(layers.data(), 4, layers.size(), f) != layers.size()) return 2;
    std::vector<std::vector<SlState>> paths(n_paths);
    std::vector<int> map_of(n_paths);
    for (int k = 0; k < n_paths; ++k) {
        int32_t nm[2];
        if (std::fread(nm, 4, 2, f) != 2) return 2;
        map_of[k] = nm[1];
        paths[k].resize(nm[0]);
        for (auto& s : paths[k]) {
            double v[3];
            if (std::fread(v, 8, 3, f) != 3) return 2;
            s.x = v[0]; s.y = v[1]; s.heading = v[2];
        }
    }
    std::fclose(f);

    FootprintChecker checker(layers.data(), n_maps, geom);
    if (!checker.ok()) { std::fprintf(stderr, "no checker: %s\n", pqp_last_error()); return 1; }
    std::vector<int> first_c, first_b;
    std::vector<std::vector<uint8_t>> free_c;
    if (!checker.checkPaths(paths, &first_c, PQP_FOOTPRINT_CIRCLES, &map_of, &free_c) ||
        !checker.checkPaths(paths, &first_b, PQP_FOOTPRINT_BOUNDING_FIRST, &map_of)) {
        std::fprintf(stderr, "checkPaths: %s\n", pqp_last_error());
        return 1;
    }
    for (int k = 0; k < n_paths; ++k) {
        std::printf("path %d %d\n", first_c[k], first_b[k]);
        for (size_t i = 0; i < paths[k].size(); ++i) {
            const State& s = paths[k][i];
            std::printf("%d %d %d\n", checker.isSingleStateCollisionFree(s, map_of[k]) ? 1 : 0,
                        checker.isSingleStateCollisionFreeImproved(s, map_of[k]) ? 1 : 0, (int)free_c[k][i]);
        }
    }
    return 0;
}
