// PathOptimizationNS::PathSelector (include/pqp_path_selector.hpp) from C++ (tests/test_select_paths.py, tests/test_gpu_select_paths.py).
// Reads a binary file:
//   int32 n_paths, groups; int32 group_start [groups + 1]; per path: int32 n; double [n][7] x, y, heading, l, d_heading, k, dk
// and prints one line "best <index>" per group, then one line "score <%.17g>" per path.  Exit 1 without a usable GPU.
#include <cstdio>
#include <vector>

#include "../../include/pqp_path_selector.hpp"

using PathOptimizationNS::PathSelector;
using PathOptimizationNS::SlState;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: select_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    const auto bad_file = [&]() { std::fclose(f); std::fprintf(stderr, "select_demo: short or bad file\n"); return 2; };
    int32_t hdr[2];
    if (std::fread(hdr, 4, 2, f) != 2 || hdr[0] < 0 || hdr[1] < 0) return bad_file();
    const int n_paths = hdr[0], groups = hdr[1];
    std::vector<int32_t> gs(groups + 1);
    if (std::fread(gs.data(), 4, gs.size(), f) != gs.size()) return bad_file();
    std::vector<std::vector<SlState>> paths(n_paths);
    for (auto& p : paths) {
        int32_t n;
        if (std::fread(&n, 4, 1, f) != 1 || n < 0) return bad_file();
        p.resize(n);
        for (auto& s : p) {
            double v[7];
            if (std::fread(v, 8, 7, f) != 7) return bad_file();
            s.x = v[0]; s.y = v[1]; s.heading = v[2]; s.l = v[3]; s.d_heading = v[4]; s.k = v[5]; s.d_k = v[6];
        }
    }
    std::fclose(f);

    PathSelector selector;
    if (!selector.ok()) { std::fprintf(stderr, "no selector: %s\n", pqp_last_error()); return 1; }
    std::vector<int> best;
    std::vector<double> score;
    if (!selector.selectBest(paths, std::vector<int>(gs.begin(), gs.end()), &best, &score)) {
        std::fprintf(stderr, "selectBest: %s\n", pqp_last_error());
        return 1;
    }
    for (int g = 0; g < groups; ++g) std::printf("best %d\n", best[g]);
    for (int b = 0; b < n_paths; ++b) std::printf("score %.17g\n", score[b]);
    return 0;
}
