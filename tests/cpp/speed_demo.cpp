// PathOptimizationNS::SpeedProfiler (include/pqp_speed_profiler.hpp) from C++ (tests/test_speed_profile.py,
// tests/test_gpu_speed_profile.py).  Reads a binary file:
//   int32 B, n; int32 n_of [B], stop_before [B]; double v_start [B], v_end [B]; double [B][n][3] x, y, k (the paths)
// and prints one line per path: "path b flags", then one line per state of it: s v a t (%.17g each).
// Exit 1 without a usable GPU.
#include <cstdio>
#include <vector>

#include "../../include/pqp_speed_profiler.hpp"

using PathOptimizationNS::SlState;
using PathOptimizationNS::SpeedProfiler;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: speed_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    const auto bad_file = [&]() { std::fclose(f); std::fprintf(stderr, "speed_demo: short or bad file\n"); return 2; };
    int32_t hdr[2];
    if (std::fread(hdr, 4, 2, f) != 2 || hdr[0] < 1 || hdr[1] < 1) return bad_file();
    const size_t B = hdr[0], n = hdr[1];
    std::vector<int32_t> n_of(B), stop(B);
    std::vector<double> v_start(B), v_end(B), p(B * n * 3);
    if (std::fread(n_of.data(), 4, B, f) != B || std::fread(stop.data(), 4, B, f) != B || std::fread(v_start.data(), 8, B, f) != B ||
        std::fread(v_end.data(), 8, B, f) != B || std::fread(p.data(), 8, B * n * 3, f) != B * n * 3)
        return bad_file();
    std::fclose(f);
    for (size_t b = 0; b < B; ++b)
        if (n_of[b] < 0 || (size_t)n_of[b] > n) { std::fprintf(stderr, "speed_demo: short or bad file\n"); return 2; }

    pqp_handle* h = nullptr;
    if (pqp_create(&h, nullptr, 0, 1, 2) != PQP_OK) { std::fprintf(stderr, "no profiler: %s\n", pqp_last_error()); return 1; }
    int rc = 0;
    {
        SpeedProfiler profiler(*h);
        std::vector<std::vector<SlState>> paths(B);
        for (size_t b = 0; b < B; ++b) {
            paths[b].resize(n_of[b]);
            for (size_t i = 0; i < paths[b].size(); ++i) {
                const double* r = &p[(b * n + i) * 3];
                paths[b][i].x = r[0]; paths[b][i].y = r[1]; paths[b][i].k = r[2];
            }
        }
        std::vector<std::vector<double>> times;
        std::vector<int> flags, stop_before(stop.begin(), stop.end());
        if (!profiler.profile(&paths, v_start, &times, &flags, &stop_before, &v_end)) {
            std::fprintf(stderr, "profile: %s\n", pqp_last_error());
            rc = 1;
        } else {
            for (size_t b = 0; b < B; ++b) {
                std::printf("path %zu %d\n", b, flags[b]);
                for (size_t i = 0; i < paths[b].size(); ++i)
                    std::printf("%.17g %.17g %.17g %.17g\n", paths[b][i].s, paths[b][i].v, paths[b][i].a, times[b][i]);
            }
        }
    }
    pqp_destroy(h);
    return rc;
}
