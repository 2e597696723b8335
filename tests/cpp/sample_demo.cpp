// PathOptimizationNS::TrajectorySampler (include/pqp_trajectory_sampler.hpp) from C++ (tests/test_sample_trajectory.py,
// tests/test_gpu_sample_trajectory.py).  Reads a binary file:
//   int32 B, n, m, hold_last; double dt; int32 n_of [B], stop_before [B]; double t0 [B]; double [B][n][8] x, y, heading, k, s, v, a, t
// and prints one line per path: "path b flags rows", then one line per sample of it: x y heading k s v a t (%.17g each).
// Exit 1 without a usable GPU.
#include <cstdio>
#include <vector>

#include "../../include/pqp_trajectory_sampler.hpp"

using PathOptimizationNS::State;
using PathOptimizationNS::TrajectorySampler;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: sample_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    const auto bad_file = [&]() { std::fclose(f); std::fprintf(stderr, "sample_demo: short or bad file\n"); return 2; };
    int32_t hdr[4];
    double dt;
    if (std::fread(hdr, 4, 4, f) != 4 || std::fread(&dt, 8, 1, f) != 1 || hdr[0] < 1 || hdr[1] < 1 || hdr[2] < 1) return bad_file();
    const size_t B = hdr[0], n = hdr[1];
    const int m = hdr[2];
    std::vector<int32_t> n_of(B), stop(B);
    std::vector<double> t0(B), p(B * n * 8);
    if (std::fread(n_of.data(), 4, B, f) != B || std::fread(stop.data(), 4, B, f) != B || std::fread(t0.data(), 8, B, f) != B ||
        std::fread(p.data(), 8, B * n * 8, f) != B * n * 8)
        return bad_file();
    std::fclose(f);
    for (size_t b = 0; b < B; ++b)
        if (n_of[b] < 0 || (size_t)n_of[b] > n) { std::fprintf(stderr, "sample_demo: short or bad file\n"); return 2; }

    pqp_handle* h = nullptr;
    if (pqp_create(&h, nullptr, 0, 1, 2) != PQP_OK) { std::fprintf(stderr, "no sampler: %s\n", pqp_last_error()); return 1; }
    int rc = 0;
    {
        TrajectorySampler sampler(*h);
        sampler.params().dt = dt;
        sampler.params().hold_last = hdr[3];
        std::vector<std::vector<State>> paths(B), samples;
        std::vector<std::vector<double>> times(B), sample_times;
        for (size_t b = 0; b < B; ++b) {
            paths[b].resize(n_of[b]);
            times[b].resize(n_of[b]);
            for (size_t i = 0; i < paths[b].size(); ++i) {
                const double* r = &p[(b * n + i) * 8];
                State& q = paths[b][i];
                q.x = r[0]; q.y = r[1]; q.heading = r[2]; q.k = r[3]; q.s = r[4]; q.v = r[5]; q.a = r[6];
                times[b][i] = r[7];
            }
        }
        std::vector<int> flags, stop_before(stop.begin(), stop.end());
        if (!sampler.sample(paths, times, m, &samples, &sample_times, &flags, &stop_before, &t0)) {
            std::fprintf(stderr, "sample: %s\n", pqp_last_error());
            rc = 1;
        } else {
            for (size_t b = 0; b < B; ++b) {
                std::printf("path %zu %d %zu\n", b, flags[b], samples[b].size());
                for (size_t k = 0; k < samples[b].size(); ++k) {
                    const State& q = samples[b][k];
                    std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", q.x, q.y, q.heading, q.k, q.s, q.v, q.a, sample_times[b][k]);
                }
            }
        }
    }
    pqp_destroy(h);
    return rc;
}
