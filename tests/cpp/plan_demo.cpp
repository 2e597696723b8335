// PathOptimizationNS::PlanSampler (include/pqp_plan_sampler.hpp) from C++ (tests/test_plan_sample.py, tests/test_gpu_plan_sample.py).
// Reads the binary file of search_demo.cpp (tests/search_util.py's write_case) and the sub-steps per layer, and prints one line per path:
// "path b flags refine_flags layers states s_0 v_0 a_0 s_1 v_1 a_1 ..." with every double as %.17g.  The driven count of a path is
// min(n_of, stop_before).  Exit 1 without a usable GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/pqp_plan_sampler.hpp"

using PathOptimizationNS::PlanSampler;
using PathOptimizationNS::PredictedAgent;
using PathOptimizationNS::SpeedRefiner;
using PathOptimizationNS::SpeedSearcher;
using PathOptimizationNS::State;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: plan_demo <file> <sub-steps>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    const auto bad_file = [&]() { if (f) std::fclose(f); std::fprintf(stderr, "plan_demo: short or bad file\n"); return 2; };
    int32_t hdr[9];
    double prm[5];
    if (std::fread(hdr, 4, 9, f) != 9 || std::fread(prm, 8, 5, f) != 5 || hdr[0] < 1 || hdr[1] < 1 || hdr[2] < 1 || hdr[3] < 1 || hdr[4] < 0) return bad_file();
    const size_t B = hdr[0], n = hdr[1], m = hdr[2], S = hdr[3], A = hdr[4];
    std::vector<int32_t> n_of(B), stop(B), a_of(S), scene_of(B);
    std::vector<double> v_start(B), rows(B * n * 8), agents(S * A * m * 6);
    if (std::fread(n_of.data(), 4, B, f) != B || std::fread(stop.data(), 4, B, f) != B || std::fread(a_of.data(), 4, S, f) != S ||
        std::fread(scene_of.data(), 4, B, f) != B || std::fread(v_start.data(), 8, B, f) != B || std::fread(rows.data(), 8, rows.size(), f) != rows.size() ||
        std::fread(agents.data(), 8, agents.size(), f) != agents.size())
        return bad_file();
    std::fclose(f);
    f = nullptr;
    for (size_t b = 0; b < B; ++b)
        if (n_of[b] < 0 || (size_t)n_of[b] > n || stop[b] < 0 || scene_of[b] < 0 || (size_t)scene_of[b] >= S) return bad_file();
    for (size_t s = 0; s < S; ++s)
        if (a_of[s] < 0 || (size_t)a_of[s] > A) return bad_file();

    pqp_handle* h = nullptr;
    if (pqp_create(&h, nullptr, 0, 1, 2) != PQP_OK) { std::fprintf(stderr, "no plan sampler: %s\n", pqp_last_error()); return 1; }
    int rc = 0;
    {
        SpeedSearcher searcher(*h);
        pqp_search_params& p = searcher.params();
        p.stations = hdr[5]; p.q_max = hdr[6]; p.q_up = hdr[7]; p.q_down = hdr[8];
        p.dt = prm[0]; p.ds = prm[1]; p.w_slow = prm[2]; p.w_accel = prm[3]; p.margin = prm[4];
        SpeedRefiner refiner(searcher);
        PlanSampler sampler(refiner);
        sampler.sub_steps() = std::atoi(argv[2]);
        std::vector<std::vector<State>> paths(B);
        for (size_t b = 0; b < B; ++b) {
            paths[b].resize(std::min(n_of[b], stop[b]));
            for (size_t i = 0; i < paths[b].size(); ++i) {
                const double* r = &rows[(b * n + i) * 8];
                State& st = paths[b][i];
                st.x = r[0]; st.y = r[1]; st.heading = r[2]; st.k = r[3]; st.s = r[4]; st.v = r[5]; st.a = r[6];
            }
        }
        std::vector<std::vector<std::vector<PredictedAgent>>> scenes(S);
        for (size_t s = 0; s < S; ++s) {
            scenes[s].resize(a_of[s]);
            for (size_t a = 0; a < scenes[s].size(); ++a) {
                scenes[s][a].resize(m);
                for (size_t k = 0; k < m; ++k) {
                    const double* r = &agents[((s * A + a) * m + k) * 6];
                    scenes[s][a][k] = PredictedAgent{r[0], r[1], r[2], r[3], r[4], r[5]};
                }
            }
        }
        std::vector<PlanSampler::Result> results;
        std::vector<std::vector<State>> states;
        std::vector<int> scene(scene_of.begin(), scene_of.end());
        if (!sampler.sample(paths, v_start, scenes, &results, &states, &scene, (int)m)) {
            std::fprintf(stderr, "sample: %s\n", pqp_last_error());
            rc = 1;
        } else {
            for (size_t b = 0; b < B; ++b) {
                std::printf("path %zu %d %d %d %zu", b, results[b].flags, results[b].refine_flags, results[b].layers, states[b].size());
                for (const State& st : states[b]) std::printf(" %.17g %.17g %.17g", st.s, st.v, st.a);
                std::printf("\n");
            }
        }
    }
    pqp_destroy(h);
    return rc;
}
