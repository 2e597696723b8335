// PathOptimizationNS::SpeedSearcher (include/pqp_speed_searcher.hpp) from C++ (tests/test_speed_search.py, tests/test_gpu_speed_search.py).
// Reads a binary file:
//   int32 B, n, m, n_scenes, a_max, stations, q_max, q_up, q_down; double dt, ds, w_slow, w_accel, margin;
//   int32 n_of [B], stop_before [B], a_of [n_scenes], scene_of [B]; double v_start [B];
//   double rows [B][n][8] x, y, heading, k, s, v, a, t; double agents [n_scenes][a_max][m][6]
// and prints one line per path: "path b reached flags j_0 q_0 j_1 q_1 ...".  The driven count of a path is min(n_of, stop_before).
// Exit 1 without a usable GPU.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../include/pqp_speed_searcher.hpp"

using PathOptimizationNS::PredictedAgent;
using PathOptimizationNS::SpeedSearcher;
using PathOptimizationNS::State;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: search_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    const auto bad_file = [&]() { if (f) std::fclose(f); std::fprintf(stderr, "search_demo: short or bad file\n"); return 2; };
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
    if (pqp_create(&h, nullptr, 0, 1, 2) != PQP_OK) { std::fprintf(stderr, "no searcher: %s\n", pqp_last_error()); return 1; }
    int rc = 0;
    {
        SpeedSearcher searcher(*h);
        pqp_search_params& p = searcher.params();
        p.stations = hdr[5]; p.q_max = hdr[6]; p.q_up = hdr[7]; p.q_down = hdr[8];
        p.dt = prm[0]; p.ds = prm[1]; p.w_slow = prm[2]; p.w_accel = prm[3]; p.margin = prm[4];
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
        std::vector<SpeedSearcher::Plan> plans;
        std::vector<int> scene(scene_of.begin(), scene_of.end());
        if (!searcher.search(paths, v_start, scenes, &plans, (std::vector<std::vector<State>>*)nullptr, &scene, (int)m)) {
            std::fprintf(stderr, "search: %s\n", pqp_last_error());
            rc = 1;
        } else {
            for (size_t b = 0; b < B; ++b) {
                std::printf("path %zu %zu %d", b, plans[b].station.size(), plans[b].flags);
                for (size_t k = 0; k < m; ++k)
                    std::printf(" %d %d", k < plans[b].station.size() ? plans[b].station[k] : -1, k < plans[b].step.size() ? plans[b].step[k] : -1);
                std::printf("\n");
            }
        }
    }
    pqp_destroy(h);
    return rc;
}
