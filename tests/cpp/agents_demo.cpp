// PathOptimizationNS::AgentChecker (include/pqp_agent_checker.hpp) from C++ (tests/test_agents_check.py, tests/test_gpu_agents_check.py).
// Reads a binary file:
//   int32 B, m, n_scenes, a_max; double margin; int32 m_of [B], a_of [n_scenes], scene_of [B]; double traj [B][m][3] x, y, heading;
//   double agents [n_scenes][a_max][m][6] x, y, heading, half_length, half_width, radius
// and prints one line per path: "path b first_hit hit_agent rows", then one line per checked sample of it: its clearance (%.17g).
// Exit 1 without a usable GPU.
#include <cstdio>
#include <vector>

#include "../../include/pqp_agent_checker.hpp"

using PathOptimizationNS::AgentChecker;
using PathOptimizationNS::PredictedAgent;
using PathOptimizationNS::State;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: agents_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    const auto bad_file = [&]() { std::fclose(f); std::fprintf(stderr, "agents_demo: short or bad file\n"); return 2; };
    int32_t hdr[4];
    double margin;
    if (std::fread(hdr, 4, 4, f) != 4 || std::fread(&margin, 8, 1, f) != 1 || hdr[0] < 1 || hdr[1] < 1 || hdr[2] < 1 || hdr[3] < 0) return bad_file();
    const size_t B = hdr[0], m = hdr[1], S = hdr[2], A = hdr[3];
    std::vector<int32_t> m_of(B), a_of(S), scene_of(B);
    std::vector<double> traj(B * m * 3), agents(S * A * m * 6);
    if (std::fread(m_of.data(), 4, B, f) != B || std::fread(a_of.data(), 4, S, f) != S || std::fread(scene_of.data(), 4, B, f) != B ||
        std::fread(traj.data(), 8, traj.size(), f) != traj.size() || std::fread(agents.data(), 8, agents.size(), f) != agents.size())
        return bad_file();
    std::fclose(f);
    for (size_t b = 0; b < B; ++b)
        if (m_of[b] < 0 || (size_t)m_of[b] > m || scene_of[b] < 0 || (size_t)scene_of[b] >= S) { std::fprintf(stderr, "agents_demo: short or bad file\n"); return 2; }
    for (size_t s = 0; s < S; ++s)
        if (a_of[s] < 0 || (size_t)a_of[s] > A) { std::fprintf(stderr, "agents_demo: short or bad file\n"); return 2; }

    pqp_handle* h = nullptr;
    if (pqp_create(&h, nullptr, 0, 1, 2) != PQP_OK) { std::fprintf(stderr, "no checker: %s\n", pqp_last_error()); return 1; }
    int rc = 0;
    {
        AgentChecker checker(*h);
        checker.params().margin = margin;
        std::vector<std::vector<State>> paths(B);
        for (size_t b = 0; b < B; ++b) {
            paths[b].resize(m_of[b]);
            for (size_t k = 0; k < paths[b].size(); ++k) {
                const double* r = &traj[(b * m + k) * 3];
                paths[b][k].x = r[0]; paths[b][k].y = r[1]; paths[b][k].heading = r[2];
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
        std::vector<int> first_hit, hit_agent, scene(scene_of.begin(), scene_of.end());
        std::vector<std::vector<double>> clearance;
        if (!checker.check(paths, scenes, &first_hit, &hit_agent, &clearance, &scene)) {
            std::fprintf(stderr, "check: %s\n", pqp_last_error());
            rc = 1;
        } else {
            for (size_t b = 0; b < B; ++b) {
                std::printf("path %zu %d %d %zu\n", b, first_hit[b], hit_agent[b], clearance[b].size());
                for (const double c : clearance[b]) std::printf("%.17g\n", c);
            }
        }
    }
    pqp_destroy(h);
    return rc;
}
