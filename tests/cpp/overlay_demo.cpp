// PathOptimizationNS::AgentOverlay (include/pqp_agent_overlay.hpp) from C++ (tests/test_overlay_agents.py, tests/test_gpu_overlay_agents.py).
// Reads a binary file (tests/overlay_util.py, write_case):
//   int32 n_maps, rows, cols, n_scenes, a_max; double resolution, length_x, length_y, pos_x, pos_y, inflate; int32 base_of [n_scenes];
//   float dist [n_maps][cols][rows]; double agents [n_scenes][a_max][6] x, y, heading, half_length, half_width, radius
// and prints one line per scene: "scene s flag", then its layer [cols][rows], one value per line as the hexadecimal of its bits.
// Exit 1 without a usable GPU.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/pqp_agent_overlay.hpp"

using PathOptimizationNS::AgentOverlay;
using PathOptimizationNS::StandingAgent;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: overlay_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    const auto bad_file = [&]() { std::fclose(f); std::fprintf(stderr, "overlay_demo: short or bad file\n"); return 2; };
    int32_t hdr[5];
    double par[6];
    if (std::fread(hdr, 4, 5, f) != 5 || std::fread(par, 8, 6, f) != 6 || hdr[0] < 1 || hdr[1] < 2 || hdr[2] < 2 || hdr[3] < 1 || hdr[4] < 0)
        return bad_file();
    const size_t M = hdr[0], cells = (size_t)hdr[1] * hdr[2], S = hdr[3], A = hdr[4];
    std::vector<int32_t> base_of(S);
    std::vector<float> dist(M * cells);
    std::vector<double> rows(S * A * 6);
    if (std::fread(base_of.data(), 4, S, f) != S || std::fread(dist.data(), 4, dist.size(), f) != dist.size() ||
        std::fread(rows.data(), 8, rows.size(), f) != rows.size())
        return bad_file();
    std::fclose(f);
    pqp_grid_geometry geom;
    geom.rows = hdr[1]; geom.cols = hdr[2]; geom.resolution = par[0]; geom.length_x = par[1]; geom.length_y = par[2];
    geom.pos_x = par[3]; geom.pos_y = par[4];

    AgentOverlay over(dist.data(), (int)M, geom);
    if (!over.ok()) { std::fprintf(stderr, "no overlay: %s\n", pqp_last_error()); return 1; }
    std::vector<std::vector<StandingAgent>> scenes(S);
    for (size_t s = 0; s < S; ++s)
        for (size_t a = 0; a < A; ++a) {
            const double* r = &rows[(s * A + a) * 6];
            scenes[s].push_back(StandingAgent{r[0], r[1], r[2], r[3], r[4], r[5]});
        }
    std::vector<int> base(base_of.begin(), base_of.end()), flags;
    std::vector<float> layers;
    if (!over.overlay(scenes, nullptr, &base, par[5], &layers, &flags)) { std::fprintf(stderr, "overlay: %s\n", pqp_last_error()); return 1; }
    if (!over.layers() || over.scenes() != (int)S) { std::fprintf(stderr, "overlay: no layers on the device\n"); return 1; }
    for (size_t s = 0; s < S; ++s) {
        std::printf("scene %zu %d\n", s, flags[s]);
        for (size_t k = 0; k < cells; ++k) {
            uint32_t bits;
            std::memcpy(&bits, &layers[s * cells + k], 4);
            std::printf("%08x\n", bits);
        }
    }
    return 0;
}
