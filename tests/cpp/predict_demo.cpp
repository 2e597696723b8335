// PathOptimizationNS::AgentPredictor (include/pqp_agent_predictor.hpp) from C++ (tests/test_predict_agents.py,
// tests/test_gpu_predict_agents.py).  Reads a binary file:
//   int32 A, m, r; double dt; double tracks [A][9] x, y, heading, v, a, yaw_rate, half_length, half_width, radius
// - one scene of free-model tracks from t0 = 0 - and prints one line per agent: "agent a flags rows", then one line per step of it: its six
// values (%.17g).  Exit 1 without a usable GPU.
#include <cstdio>
#include <vector>

#include "../../include/pqp_agent_predictor.hpp"

using PathOptimizationNS::AgentPredictor;
using PathOptimizationNS::PredictedAgent;
using PathOptimizationNS::TrackedAgent;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: predict_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    int32_t hdr[3];
    double dt;
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(&dt, 8, 1, f) != 1 || hdr[0] < 0 || hdr[0] > (1 << 20) || hdr[1] < 1 || hdr[2] < 1) {
        std::fclose(f); std::fprintf(stderr, "predict_demo: short or bad file\n"); return 2;
    }
    const size_t A = hdr[0];
    std::vector<double> tracks(A * PQP_TRACK_STRIDE);
    const bool whole = std::fread(tracks.data(), 8, tracks.size(), f) == tracks.size();
    std::fclose(f);
    if (!whole) { std::fprintf(stderr, "predict_demo: short or bad file\n"); return 2; }

    pqp_handle* h = nullptr;
    if (pqp_create(&h, nullptr, 0, 1, 2) != PQP_OK) { std::fprintf(stderr, "no predictor: %s\n", pqp_last_error()); return 1; }
    int rc = 0;
    {
        AgentPredictor predictor(*h);
        std::vector<std::vector<TrackedAgent>> scenes(1);
        for (size_t a = 0; a < A; ++a) {
            const double* q = &tracks[a * PQP_TRACK_STRIDE];
            scenes[0].push_back(TrackedAgent{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], -1});
        }
        std::vector<std::vector<std::vector<PredictedAgent>>> rows;
        std::vector<std::vector<int>> flags;
        if (!predictor.predict(scenes, 0.0, dt, hdr[1], hdr[2], &rows, &flags)) {
            std::fprintf(stderr, "predict: %s\n", pqp_last_error());
            rc = 1;
        } else {
            for (size_t a = 0; a < A; ++a) {
                std::printf("agent %zu %d %zu\n", a, flags[0][a], rows[0][a].size());
                for (const PredictedAgent& p : rows[0][a])
                    std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", p.x, p.y, p.heading, p.half_length, p.half_width, p.radius);
            }
        }
    }
    pqp_destroy(h);
    return rc;
}
