// PathOptimizationNS::PlanSelector (include/pqp_plan_selector.hpp) from C++ (tests/test_select_plans.py, tests/test_gpu_select_plans.py).
// Reads a binary file (tests/rank_util.py's write_case):
//   int32 batch, m, groups; double dt; int32 group_start [groups + 1]; int32 m_of [batch]; double path_score [batch];
//   double traj [batch][m][8] = x, y, heading, k, s, v, a, t (t is not read: state f is at f * dt)
// and prints one line "best <index> <states of the winner>" per group, then one line "terms <ten %.17g>" per candidate.  Exit 1 without a
// usable GPU, 2 on a short or bad file.
#include <cstdio>
#include <vector>

#include "../../include/pqp_plan_selector.hpp"

using PathOptimizationNS::PlanSelector;
using PathOptimizationNS::State;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: rank_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    const auto bad_file = [&]() { if (f) std::fclose(f); std::fprintf(stderr, "rank_demo: short or bad file\n"); return 2; };
    int32_t hdr[3];
    double dt;
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(&dt, 8, 1, f) != 1 || hdr[0] < 1 || hdr[1] < 1 || hdr[2] < 0 || hdr[0] > (1 << 20) ||
        hdr[1] > (1 << 20) || hdr[2] > (1 << 20))
        return bad_file();
    const size_t B = hdr[0], m = hdr[1], groups = hdr[2];
    std::vector<int32_t> gs(groups + 1), m_of(B);
    std::vector<double> path_score(B), rows(B * m * 8);
    if (std::fread(gs.data(), 4, gs.size(), f) != gs.size() || std::fread(m_of.data(), 4, B, f) != B || std::fread(path_score.data(), 8, B, f) != B ||
        std::fread(rows.data(), 8, rows.size(), f) != rows.size())
        return bad_file();
    std::fclose(f);
    f = nullptr;
    for (size_t b = 0; b < B; ++b)
        if (m_of[b] < 0 || (size_t)m_of[b] > m) return bad_file();

    PlanSelector selector;
    if (!selector.ok()) { std::fprintf(stderr, "no plan selector: %s\n", pqp_last_error()); return 1; }
    std::vector<std::vector<State>> trajectories(B);
    for (size_t b = 0; b < B; ++b) {
        trajectories[b].resize(m_of[b]);
        for (size_t k = 0; k < trajectories[b].size(); ++k) {
            const double* r = &rows[(b * m + k) * 8];
            State& st = trajectories[b][k];
            st.x = r[0]; st.y = r[1]; st.heading = r[2]; st.k = r[3]; st.s = r[4]; st.v = r[5]; st.a = r[6];
        }
    }
    std::vector<int> best;
    std::vector<double> terms;
    std::vector<std::vector<State>> winners;
    PlanSelector::Optional opt;
    opt.path_score = &path_score;
    if (!selector.selectBest(trajectories, dt, std::vector<int>(gs.begin(), gs.end()), &best, &terms, &winners, opt)) {
        std::fprintf(stderr, "selectBest: %s\n", pqp_last_error());
        return 1;
    }
    for (size_t g = 0; g < groups; ++g) std::printf("best %d %zu\n", best[g], winners[g].size());
    for (size_t b = 0; b < B; ++b) {
        std::printf("terms");
        for (int e = 0; e < PQP_PLAN_SCORE_STRIDE; ++e) std::printf(" %.17g", terms[b * PQP_PLAN_SCORE_STRIDE + e]);
        std::printf("\n");
    }
    return 0;
}
