// PathOptimizationNS::FallbackPlanner (include/pqp_fallback_planner.hpp) from C++ (tests/test_fallback.py, tests/test_gpu_fallback.py).
// Reads a binary file (tests/fallback_util.py's write_case):
//   int32 G, mp, m, r; double dt; int32 prev_m [G]; int32 stitch_flags [G]; double state [G][8];
//   double prev [G][mp][8] = x, y, heading, k, s, v, a, t (t is not read);
//   int32 first_hit [G * L]; int32 first_collision [G * L]      with L = the planner's default levels
// and prints per vehicle and level "plan <flags> <stop_row> <T %.17g> <e(T) %.17g>", then per vehicle "group <level> <flags> <states>" and
// one "row <eight %.17g>" per state of its plan.  Exit 1 without a usable GPU, 2 on a short or bad file.
#include <cstdio>
#include <vector>

#include "../../include/pqp_fallback_planner.hpp"

using PathOptimizationNS::FallbackPlanner;
using PathOptimizationNS::State;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: fallback_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    const auto bad_file = [&]() { if (f) std::fclose(f); std::fprintf(stderr, "fallback_demo: short or bad file\n"); return 2; };
    int32_t hdr[4];
    double dt;
    if (std::fread(hdr, 4, 4, f) != 4 || std::fread(&dt, 8, 1, f) != 1) return bad_file();
    for (int k = 0; k < 4; ++k)
        if (hdr[k] < 1 || hdr[k] > (1 << 16)) return bad_file();
    const size_t G = hdr[0], mp = hdr[1], L = PQP_FALLBACK_DEFAULT_LEVELS;
    const int m = hdr[2], r = hdr[3];
    std::vector<int32_t> prev_m(G), sflags(G), first_hit(G * L), first_collision(G * L);
    std::vector<double> state(G * 8), rows(G * mp * 8);
    if (std::fread(prev_m.data(), 4, G, f) != G || std::fread(sflags.data(), 4, G, f) != G || std::fread(state.data(), 8, state.size(), f) != state.size() ||
        std::fread(rows.data(), 8, rows.size(), f) != rows.size() || std::fread(first_hit.data(), 4, G * L, f) != G * L ||
        std::fread(first_collision.data(), 4, G * L, f) != G * L)
        return bad_file();
    std::fclose(f);
    f = nullptr;
    for (size_t g = 0; g < G; ++g)
        if (prev_m[g] < 0 || (size_t)prev_m[g] > mp) return bad_file();

    FallbackPlanner planner;
    if (!planner.ok()) { std::fprintf(stderr, "no fallback planner: %s\n", pqp_last_error()); return 1; }
    std::vector<std::vector<State>> previous(G);
    std::vector<FallbackPlanner::Start> starts(G);
    for (size_t g = 0; g < G; ++g) {
        previous[g].resize(prev_m[g]);
        for (size_t k = 0; k < previous[g].size(); ++k) {
            const double* q = &rows[(g * mp + k) * 8];
            State& st = previous[g][k];
            st.x = q[0]; st.y = q[1]; st.heading = q[2]; st.k = q[3]; st.s = q[4]; st.v = q[5]; st.a = q[6];
        }
        for (int c = 0; c < 8; ++c) starts[g].row[c] = state[g * 8 + c];
        starts[g].stitch_flags = sflags[g];
    }
    FallbackPlanner::Plans plans;
    std::vector<FallbackPlanner::Result<State>> results;
    if (!planner.brake(previous, starts, dt, r, m, &plans) || !planner.pick(plans, &first_hit, &first_collision, &results)) {
        std::fprintf(stderr, "fallback: %s\n", pqp_last_error());
        return 1;
    }
    for (size_t p = 0; p < G * L; ++p) std::printf("plan %d %d %.17g %.17g\n", plans.flags[p], plans.stop_row[p], plans.stop[2 * p], plans.stop[2 * p + 1]);
    for (size_t g = 0; g < G; ++g) {
        const auto& res = results[g];
        std::printf("group %d %d %zu\n", res.level, res.flags, res.plan.size());
        for (size_t k = 0; k < res.plan.size(); ++k) {
            const State& s = res.plan[k];
            std::printf("row %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", s.x, s.y, s.heading, s.k, s.s, s.v, s.a, res.t[k]);
        }
    }
    return 0;
}
