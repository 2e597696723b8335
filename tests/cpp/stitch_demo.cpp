// PathOptimizationNS::TrajectoryStitcher (include/pqp_trajectory_stitcher.hpp) from C++ (tests/test_stitch_trajectory.py,
// tests/test_gpu_stitch_trajectory.py).  Reads a binary file (tests/stitch_util.py's write_case):
//   int32 G, m; double dt; int32 m_of [G]; double meas [G][6]; double t_now [G];
//   double prev [G][m][8] = x, y, heading, k, s, v, a, t (t is not read: state f is at f * dt)
// and prints per vehicle "group <flags> <prefix_n>", "state <eight %.17g>", "dev <three %.17g>" and one "prefix <eight %.17g>" per state
// of the piece.  Exit 1 without a usable GPU, 2 on a short or bad file.
#include <cstdio>
#include <vector>

#include "../../include/pqp_trajectory_stitcher.hpp"

using PathOptimizationNS::State;
using PathOptimizationNS::TrajectoryStitcher;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: stitch_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    const auto bad_file = [&]() { if (f) std::fclose(f); std::fprintf(stderr, "stitch_demo: short or bad file\n"); return 2; };
    int32_t hdr[2];
    double dt;
    if (std::fread(hdr, 4, 2, f) != 2 || std::fread(&dt, 8, 1, f) != 1 || hdr[0] < 1 || hdr[1] < 1 || hdr[0] > (1 << 20) || hdr[1] > (1 << 20))
        return bad_file();
    const size_t G = hdr[0], m = hdr[1];
    std::vector<int32_t> m_of(G);
    std::vector<double> meas(G * 6), t_now(G), rows(G * m * 8);
    if (std::fread(m_of.data(), 4, G, f) != G || std::fread(meas.data(), 8, meas.size(), f) != meas.size() || std::fread(t_now.data(), 8, G, f) != G ||
        std::fread(rows.data(), 8, rows.size(), f) != rows.size())
        return bad_file();
    std::fclose(f);
    f = nullptr;
    for (size_t g = 0; g < G; ++g)
        if (m_of[g] < 0 || (size_t)m_of[g] > m) return bad_file();

    TrajectoryStitcher stitcher;
    if (!stitcher.ok()) { std::fprintf(stderr, "no trajectory stitcher: %s\n", pqp_last_error()); return 1; }
    std::vector<std::vector<State>> previous(G);
    std::vector<TrajectoryStitcher::Measured> measured(G);
    for (size_t g = 0; g < G; ++g) {
        previous[g].resize(m_of[g]);
        for (size_t k = 0; k < previous[g].size(); ++k) {
            const double* r = &rows[(g * m + k) * 8];
            State& st = previous[g][k];
            st.x = r[0]; st.y = r[1]; st.heading = r[2]; st.k = r[3]; st.s = r[4]; st.v = r[5]; st.a = r[6];
        }
        const double* q = &meas[g * 6];
        TrajectoryStitcher::Measured& c = measured[g];
        c.x = q[0]; c.y = q[1]; c.heading = q[2]; c.v = q[3]; c.a = q[4]; c.yaw_rate = q[5]; c.t = t_now[g];
    }
    std::vector<TrajectoryStitcher::Result<State>> results;
    if (!stitcher.stitch(previous, dt, measured, &results)) {
        std::fprintf(stderr, "stitch: %s\n", pqp_last_error());
        return 1;
    }
    for (size_t g = 0; g < G; ++g) {
        const auto& r = results[g];
        std::printf("group %d %zu\nstate", r.flags, r.prefix.size());
        for (int c = 0; c < 8; ++c) std::printf(" %.17g", r.row[c]);
        std::printf("\ndev %.17g %.17g %.17g\n", r.lon, r.lat, r.dh);
        for (size_t j = 0; j < r.prefix.size(); ++j) {
            const State& s = r.prefix[j];
            std::printf("prefix %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", s.x, s.y, s.heading, s.k, s.s, s.v, s.a, r.prefix_t[j]);
        }
    }
    return 0;
}
