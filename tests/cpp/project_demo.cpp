// PathOptimizationNS::FrenetProjector (include/pqp_frenet_projector.hpp) from C++ (tests/test_project_points.py,
// tests/test_gpu_project_points.py).  Reads a binary file:
//   int32 m, q; double s [m], x [m], y [m] (the line's knots); double [q][3] x, y, heading (the points)
// and prints one line per point: s l d_heading x y heading k (%.17g each), the distance along the tangent, the flags.
// Exit 1 without a usable GPU.
#include <cstdio>
#include <vector>

#include "../../include/pqp_frenet_projector.hpp"

using PathOptimizationNS::FrenetProjector;
using PathOptimizationNS::SlState;
using PathOptimizationNS::State;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: project_demo <file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    const auto bad_file = [&]() { std::fclose(f); std::fprintf(stderr, "project_demo: short or bad file\n"); return 2; };
    int32_t hdr[2];
    if (std::fread(hdr, 4, 2, f) != 2 || hdr[0] < 3 || hdr[1] < 1) return bad_file();
    const size_t m = hdr[0], q = hdr[1];
    std::vector<double> s(m), x(m), y(m), p(3 * q);
    if (std::fread(s.data(), 8, m, f) != m || std::fread(x.data(), 8, m, f) != m || std::fread(y.data(), 8, m, f) != m ||
        std::fread(p.data(), 8, 3 * q, f) != 3 * q)
        return bad_file();
    std::fclose(f);

    pqp_handle* h = nullptr;
    if (pqp_create(&h, nullptr, 0, 1, 2) != PQP_OK) { std::fprintf(stderr, "no projector: %s\n", pqp_last_error()); return 1; }
    int rc = 0;
    {
        FrenetProjector projector(*h);
        std::vector<State> points;
        for (size_t i = 0; i < q; ++i) points.emplace_back(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
        std::vector<SlState> out;
        std::vector<int> flags;
        std::vector<double> along;
        if (!projector.setLine(s, x, y) || !projector.project(points, &out, &flags, &along)) {
            std::fprintf(stderr, "project: %s\n", pqp_last_error());
            rc = 1;
        } else {
            for (size_t i = 0; i < q; ++i)
                std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d\n", out[i].s, out[i].l, out[i].d_heading, out[i].x, out[i].y,
                            out[i].heading, out[i].k, along[i], flags[i]);
        }
    }
    pqp_destroy(h);
    return rc;
}
