// pqp_frenet_projector.hpp — PathOptimizationNS::FrenetProjector: many points onto one reference line, Cartesian to Frenet, over
// pqp_project_points.  Header-only over the C ABI (link libpqp_hip and libamdhip64).  What the reference does point by point with
// getProjection + global2Local (src/tools/tools.cpp:57-126; path_optimizer.cpp:73-85, reference_path_smoother.cpp:148-165).
// The projector borrows a handle - the planner's own, so the projection runs on that handle's stream and GPU - and keeps a host copy of
// one line's spline table.
//
//   setLine(s, x, y)              the line through the knots, fitted as tk::spline::set_points does (pqp_spline_fit); length = s.back().
//                                 Three knots or more: pqp_spline_fit's minimum, as tk::spline asserts (spline.cpp:164)
//   setTable(spline, ext, length) a line fitted already: [9][m] and [4] as pqp_spline_fit writes them; m >= 2, what pqp_project_points takes
//   project(points, &out)         out[i]: s, l, d_heading of points[i] and x, y, heading, k of the line at s
//
// Not copyable, not thread-safe, no exceptions; every method returns false on a GPU error or a bad argument (pqp_last_error()).
#pragma once
#include <cstdint>
#include <vector>

#include "pqp.h"
#ifndef PQP_USE_REFERENCE_TYPES
#include "pqp_types.hpp"
#endif
#include "pqp_wrapper_detail.hpp"

namespace PathOptimizationNS {

class FrenetProjector {
 public:
    explicit FrenetProjector(pqp_handle& handle) : h_(handle) {}
    FrenetProjector(const FrenetProjector&) = delete;
    FrenetProjector& operator=(const FrenetProjector&) = delete;

    bool setLine(const std::vector<double>& s, const std::vector<double>& x, const std::vector<double>& y) {
        const size_t m = s.size();
        if (m < 3 || x.size() != m || y.size() != m) return false;
        std::vector<double> tab(9 * m), ext(4);
        if (pqp_spline_fit(&h_, 1, (int)m, s.data(), x.data(), y.data(), tab.data(), ext.data()) != PQP_OK) return false;
        tab_.swap(tab); ext_.swap(ext);
        length_ = s.back();
        return true;
    }
    bool setTable(const std::vector<double>& spline, const std::vector<double>& spline_ext, double length) {
        if (spline.size() < 18 || spline.size() % 9 != 0 || spline_ext.size() != 4) return false;
        tab_ = spline; ext_ = spline_ext; length_ = length;
        return true;
    }
    double length() const { return length_; }

    // out[i]: s, l (positive to the left), d_heading = constrainAngle(points[i].heading - heading) and the line's x, y, heading, k at s.
    // flags (optional): PQP_PROJ_* of every point - a point that is not finite comes back as NaNs with PQP_PROJ_NOT_FINITE.
    // along (optional): the distance along the tangent, non-zero only where the projection was clipped at the line's end.
    bool project(const std::vector<State>& points, std::vector<SlState>* out, std::vector<int>* flags = nullptr, std::vector<double>* along = nullptr) {
        if (!out || tab_.empty() || points.empty()) return false;
        const size_t q = points.size();
        std::vector<double> in(q * 3), proj(q * PQP_PROJ_STRIDE);
        std::vector<int32_t> fl(q);
        for (size_t i = 0; i < q; ++i) detail::PoseRow()(points[i], i, &in[i * 3]);
        if (pqp_project_points(&h_, 1, (int)(tab_.size() / 9), tab_.data(), ext_.data(), &length_, (int)q, 3, 1, in.data(), nullptr, proj.data(),
                               fl.data()) != PQP_OK)
            return false;
        out->assign(q, SlState());
        if (along) along->resize(q);
        for (size_t i = 0; i < q; ++i) {
            const double* p = &proj[i * PQP_PROJ_STRIDE];           // s, l, along, d_heading, then the line's x, y, heading, k at s
            SlState& o = (*out)[i];
            o.s = p[0]; o.l = p[1]; o.d_heading = p[3]; o.x = p[4]; o.y = p[5]; o.heading = p[6]; o.k = p[7];
            if (along) (*along)[i] = p[2];
        }
        if (flags) flags->assign(fl.begin(), fl.end());
        return true;
    }

 private:
    pqp_handle& h_;
    std::vector<double> tab_, ext_;
    double length_ = 0.0;
};

}  // namespace PathOptimizationNS
