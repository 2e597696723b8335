// pqp_speed_profiler.hpp — PathOptimizationNS::SpeedProfiler: planned paths to trajectories over pqp_speed_profile.  Header-only over the
// C ABI (link libpqp_hip and libamdhip64).  The reference's State carries s, v and a (include/data_struct/data_struct.hpp:14-26) and
// nothing fills them; getOptimizedPath adds the chords up in tmp_s and drops the sum (src/solver/base_solver.cpp:268,282-284).  This fills
// them, for many paths per call: s along the path's own chords, v under the curvature and acceleration limits, a between waypoints.
// The profiler borrows a handle - the planner's own, so the profile runs on that handle's stream and GPU.
//
//   params()                       pqp_speed_params to edit (pqp_speed_default_params: this library's choice, the reference has no such flags)
//   profile(&paths, v_start, ...)  fills State::s, v, a of every state that is driven; the optional arguments are pqp_speed_profile's
//
// Not copyable, not thread-safe, no exceptions; profile() returns false on a GPU error or a bad argument (pqp_last_error()).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "pqp.h"
#ifndef PQP_USE_REFERENCE_TYPES
#include "pqp_types.hpp"
#endif
#include "pqp_wrapper_detail.hpp"

namespace PathOptimizationNS {

class SpeedProfiler {
 public:
    explicit SpeedProfiler(pqp_handle& handle) : h_(handle) { pqp_speed_default_params(&prm_); }
    SpeedProfiler(const SpeedProfiler&) = delete;
    SpeedProfiler& operator=(const SpeedProfiler&) = delete;

    pqp_speed_params& params() { return prm_; }

    // paths: x, y and k of every state are read; s, v, a of the states that are driven are written (a state behind an early stop, or
    //        any state of a path flagged PQP_SPEED_NOT_FINITE, is left as it was)
    // v_start [paths]: the speed at each path's first state
    // times (optional): t of every state of every path, 0 where it is not driven
    // flags (optional): PQP_SPEED_* of every path
    // stop_before (optional, [paths]): e.g. FootprintChecker's first collision index - the path is driven up to the state before it and
    //        ends at speed 0 there
    // v_end (optional, [paths]): the speed at the last driven state; NaN: free
    // v_limit (optional, like paths): a cap per state
    bool profile(std::vector<std::vector<SlState>>* paths, const std::vector<double>& v_start, std::vector<std::vector<double>>* times = nullptr,
                 std::vector<int>* flags = nullptr, const std::vector<int>* stop_before = nullptr, const std::vector<double>* v_end = nullptr,
                 const std::vector<std::vector<double>>* v_limit = nullptr) {
        if (!paths || paths->empty()) return false;
        const size_t B = paths->size();
        if (v_start.size() != B || (stop_before && stop_before->size() != B) || (v_end && v_end->size() != B) || (v_limit && v_limit->size() != B))
            return false;
        for (size_t b = 0; v_limit && b < B; ++b)
            if ((*v_limit)[b].size() != (*paths)[b].size()) return false;
        const detail::Packed in = detail::pack(*paths, 6, detail::PathRow{false});
        const size_t n = in.n;
        detail::Packed lim;
        if (v_limit) lim = detail::pack(*v_limit, 1, [](double v, size_t, double* r) { *r = v; });
        std::vector<double> prof(B * n * PQP_SPEED_STRIDE);
        std::vector<int32_t> stop, fl(B);
        if (stop_before) stop.assign(stop_before->begin(), stop_before->end());
        if (pqp_speed_profile(&h_, &prm_, (int)B, (int)n, 6, in.rows.data(), in.count.data(), stop_before ? stop.data() : nullptr,
                              v_limit ? lim.rows.data() : nullptr, v_start.data(), v_end ? v_end->data() : nullptr, prof.data(), fl.data()) != PQP_OK)
            return false;
        if (times) times->assign(B, std::vector<double>());
        for (size_t b = 0; b < B; ++b) {
            auto& p = (*paths)[b];
            const size_t driven = (fl[b] & PQP_SPEED_NOT_FINITE) ? 0
                                  : stop_before ? std::min(p.size(), (size_t)std::max((*stop_before)[b], 0)) : p.size();
            if (times) (*times)[b].assign(p.size(), 0.0);
            for (size_t i = 0; i < driven; ++i) {
                const double* r = &prof[(b * n + i) * PQP_SPEED_STRIDE];
                detail::ProfileRow::read(r, &p[i]);
                if (times) (*times)[b][i] = r[3];
            }
        }
        if (flags) flags->assign(fl.begin(), fl.end());
        return true;
    }

 private:
    pqp_handle& h_;
    pqp_speed_params prm_;
};

}  // namespace PathOptimizationNS
