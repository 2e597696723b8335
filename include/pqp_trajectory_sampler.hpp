// pqp_trajectory_sampler.hpp — PathOptimizationNS::TrajectorySampler: time-stamped trajectories at a fixed time step over
// pqp_sample_trajectory.  Header-only over the C ABI (link libpqp_hip and libamdhip64).  SpeedProfiler (pqp_speed_profiler.hpp) fills
// State::s, v, a of every waypoint and hands out the time stamps; a controller, a simulator step or an MPC horizon asks where the car is at
// t0 + k dt.  This answers that for many paths per call, with the profile's own kinematics: constant acceleration along each chord.
// The sampler borrows a handle - the planner's own, so the samples are taken on that handle's stream and GPU.
//
//   params()                              pqp_sample_params to edit (pqp_sample_default_params: dt 0.1 s, hold_last 0)
//   sample(paths, times, m, &samples...)  the states at t0 + k dt, k < m; the optional arguments are pqp_sample_trajectory's
//
// Not copyable, not thread-safe, no exceptions; sample() returns false on a GPU error or a bad argument (pqp_last_error()).
#pragma once
#include <cstdint>
#include <vector>

#include "pqp.h"
#ifndef PQP_USE_REFERENCE_TYPES
#include "pqp_types.hpp"
#endif
#include "pqp_wrapper_detail.hpp"

namespace PathOptimizationNS {

class TrajectorySampler {
 public:
    explicit TrajectorySampler(pqp_handle& handle) : h_(handle) { pqp_sample_default_params(&prm_); }
    TrajectorySampler(const TrajectorySampler&) = delete;
    TrajectorySampler& operator=(const TrajectorySampler&) = delete;

    pqp_sample_params& params() { return prm_; }

    // paths: State or SlState with x, y, heading, k and - from SpeedProfiler::profile - s, v, a filled
    // times [paths][states]: SpeedProfiler's `times`
    // m: samples per path
    // samples: of every path the states at t0 + k dt that lie on it (x, y, heading, k, s, v, a); with params().hold_last all m, the ones
    //        behind the arrival at rest at the last driven state.  None for a path flagged PQP_TRAJ_EMPTY or PQP_TRAJ_NOT_FINITE
    // sample_times (optional): t0 + k dt of every state in `samples`
    // flags (optional): PQP_TRAJ_* of every path
    // stop_before (optional, [paths]): what SpeedProfiler::profile got - the states from that index on are not driven
    // t0 (optional, [paths]): the time of sample 0; absent: 0
    template <class StateT>
    bool sample(const std::vector<std::vector<StateT>>& paths, const std::vector<std::vector<double>>& times, int m,
                std::vector<std::vector<State>>* samples, std::vector<std::vector<double>>* sample_times = nullptr, std::vector<int>* flags = nullptr,
                const std::vector<int>* stop_before = nullptr, const std::vector<double>* t0 = nullptr) {
        if (!samples || paths.empty() || m < 1) return false;
        const size_t B = paths.size();
        if (times.size() != B || (stop_before && stop_before->size() != B) || (t0 && t0->size() != B)) return false;
        for (size_t b = 0; b < B; ++b)
            if (times[b].size() != paths[b].size()) return false;
        const detail::Packed in = detail::pack(paths, 6, detail::PathRow());
        detail::Packed prof = detail::pack(paths, PQP_SPEED_STRIDE, detail::ProfileRow());
        const size_t n = in.n;
        for (size_t b = 0; b < B; ++b)
            for (size_t i = 0; i < times[b].size(); ++i) prof.rows[(b * n + i) * PQP_SPEED_STRIDE + 3] = times[b][i];
        std::vector<double> traj(B * (size_t)m * PQP_TRAJ_STRIDE);
        std::vector<int32_t> stop, m_of(B), fl(B);
        if (stop_before) stop.assign(stop_before->begin(), stop_before->end());
        if (pqp_sample_trajectory(&h_, &prm_, (int)B, (int)n, 6, in.rows.data(), in.count.data(), stop_before ? stop.data() : nullptr, prof.rows.data(),
                                  t0 ? t0->data() : nullptr, m, traj.data(), m_of.data(), fl.data()) != PQP_OK)
            return false;
        samples->assign(B, std::vector<State>());
        if (sample_times) sample_times->assign(B, std::vector<double>());
        for (size_t b = 0; b < B; ++b) {
            const bool none = (fl[b] & (PQP_TRAJ_EMPTY | PQP_TRAJ_NOT_FINITE)) != 0;
            const size_t rows = none ? 0 : prm_.hold_last ? (size_t)m : (size_t)m_of[b];
            (*samples)[b].resize(rows);
            if (sample_times) (*sample_times)[b].resize(rows);
            for (size_t k = 0; k < rows; ++k) {
                const double* r = &traj[(b * (size_t)m + k) * PQP_TRAJ_STRIDE];
                (*samples)[b][k] = detail::TrajRow::read<State>(r);
                if (sample_times) (*sample_times)[b][k] = r[7];
            }
        }
        if (flags) flags->assign(fl.begin(), fl.end());
        return true;
    }

 private:
    pqp_handle& h_;
    pqp_sample_params prm_;
};

}  // namespace PathOptimizationNS
