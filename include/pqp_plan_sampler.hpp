// pqp_plan_sampler.hpp — PathOptimizationNS::PlanSampler: speed plans on a fine time step, over pqp_sample_plan.
// Header-only over the C ABI (link libpqp_hip and libamdhip64).  SpeedSearcher (pqp_speed_searcher.hpp) and SpeedRefiner
// (pqp_speed_refiner.hpp) write a plan as one state per layer, dt apart.  This runs both and puts the plan they end with on r sub-steps
// per layer: a refined path under its constant-acceleration kinematics, a path that kept the search's staircase linearly.  The fine states
// are what a controller tracks, and what AgentChecker (pqp_agent_checker.hpp) takes to judge the plan between the layers as well.
// The sampler borrows a refiner - and through it the searcher, its handle, its grid, its car.
//
//   sub_steps()                           r, the sub-steps per layer, to edit (10)
//   sample(paths, v_start, scenes, ...)   per path the fine states, PQP_PLAN_* flags, the defect and the excess
//
// Not copyable, not thread-safe, no exceptions; sample() returns false on a GPU error or a bad argument (pqp_last_error()).
#pragma once
#include <cstdint>
#include <vector>

#include "pqp.h"
#include "pqp_speed_refiner.hpp"

namespace PathOptimizationNS {

class PlanSampler {
 public:
    explicit PlanSampler(SpeedRefiner& refiner) : refiner_(refiner) {}
    PlanSampler(const PlanSampler&) = delete;
    PlanSampler& operator=(const PlanSampler&) = delete;

    int& sub_steps() { return r_; }

    struct Result {
        int flags = 0;                    // PQP_PLAN_*
        int refine_flags = 0;             // PQP_REFINE_*: REFINED - sampled under constant acceleration; otherwise linearly
        int search_flags = 0;             // PQP_SEARCH_*
        int layers = 0;                   // the layers the search reached
        double dt = 0.0;                  // the time between two fine states: the grid's dt / r
        double defect = 0.0, excess = 0.0;      // NaN for a path without samples
    };

    // paths, v_start, scenes, scene_of, layers: SpeedSearcher::search's
    // results: per path the outcome; states: per path the fine states on the plan, (layers - 1) r + 1 of them, state f at time f * dt -
    // x, y, heading, k, s, v, a
    template <class StateT>
    bool sample(const std::vector<std::vector<StateT>>& paths, const std::vector<double>& v_start,
                const std::vector<std::vector<std::vector<PredictedAgent>>>& scenes, std::vector<Result>* results,
                std::vector<std::vector<StateT>>* states, const std::vector<int>* scene_of = nullptr, int layers = 1) {
        SpeedRefiner::Raw raw;
        if (!results || !states || !refiner_.refine_raw(paths, v_start, scenes, scene_of, layers, &raw)) return false;
        const SpeedSearcher::Raw& se = raw.search;
        const size_t B = se.B, m = se.m;
        const double dt = refiner_.searcher().params().dt;
        if (r_ < 1 || (m - 1) > (size_t)(INT32_MAX - 1) / (size_t)r_) {       // no vector is sized by such an r: the library's refusal, for its message
            (void)pqp_sample_plan(&refiner_.searcher().handle(), dt, r_, 0, (int)B, (int)se.n, 6, se.rows.data(), se.n_of.data(), nullptr,
                                  se.profile.data(), (int)m, raw.traj.data(), se.reached.data(), raw.flags.data(), nullptr, nullptr, nullptr, nullptr,
                                  nullptr);
            return false;
        }
        const size_t M = (m - 1) * (size_t)r_ + 1;
        std::vector<double> fine(B * M * PQP_TRAJ_STRIDE), defect(B), excess(B);
        std::vector<int32_t> m_of(B), flags(B);
        if (pqp_sample_plan(&refiner_.searcher().handle(), dt, r_, 0, (int)B, (int)se.n, 6, se.rows.data(), se.n_of.data(), nullptr, se.profile.data(),
                            (int)m, raw.traj.data(), se.reached.data(), raw.flags.data(), fine.data(), m_of.data(), defect.data(), excess.data(),
                            flags.data()) != PQP_OK)
            return false;
        results->assign(B, Result());
        detail::read_trajectories(fine, M, m_of, states);
        for (size_t b = 0; b < B; ++b) {
            Result& r = (*results)[b];
            r.flags = flags[b]; r.refine_flags = raw.flags[b]; r.search_flags = se.flags[b]; r.layers = se.reached[b]; r.dt = dt / (double)r_;
            r.defect = defect[b]; r.excess = excess[b];
        }
        return true;
    }

 private:
    SpeedRefiner& refiner_;
    int r_ = 10;
};

}  // namespace PathOptimizationNS
