// pqp_fallback_planner.hpp — PathOptimizationNS::FallbackPlanner: a plan for every vehicle in a cycle that ends without a winner, over
// pqp_fallback_rows and pqp_fallback_pick.  Header-only over the C ABI (link libpqp_hip and libamdhip64).  TrajectoryStitcher
// (pqp_trajectory_stitcher.hpp) gives the state a cycle starts from on the previous plan; PlanSelector (pqp_plan_selector.hpp) leaves a
// vehicle none of whose candidates is eligible without a plan.  This brakes such a vehicle along the plan it is already on - or along
// the arc it is on where there is no usable plan - at each of a few braking levels, the acceleration leaving the value it had at the
// seam at a bounded jerk, and takes the gentlest level the caller's checks passed (AgentChecker, FootprintChecker on Plans::rows).  It
// does not steer away and does not re-plan the path.  The reference has no counterpart.  The planner keeps its own handle.
//
//   levels(), a_cap()                               the braking levels (d, j pairs) and the cap on the starting acceleration, to edit
//   brake(previous, starts, dt, r, m, &plans)       one braking plan per vehicle and level
//   pick(plans, first_hit, first_collision, &out)   one trajectory per vehicle: the gentlest level that passed both checks
//
// Not copyable, not thread-safe, no exceptions; without a usable GPU ok() is false and both return false.
#pragma once
#include <cstdint>
#include <vector>

#include "pqp.h"
#ifndef PQP_USE_REFERENCE_TYPES
#include "pqp_types.hpp"
#endif
#include "pqp_wrapper_detail.hpp"

namespace PathOptimizationNS {

class FallbackPlanner {
 public:
    explicit FallbackPlanner(int device = 0) : h_(device) {
        int n = 0;
        levels_.assign(2 * PQP_FALLBACK_DEFAULT_LEVELS, 0.0);
        pqp_fallback_default_params(prm_, levels_.data(), &n);
        levels_.resize(2 * (size_t)n);
    }
    bool ok() const { return h_.ok(); }
    std::vector<double>& levels() { return levels_; }          // d0, j0, d1, j1, ...: d ascending, at most PQP_FALLBACK_MAX_LEVELS pairs
    double& a_cap() { return prm_[PQP_FALLBACK_A_CAP]; }

    struct Start {
        double row[PQP_TRAJ_STRIDE] = {};     // TrajectoryStitcher::Result::row: x, y, heading, k, the station on the previous plan, v, a, t
        int stitch_flags = PQP_STITCH_STITCHED;          // TrajectoryStitcher::Result::flags
    };

    struct Plans {
        int vehicles = 0, levels = 0, rows_per_plan = 0;
        std::vector<double> rows;             // [vehicles][levels][rows_per_plan][PQP_TRAJ_STRIDE], as the checks take them
        std::vector<double> stop;             // [vehicles][levels][2]: the stop time and the distance to the stop
        std::vector<int32_t> stop_row, flags; // [vehicles][levels]
    };

    template <class StateT>
    struct Result {
        std::vector<StateT> plan;             // the braking plan, state f at ...
        std::vector<double> t;                // ... t[f]
        int level = -1;                       // the braking level taken, -1 for a bad state
        int flags = 0;                        // PQP_FALLBACK_*
        bool clear() const { return (flags & (PQP_FALLBACK_BAD | PQP_FALLBACK_NOT_CLEAR)) == 0; }
    };

    // previous: per vehicle the states of its previous plan (what TrajectoryStitcher::stitch took); starts: one per vehicle; m layers of
    // dt with r sub-steps each.  false: a GPU error or a bad argument (pqp_last_error()).
    template <class StateT>
    bool brake(const std::vector<std::vector<StateT>>& previous, const std::vector<Start>& starts, double dt, int r, int m, Plans* plans) {
        const size_t G = previous.size(), L = levels_.size() / 2;
        if (!ok() || !plans || G == 0 || starts.size() != G || L == 0 || r < 1 || m < 1) return false;
        const detail::Packed prev = detail::pack(previous, PQP_TRAJ_STRIDE, detail::TrajRow());
        const size_t mp = prev.n, M = (size_t)(m - 1) * r + 1;
        std::vector<double> state(G * PQP_TRAJ_STRIDE);
        std::vector<int32_t> sflags(G);
        for (size_t g = 0; g < G; ++g) {
            for (int c = 0; c < PQP_TRAJ_STRIDE; ++c) state[g * PQP_TRAJ_STRIDE + c] = starts[g].row[c];
            sflags[g] = starts[g].stitch_flags;
        }
        plans->vehicles = (int)G; plans->levels = (int)L; plans->rows_per_plan = (int)M;
        plans->rows.assign(G * L * M * PQP_TRAJ_STRIDE, 0.0);
        plans->stop.assign(G * L * 2, 0.0);
        plans->stop_row.assign(G * L, 0);
        plans->flags.assign(G * L, 0);
        return pqp_fallback_rows(h_.get(), prm_, (int)L, levels_.data(), dt, r, m, (int)G, (int)mp, PQP_TRAJ_STRIDE, prev.rows.data(), prev.count.data(),
                                 state.data(), sflags.data(), plans->rows.data(), plans->stop.data(), plans->stop_row.data(), plans->flags.data()) == PQP_OK;
    }

    // first_hit / first_collision: AgentChecker's and FootprintChecker's verdicts on the vehicles * levels plans of `plans`, or nullptr
    // where that check was not run
    template <class StateT>
    bool pick(const Plans& plans, const std::vector<int32_t>* first_hit, const std::vector<int32_t>* first_collision, std::vector<Result<StateT>>* results) {
        const size_t G = plans.vehicles, L = plans.levels, M = plans.rows_per_plan;
        if (!ok() || !results || G == 0 || (first_hit && first_hit->size() != G * L) || (first_collision && first_collision->size() != G * L)) return false;
        std::vector<double> final_traj(G * M * PQP_TRAJ_STRIDE);
        std::vector<int32_t> final_m(G), level(G), flags(G);
        if (pqp_fallback_pick(h_.get(), (int)G, (int)L, (int)M, nullptr, nullptr, nullptr, plans.rows.data(), plans.flags.data(),
                              first_hit ? first_hit->data() : nullptr, first_collision ? first_collision->data() : nullptr, final_traj.data(),
                              final_m.data(), level.data(), flags.data()) != PQP_OK)
            return false;
        results->assign(G, Result<StateT>());
        for (size_t g = 0; g < G; ++g) {
            Result<StateT>& out = (*results)[g];
            out.level = level[g];
            out.flags = flags[g];
            for (int f = 0; f < final_m[g]; ++f) {
                const double* q = &final_traj[(g * M + f) * PQP_TRAJ_STRIDE];
                out.plan.push_back(detail::TrajRow::read<StateT>(q));
                out.t.push_back(q[7]);
            }
        }
        return true;
    }

 private:
    detail::OwnedHandle h_;
    double prm_[PQP_FALLBACK_PARAMS];
    std::vector<double> levels_;
};

}  // namespace PathOptimizationNS
