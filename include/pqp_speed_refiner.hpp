// pqp_speed_refiner.hpp — PathOptimizationNS::SpeedRefiner: searched speed plans made drivable, over pqp_speed_refine.
// Header-only over the C ABI (link libpqp_hip and libamdhip64).  SpeedSearcher (pqp_speed_searcher.hpp) decides who yields, on a grid:
// whole cells of ds, whole cells per layer.  This runs that search and, behind it, the jerk-limited speed QP in the corridor the search's
// own occupancy leaves free around its plan: per path a state for every layer with s, v and a that follow constant-acceleration
// kinematics inside the limits.  A path the search does not get through, or whose QP has no feasible point, keeps the searched states.
// The refiner borrows a searcher - its handle, its grid, its car.
//
//   params()                              the PQP_REFINE_PARAMS doubles to edit, by PQP_REFINE_W_REF .. PQP_REFINE_D_MAX
//   window()                              the corridor's half-width in cells, to edit
//   refine(paths, v_start, scenes, ...)   per path the states of every layer, PQP_REFINE_* flags, the QP's status, cost and excess
//   refine_raw(...)                       the same calls with the C ABI's arrays left to the caller (PlanSampler's input)
//
// Not copyable, not thread-safe, no exceptions; refine() returns false on a GPU error or a bad argument (pqp_last_error()).
#pragma once
#include <cstdint>
#include <vector>

#include "pqp.h"
#include "pqp_speed_searcher.hpp"

namespace PathOptimizationNS {

class SpeedRefiner {
 public:
    explicit SpeedRefiner(SpeedSearcher& searcher) : searcher_(searcher) { pqp_refine_default_params(prm_, &window_); }
    SpeedRefiner(const SpeedRefiner&) = delete;
    SpeedRefiner& operator=(const SpeedRefiner&) = delete;

    double* params() { return prm_; }
    int& window() { return window_; }

    struct Result {
        int flags = 0;                    // PQP_REFINE_*
        int status = 0;                   // pqp_status of the QP (PQP_STATUS_UNSOLVED: the path never got to it)
        int search_flags = 0;             // PQP_SEARCH_*
        double cost = 0.0, excess = 0.0;  // NaN for a path that is kept
        std::vector<double> lo, hi, vcap; // the corridor of every layer; zeros for a path that is kept
    };

    // what the two calls wrote, as the C ABI has it (PlanSampler's input): the search's arrays, then pqp_speed_refine's
    struct Raw {
        SpeedSearcher::Raw search;
        std::vector<double> traj, bounds, cost, excess;     // [B][m][8], [B][m][3], [B], [B]
        std::vector<int32_t> status, iters, flags;          // [B]
    };

    // paths, v_start, scenes, scene_of, layers: SpeedSearcher::search's
    // results: per path the outcome; states: per path the state of every layer the search reached - x, y, heading, k, s, v, a
    template <class StateT>
    bool refine(const std::vector<std::vector<StateT>>& paths, const std::vector<double>& v_start,
                const std::vector<std::vector<std::vector<PredictedAgent>>>& scenes, std::vector<Result>* results,
                std::vector<std::vector<StateT>>* states, const std::vector<int>* scene_of = nullptr, int layers = 1) {
        Raw raw;
        if (!results || !states || !refine_raw(paths, v_start, scenes, scene_of, layers, &raw)) return false;
        const size_t B = raw.search.B, m = raw.search.m;
        results->assign(B, Result());
        detail::read_trajectories(raw.traj, m, raw.search.reached, states);
        for (size_t b = 0; b < B; ++b) {
            Result& r = (*results)[b];
            r.flags = raw.flags[b]; r.status = raw.status[b]; r.search_flags = raw.search.flags[b]; r.cost = raw.cost[b]; r.excess = raw.excess[b];
            for (size_t k = 0; k < m; ++k) {
                const double* c = &raw.bounds[(b * m + k) * 3];
                r.lo.push_back(c[0]); r.hi.push_back(c[1]); r.vcap.push_back(c[2]);
            }
        }
        return true;
    }

    // the same two calls with the C ABI's arrays left to the caller
    template <class StateT>
    bool refine_raw(const std::vector<std::vector<StateT>>& paths, const std::vector<double>& v_start,
                    const std::vector<std::vector<std::vector<PredictedAgent>>>& scenes, const std::vector<int>* scene_of, int layers, Raw* out) {
        if (!out || !searcher_.search_raw(paths, v_start, scenes, scene_of, layers, true, &out->search)) return false;
        const SpeedSearcher::Raw& raw = out->search;
        const size_t B = raw.B, m = raw.m;
        out->traj.assign(B * m * PQP_TRAJ_STRIDE, 0.0); out->bounds.assign(B * m * 3, 0.0); out->cost.assign(B, 0.0); out->excess.assign(B, 0.0);
        out->status.assign(B, 0); out->iters.assign(B, 0); out->flags.assign(B, 0);
        return pqp_speed_refine(&searcher_.handle(), &searcher_.params(), prm_, window_, (int)B, (int)raw.n, 6, raw.rows.data(), raw.n_of.data(), nullptr,
                                raw.profile.data(), v_start.data(), (int)m, raw.blocked.data(), raw.steps.data(), raw.reached.data(), raw.traj.data(),
                                out->traj.data(), out->bounds.data(), out->cost.data(), out->excess.data(), out->status.data(), out->iters.data(),
                                out->flags.data()) == PQP_OK;
    }

    SpeedSearcher& searcher() { return searcher_; }

 private:
    SpeedSearcher& searcher_;
    double prm_[PQP_REFINE_PARAMS];
    int window_ = 0;
};

}  // namespace PathOptimizationNS
