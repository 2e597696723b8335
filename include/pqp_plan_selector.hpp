// pqp_plan_selector.hpp — PathOptimizationNS::PlanSelector: scores of finished trajectories and each group's best over pqp_select_plans.
// Header-only over the C ABI (link libpqp_hip and libamdhip64).  PathSelector (pqp_path_selector.hpp) chooses between the candidates of a
// vehicle by their paths alone, before a speed is planned; this chooses behind SpeedSearcher, SpeedRefiner and PlanSampler, by the path and
// the speed plan on it together: progress, acceleration effort and jumps, lateral acceleration, clearance to the agents and the path's own
// score.  The reference plans one path per call and has no time axis: it ranks nothing.  The selector keeps its own handle.
//
//   weights()                                          the PQP_RANK_PARAMS doubles, to edit (pqp_rank_default_params)
//   require_free()                                     1: a trajectory that is hit cannot win
//   selectBest(trajectories, dt, group_start, &best)   one call for all groups: best[g] = index of group g's winner or -1
//
// Not copyable, not thread-safe, no exceptions; without a usable GPU ok() is false and selectBest returns false.
#pragma once
#include <cstdint>
#include <vector>

#include "pqp.h"
#ifndef PQP_USE_REFERENCE_TYPES
#include "pqp_types.hpp"
#endif
#include "pqp_wrapper_detail.hpp"

namespace PathOptimizationNS {

class PlanSelector {
 public:
    explicit PlanSelector(int device = 0) : h_(device) { pqp_rank_default_params(prm_, &require_free_); }
    bool ok() const { return h_.ok(); }
    double* weights() { return prm_; }
    int& require_free() { return require_free_; }

    struct Optional {
        const std::vector<double>* path_score = nullptr;      // one per candidate: PathSelector::selectBest's score
        const std::vector<int>* search_flags = nullptr;       // one per candidate: SpeedSearcher's PQP_SEARCH_* flags
        const std::vector<int>* first_hit = nullptr;          // one per candidate, as AgentChecker gives it on these states
    };

    // trajectories: per candidate its states, state f at time f * dt (PlanSampler::sample's states and Result::dt; or the layers of
    // SpeedRefiner, dt the grid's).  Candidates of group g: group_start[g] .. group_start[g + 1] - 1 (ascending from 0 to
    // trajectories.size()).  best[g]: the index of the group's eligible candidate with the least score, -1 when there is none.
    // terms (optional): every candidate's PQP_PLAN_SCORE_STRIDE entries, the score first.  winners (optional): per group the winner's
    // states, empty without a winner.  false: a GPU error or a bad argument (pqp_last_error()).
    template <class StateT>
    bool selectBest(const std::vector<std::vector<StateT>>& trajectories, double dt, const std::vector<int>& group_start, std::vector<int>* best,
                    std::vector<double>* terms = nullptr, std::vector<std::vector<StateT>>* winners = nullptr, const Optional& opt = Optional()) {
        const size_t B = trajectories.size();
        if (!ok() || !best || B == 0 || group_start.empty() || (opt.path_score && opt.path_score->size() != B) ||
            (opt.search_flags && opt.search_flags->size() != B) || (opt.first_hit && opt.first_hit->size() != B))
            return false;
        const int batch = (int)B, groups = (int)group_start.size() - 1;
        const detail::Packed traj = detail::pack(trajectories, PQP_TRAJ_STRIDE, detail::TimedTrajRow{dt});
        const size_t m = traj.n, G = groups > 0 ? groups : 1;
        std::vector<double> rec(B * PQP_PLAN_SCORE_STRIDE, 0.0), path_terms, won_rows(G * m * PQP_TRAJ_STRIDE, 0.0);
        std::vector<int32_t> starts(group_start.begin(), group_start.end()), sflags, first, won(G, -1), won_m(G, 0);
        if (opt.path_score) {
            path_terms.assign(B * PQP_SCORE_STRIDE, 0.0);
            for (size_t b = 0; b < B; ++b) { path_terms[b * PQP_SCORE_STRIDE] = (*opt.path_score)[b]; path_terms[b * PQP_SCORE_STRIDE + 7] = 1.0; }
        }
        if (opt.search_flags) sflags.assign(opt.search_flags->begin(), opt.search_flags->end());
        if (opt.first_hit) first.assign(opt.first_hit->begin(), opt.first_hit->end());
        if (pqp_select_plans(h_.get(), prm_, require_free_, batch, (int)m, PQP_TRAJ_STRIDE, traj.rows.data(), traj.count.data(),
                             opt.path_score ? path_terms.data() : nullptr, opt.search_flags ? sflags.data() : nullptr, opt.first_hit ? first.data() : nullptr,
                             nullptr, 0, 0, nullptr, nullptr, groups, starts.data(), rec.data(), won.data(), won_rows.data(), won_m.data(), nullptr,
                             nullptr) != PQP_OK)
            return false;
        best->assign(won.begin(), won.begin() + groups);
        if (terms) *terms = rec;
        won_m.resize(groups);
        if (winners) detail::read_trajectories(won_rows, m, won_m, winners);
        return true;
    }

 private:
    detail::OwnedHandle h_;
    double prm_[PQP_RANK_PARAMS];
    int require_free_ = 1;
};

}  // namespace PathOptimizationNS
