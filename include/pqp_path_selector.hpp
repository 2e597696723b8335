// pqp_path_selector.hpp — PathOptimizationNS::PathSelector: scores of candidate paths and each group's best over pqp_select_paths.
// Header-only over the C ABI (link libpqp_hip and libamdhip64).  The reference plans one path per call and ranks nothing; the default
// weights are its path QP's own (base_solver.cpp:123-147: 20 on k, 100 on dk), so the best of a group is the candidate that QP would
// rate best.  The selector keeps its own handle.
//
//   selectBest(candidates, group_start, &best, &score)   one call for all groups: best[g] = index of group g's winner or -1
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

class PathSelector {
 public:
    // prm == nullptr: pqp_select_default_params
    explicit PathSelector(const pqp_select_params* prm = nullptr, int device = 0) : h_(device) {
        if (prm) prm_ = *prm; else pqp_select_default_params(&prm_);
    }
    bool ok() const { return h_.ok(); }
    pqp_select_params& params() { return prm_; }

    // candidates of group g: group_start[g] .. group_start[g + 1] - 1 (ascending from 0 to candidates.size()).  best[g]: the index of the
    // group's candidate with the least score among those of two states or more whose score is finite, -1 when there is none.
    // score (optional): every candidate's score.  first_collision (optional, one per candidate, as FootprintChecker::checkPaths gives it):
    // a candidate that collides cannot win while params().require_free is set.  false: a GPU error or a bad argument (pqp_last_error()).
    bool selectBest(const std::vector<std::vector<SlState>>& candidates, const std::vector<int>& group_start, std::vector<int>* best,
                    std::vector<double>* score = nullptr, const std::vector<int>* first_collision = nullptr) {
        if (!ok() || !best || candidates.empty() || group_start.empty() || (first_collision && first_collision->size() != candidates.size()))
            return false;
        const size_t B = candidates.size();
        const int groups = (int)group_start.size() - 1;
        const detail::Packed paths = detail::pack(candidates, PQP_OUT_STRIDE, [](const SlState& s, size_t, double* r) {          // the chain's output row
            r[0] = s.x; r[1] = s.y; r[2] = s.heading; r[3] = s.l; r[4] = s.d_heading; r[5] = s.k; r[6] = s.d_k;
        });
        std::vector<double> terms(B * PQP_SCORE_STRIDE, 0.0);
        std::vector<int32_t> starts(group_start.begin(), group_start.end()), first, won(groups > 0 ? groups : 1, -1);
        if (first_collision) first.assign(first_collision->begin(), first_collision->end());
        if (pqp_select_paths(h_.get(), &prm_, (int)B, (int)paths.n, PQP_OUT_STRIDE, paths.rows.data(), paths.count.data(), nullptr, nullptr,
                             first_collision ? first.data() : nullptr, nullptr, groups, starts.data(), terms.data(), won.data(), nullptr, nullptr) != PQP_OK)
            return false;
        best->assign(won.begin(), won.begin() + groups);
        if (score) {
            score->resize(B);
            for (size_t b = 0; b < B; ++b) (*score)[b] = terms[b * PQP_SCORE_STRIDE];
        }
        return true;
    }

 private:
    detail::OwnedHandle h_;
    pqp_select_params prm_;
};

}  // namespace PathOptimizationNS
