// pqp_agent_checker.hpp — PathOptimizationNS::AgentChecker: sampled trajectories against predicted moving agents over pqp_agents_check.
// Header-only over the C ABI (link libpqp_hip and libamdhip64).  TrajectorySampler (pqp_trajectory_sampler.hpp) hands out the states at
// t0 + k dt; a prediction module hands out where the other vehicles and pedestrians are at those times.  This says, for many
// trajectories per call, whether the car's six-circle footprint comes within a margin of one of them, at which sample, and which one.
// The checker borrows a handle - the planner's own, so the check runs on that handle's stream and GPU.
//
//   params()                              the check's parameters to edit: margin (pqp_agents_default_params: 0 m)
//   car()                                 pqp_car_geometry to edit (pqp_car_default_geometry: the reference's flags)
//   check(trajectories, scenes, ...)      first hit sample, hitting agent and (optionally) the clearance of every sample
//
// Not copyable, not thread-safe, no exceptions; check() returns false on a GPU error or a bad argument (pqp_last_error()).
#pragma once
#include <cstdint>
#include <vector>

#include "pqp.h"
#ifndef PQP_USE_REFERENCE_TYPES
#include "pqp_types.hpp"
#endif
#include "pqp_wrapper_detail.hpp"          // PredictedAgent

namespace PathOptimizationNS {

class AgentChecker {
 public:
    explicit AgentChecker(pqp_handle& handle) : h_(handle) {
        pqp_agents_default_params(&prm_.margin);
        pqp_car_default_geometry(&car_);
    }
    AgentChecker(const AgentChecker&) = delete;
    AgentChecker& operator=(const AgentChecker&) = delete;

    struct Params { double margin; };     // m, finite, >= 0: the distance demanded beyond touching
    Params& params() { return prm_; }
    pqp_car_geometry& car() { return car_; }

    // trajectories: State or SlState with x, y, heading - sample k of each at the k-th time step (TrajectorySampler::sample's `samples`)
    // scenes [scene][agent][step]: the predicted agents; an agent with fewer steps than a trajectory is absent behind its last one
    // first_hit: of every trajectory the first sample that comes within params().margin of an agent (or is not finite), its size when none
    // hit_agent: the lowest index of an agent hit at that sample; -1 when there is no hit or the sample itself is not finite
    // clearance (optional): of every sample the least distance between the footprint and an agent, +inf where none is present
    // scene_of (optional, [trajectories]): the scene every trajectory is checked against; absent: scene 0
    template <class StateT>
    bool check(const std::vector<std::vector<StateT>>& trajectories, const std::vector<std::vector<std::vector<PredictedAgent>>>& scenes,
               std::vector<int>* first_hit, std::vector<int>* hit_agent, std::vector<std::vector<double>>* clearance = nullptr,
               const std::vector<int>* scene_of = nullptr) {
        if (!first_hit || !hit_agent || trajectories.empty() || scenes.empty()) return false;
        const size_t B = trajectories.size(), S = scenes.size();
        if (scene_of && scene_of->size() != B) return false;
        const detail::Packed traj = detail::pack(trajectories, 3, detail::PoseRow());
        const size_t m = traj.n;
        const detail::AgentRows ag = detail::pack_agents(scenes, m);
        std::vector<double> clear(clearance ? B * m : 0);
        std::vector<int32_t> scene, first(B), who(B);
        if (scene_of) scene.assign(scene_of->begin(), scene_of->end());
        if (pqp_agents_check(&h_, prm_.margin, &car_, (int)B, (int)m, 3, traj.rows.data(), traj.count.data(), (int)S, (int)ag.a_max,
                             ag.a_max ? ag.rows.data() : nullptr, ag.a_of.data(), scene_of ? scene.data() : nullptr, first.data(), who.data(),
                             clearance ? clear.data() : nullptr) != PQP_OK)
            return false;
        first_hit->assign(first.begin(), first.end());
        hit_agent->assign(who.begin(), who.end());
        if (clearance) {
            clearance->assign(B, std::vector<double>());
            for (size_t b = 0; b < B; ++b) (*clearance)[b].assign(clear.begin() + b * m, clear.begin() + b * m + trajectories[b].size());
        }
        return true;
    }

 private:
    pqp_handle& h_;
    Params prm_;
    pqp_car_geometry car_;
};

}  // namespace PathOptimizationNS
