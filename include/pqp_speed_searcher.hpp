// pqp_speed_searcher.hpp — PathOptimizationNS::SpeedSearcher: speeds that pass predicted moving agents, over pqp_speed_search.
// Header-only over the C ABI (link libpqp_hip and libamdhip64).  SpeedProfiler (pqp_speed_profiler.hpp) fills s, v and a of every state:
// the fastest speeds the path allows.  AgentChecker (pqp_agent_checker.hpp) says which of those trajectories hits a predicted agent.  This
// keeps the path and plans the speed: a station on the path for every time step, out of the cells the agents occupy, within the
// acceleration limits and under the profile's envelope - wait for the pedestrian, go ahead of the car that arrives later.
// The searcher borrows a handle - the planner's own, so the search runs on that handle's stream and GPU.
//
//   params()                              pqp_search_params to edit (pqp_search_default_params; pqp_search_params_from_speed)
//   car()                                 pqp_car_geometry to edit (pqp_car_default_geometry: the reference's flags)
//   search(paths, v_start, scenes, ...)   per path the planned (station, step) of every layer, the layers reached and PQP_SEARCH_* flags
//   search_raw(...)                       the same call with the C ABI's arrays left to the caller (SpeedRefiner's input)
//
// Not copyable, not thread-safe, no exceptions; search() returns false on a GPU error or a bad argument (pqp_last_error()).
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "pqp.h"
#include "pqp_agent_checker.hpp"

namespace PathOptimizationNS {

class SpeedSearcher {
 public:
    explicit SpeedSearcher(pqp_handle& handle) : h_(handle) {
        pqp_search_default_params(&prm_);
        pqp_car_default_geometry(&car_);
    }
    SpeedSearcher(const SpeedSearcher&) = delete;
    SpeedSearcher& operator=(const SpeedSearcher&) = delete;

    pqp_search_params& params() { return prm_; }
    pqp_car_geometry& car() { return car_; }

    struct Plan {
        std::vector<int> station, step;   // j_k and q_k of the layers reached
        int flags = 0;                    // PQP_SEARCH_*
        double cost = 0.0;
    };

    // what one call hands to pqp_speed_search and gets back, as the C ABI's arrays: search() reads plans out of it, and SpeedRefiner
    // (pqp_speed_refiner.hpp) hands it on to pqp_speed_refine
    struct Raw {
        size_t B = 0, n = 0, m = 0;
        std::vector<double> rows, profile, traj, cost;       // [B][n][6], [B][n][4], [B][m][8], [B]
        std::vector<int32_t> n_of, steps, reached, flags, blocked;      // blocked [B][m][W], filled when asked for
    };

    // paths: State or SlState with x, y, heading, k and the s, v, a SpeedProfiler::profile wrote
    // v_start [paths]: the speed at waypoint 0
    // scenes [scene][agent][layer]: the predicted agents at the layers' times k dt; the longest agent gives the number of layers m (at
    //   least `layers`), and an agent with fewer steps is absent behind its last one
    // plans: per path the plan; states (optional): per path the planned state of every layer reached - x, y, heading, k, s, v, a
    // scene_of (optional, [paths]): the scene every path is searched against; absent: scene 0
    template <class StateT>
    bool search(const std::vector<std::vector<StateT>>& paths, const std::vector<double>& v_start,
                const std::vector<std::vector<std::vector<PredictedAgent>>>& scenes, std::vector<Plan>* plans,
                std::vector<std::vector<StateT>>* states = nullptr, const std::vector<int>* scene_of = nullptr, int layers = 1) {
        Raw raw;
        if (!plans || !search_raw(paths, v_start, scenes, scene_of, layers, false, &raw)) return false;
        const size_t B = raw.B, m = raw.m;
        plans->assign(B, Plan());
        if (states) detail::read_trajectories(raw.traj, m, raw.reached, states);
        for (size_t b = 0; b < B; ++b) {
            Plan& p = (*plans)[b];
            p.flags = raw.flags[b];
            p.cost = raw.cost[b];
            for (int k = 0; k < raw.reached[b]; ++k) {
                p.station.push_back(raw.steps[(b * m + k) * 2]);
                p.step.push_back(raw.steps[(b * m + k) * 2 + 1]);
            }
        }
        return true;
    }

    // the same call with its arrays left in *raw (with_blocked: the occupancy bits too)
    template <class StateT>
    bool search_raw(const std::vector<std::vector<StateT>>& paths, const std::vector<double>& v_start,
                    const std::vector<std::vector<std::vector<PredictedAgent>>>& scenes, const std::vector<int>* scene_of, int layers,
                    bool with_blocked, Raw* raw) {
        if (!raw || paths.empty() || scenes.empty() || v_start.size() != paths.size()) return false;
        const size_t B = paths.size(), S = scenes.size();
        if (scene_of && scene_of->size() != B) return false;
        size_t m = (size_t)std::max(layers, 1);
        for (const auto& s : scenes) m = detail::longest(s, m);
        detail::Packed rows = detail::pack(paths, 6, detail::PathRow());
        const detail::AgentRows ag = detail::pack_agents(scenes, m);
        const size_t n = rows.n;
        raw->B = B; raw->n = n; raw->m = m;
        raw->rows = std::move(rows.rows);
        raw->n_of = std::move(rows.count);
        raw->profile = detail::pack(paths, PQP_SPEED_STRIDE, detail::ProfileRow()).rows;
        raw->traj.assign(B * m * PQP_TRAJ_STRIDE, 0.0);
        raw->cost.assign(B, 0.0);
        raw->steps.assign(B * m * 2, 0); raw->reached.assign(B, 0); raw->flags.assign(B, 0);
        raw->blocked.assign(with_blocked ? B * m * (size_t)((std::max(prm_.stations, 0) + 31) / 32) : 0, 0);
        std::vector<int32_t> scene;
        if (scene_of) scene.assign(scene_of->begin(), scene_of->end());
        return pqp_speed_search(&h_, &prm_, &car_, (int)B, (int)n, 6, raw->rows.data(), raw->n_of.data(), nullptr, raw->profile.data(), v_start.data(),
                                (int)m, (int)S, (int)ag.a_max, ag.a_max ? ag.rows.data() : nullptr, ag.a_of.data(), scene_of ? scene.data() : nullptr,
                                with_blocked ? raw->blocked.data() : nullptr, raw->steps.data(), raw->traj.data(), raw->cost.data(),
                                raw->reached.data(), raw->flags.data()) == PQP_OK;
    }

    pqp_handle& handle() { return h_; }

 private:
    pqp_handle& h_;
    pqp_search_params prm_;
    pqp_car_geometry car_;
};

}  // namespace PathOptimizationNS
