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
        if (states) states->assign(B, std::vector<StateT>());
        for (size_t b = 0; b < B; ++b) {
            Plan& p = (*plans)[b];
            p.flags = raw.flags[b];
            p.cost = raw.cost[b];
            for (int k = 0; k < raw.reached[b]; ++k) {
                p.station.push_back(raw.steps[(b * m + k) * 2]);
                p.step.push_back(raw.steps[(b * m + k) * 2 + 1]);
                if (states) {
                    const double* r = &raw.traj[(b * m + k) * PQP_TRAJ_STRIDE];
                    StateT st{};
                    st.x = r[0]; st.y = r[1]; st.heading = r[2]; st.k = r[3]; st.s = r[4]; st.v = r[5]; st.a = r[6];
                    (*states)[b].push_back(st);
                }
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
        size_t n = 1, m = (size_t)std::max(layers, 1), a_max = 0;
        for (const auto& p : paths) n = std::max(n, p.size());
        for (const auto& s : scenes) {
            a_max = std::max(a_max, s.size());
            for (const auto& a : s) m = std::max(m, a.size());
        }
        raw->B = B; raw->n = n; raw->m = m;
        raw->rows.assign(B * n * 6, 0.0);
        raw->profile.assign(B * n * PQP_SPEED_STRIDE, 0.0);
        raw->traj.assign(B * m * PQP_TRAJ_STRIDE, 0.0);
        raw->cost.assign(B, 0.0);
        raw->n_of.assign(B, 0); raw->steps.assign(B * m * 2, 0); raw->reached.assign(B, 0); raw->flags.assign(B, 0);
        raw->blocked.assign(with_blocked ? B * m * (size_t)((std::max(prm_.stations, 0) + 31) / 32) : 0, 0);
        std::vector<double> agents(S * a_max * m * PQP_AGENT_STRIDE, 0.0);
        std::vector<int32_t> a_of(S), scene;
        for (size_t b = 0; b < B; ++b) {
            raw->n_of[b] = (int32_t)paths[b].size();
            for (size_t i = 0; i < paths[b].size(); ++i) {
                const StateT& st = paths[b][i];
                double* r = &raw->rows[(b * n + i) * 6];
                double* o = &raw->profile[(b * n + i) * PQP_SPEED_STRIDE];
                r[0] = st.x; r[1] = st.y; r[2] = st.heading; r[5] = st.k;
                o[0] = st.s; o[1] = st.v; o[2] = st.a;
            }
        }
        for (size_t s = 0; s < S; ++s) {
            a_of[s] = (int32_t)scenes[s].size();
            for (size_t a = 0; a < scenes[s].size(); ++a)
                for (size_t k = 0; k < m; ++k) {
                    double* r = &agents[((s * a_max + a) * m + k) * PQP_AGENT_STRIDE];
                    if (k < scenes[s][a].size()) {
                        const PredictedAgent& p = scenes[s][a][k];
                        r[0] = p.x; r[1] = p.y; r[2] = p.heading; r[3] = p.half_length; r[4] = p.half_width; r[5] = p.radius;
                    } else {
                        r[3] = -1.0;
                    }
                }
        }
        if (scene_of) scene.assign(scene_of->begin(), scene_of->end());
        return pqp_speed_search(&h_, &prm_, &car_, (int)B, (int)n, 6, raw->rows.data(), raw->n_of.data(), nullptr, raw->profile.data(), v_start.data(),
                                (int)m, (int)S, (int)a_max, a_max ? agents.data() : nullptr, a_of.data(), scene_of ? scene.data() : nullptr,
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
