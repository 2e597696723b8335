// pqp_agent_predictor.hpp — PathOptimizationNS::AgentPredictor: tracked agents to the predicted rows AgentChecker (pqp_agent_checker.hpp)
// and the speed search read, over pqp_predict_agents.  Header-only over the C ABI (link libpqp_hip and libamdhip64).  A perception stack
// hands out tracks - a pose, a speed, an acceleration, a yaw rate and a size per agent; this says where each of them is at the layers'
// times, or on r sub-steps per layer, under constant turn rate and acceleration (capped, and standing still once stopped) or along the
// lane it is in.  The predictor borrows a handle - the planner's own, so the prediction runs on that handle's stream and GPU.
//
//   params()                              the prediction's parameters to edit: v_cap, grow, l_max (pqp_predict_default_params)
//   set_lanes(spline, ext, length, m)     the lanes' spline tables, as pqp_spline_fit writes them; none: every track is free
//   predict(scenes, t0, dt, m, r, ...)    the rows of every agent of every scene, PredictedAgent by PredictedAgent
//
// Not copyable, not thread-safe, no exceptions; predict() returns false on a GPU error or a bad argument (pqp_last_error()).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "pqp.h"
#include "pqp_agent_checker.hpp"

namespace PathOptimizationNS {

// an agent as it is tracked now: v >= 0 along the heading, a its derivative, yaw_rate the heading's; the size as PredictedAgent's.
// lane: the index of the lane it follows, or -1: none
struct TrackedAgent {
    double x{}, y{}, heading{}, v{}, a{}, yaw_rate{}, half_length{}, half_width{}, radius{};
    int lane{-1};
};

class AgentPredictor {
 public:
    explicit AgentPredictor(pqp_handle& handle) : h_(handle) {
        double prm[PQP_PREDICT_PARAMS];
        pqp_predict_default_params(prm);
        prm_ = Params{prm[PQP_PREDICT_V_CAP], prm[PQP_PREDICT_GROW], prm[PQP_PREDICT_L_MAX]};
    }
    AgentPredictor(const AgentPredictor&) = delete;
    AgentPredictor& operator=(const AgentPredictor&) = delete;

    struct Params { double v_cap, grow, l_max; };     // m/s, m/s, m: all finite and >= 0
    Params& params() { return prm_; }

    // spline [n_lanes][9][lane_m], ext [n_lanes][4], length [n_lanes]: copied
    void set_lanes(const std::vector<double>& spline, const std::vector<double>& ext, const std::vector<double>& length, int lane_m) {
        lane_spline_ = spline; lane_ext_ = ext; lane_length_ = length; lane_m_ = lane_m;
    }

    // scenes [scene][agent]: the tracks.  out [scene][agent][step]: (m - 1) * r + 1 steps, step f at t0 + (f / r) dt + ((f % r) dt) / r -
    // what AgentChecker::check and the speed search take.  flags (optional) [scene][agent]: PQP_PREDICT_*
    bool predict(const std::vector<std::vector<TrackedAgent>>& scenes, double t0, double dt, int m, int r,
                 std::vector<std::vector<std::vector<PredictedAgent>>>* out, std::vector<std::vector<int>>* flags = nullptr) {
        if (!out || scenes.empty() || m < 1 || r < 1) return false;
        const size_t S = scenes.size(), M = (size_t)(m - 1) * r + 1;
        const int n_lanes = (int)lane_length_.size();
        const detail::Packed tracks = detail::pack(scenes, PQP_TRACK_STRIDE, [](const TrackedAgent& t, size_t, double* q) {
            const double row[PQP_TRACK_STRIDE] = {t.x, t.y, t.heading, t.v, t.a, t.yaw_rate, t.half_length, t.half_width, t.radius};
            std::copy(row, row + PQP_TRACK_STRIDE, q);
        }, 0);
        const size_t a_max = tracks.n;
        std::vector<double> rows(S * a_max * M * PQP_AGENT_STRIDE);
        std::vector<int32_t> lane_of(S * a_max, -1), fl(S * a_max);
        for (size_t s = 0; s < S; ++s)
            for (size_t a = 0; a < scenes[s].size(); ++a) {
                if (scenes[s][a].lane >= n_lanes) return false;
                lane_of[s * a_max + a] = scenes[s][a].lane;
            }
        const double prm[PQP_PREDICT_PARAMS] = {prm_.v_cap, prm_.grow, prm_.l_max};
        if (pqp_predict_agents(&h_, prm, t0, dt, m, r, (int)S, (int)a_max, tracks.rows.data(), tracks.count.data(), lane_of.data(), n_lanes, lane_m_,
                               n_lanes ? lane_spline_.data() : nullptr, n_lanes ? lane_ext_.data() : nullptr,
                               n_lanes ? lane_length_.data() : nullptr, rows.data(), nullptr, fl.data()) != PQP_OK)
            return false;
        detail::unpack_agents(rows, tracks.count, a_max, M, out);
        if (flags) flags->assign(S, {});
        for (size_t s = 0; flags && s < S; ++s) (*flags)[s].assign(fl.begin() + s * a_max, fl.begin() + s * a_max + scenes[s].size());
        return true;
    }

 private:
    pqp_handle& h_;
    Params prm_;
    std::vector<double> lane_spline_, lane_ext_, lane_length_;
    int lane_m_ = 0;
};

}  // namespace PathOptimizationNS
