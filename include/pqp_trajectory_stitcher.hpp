// pqp_trajectory_stitcher.hpp — PathOptimizationNS::TrajectoryStitcher: the start of a planning cycle from the previous cycle's plan over
// pqp_stitch_trajectory.  Header-only over the C ABI (link libpqp_hip and libamdhip64).  PlanSelector (pqp_plan_selector.hpp) leaves a
// cycle's winners; this takes them one cycle later, with the measured state of every vehicle and the time since its plan began, and
// gives the state the new cycle plans from - a state of the old plan a little ahead of the car, or, where the car has left the plan, the
// measurement advanced by as much - with the verdict, the deviations and the piece of the old plan that leads to the start.  The
// reference plans one path per call from the state it is given: it stitches nothing.  The stitcher keeps its own handle.
//
//   params()                                   the PQP_STITCH_PARAMS doubles, to edit (pqp_stitch_default_params)
//   keep()                                     the states of the old plan kept behind the car
//   stitch(previous, dt, measured, &results)   one call for all vehicles
//
// Not copyable, not thread-safe, no exceptions; without a usable GPU ok() is false and stitch returns false.
#pragma once
#include <cstdint>
#include <vector>

#include "pqp.h"
#ifndef PQP_USE_REFERENCE_TYPES
#include "pqp_types.hpp"
#endif
#include "pqp_wrapper_detail.hpp"

namespace PathOptimizationNS {

class TrajectoryStitcher {
 public:
    explicit TrajectoryStitcher(int device = 0) : h_(device) { pqp_stitch_default_params(prm_, &keep_); }
    bool ok() const { return h_.ok(); }
    double* params() { return prm_; }
    int& keep() { return keep_; }

    struct Measured {
        double x = 0.0, y = 0.0, heading = 0.0, v = 0.0, a = 0.0, yaw_rate = 0.0;
        double t = 0.0;                       // the time of the measurement, in the time base of the vehicle's previous plan
    };

    template <class StateT>
    struct Result {
        StateT start{};                       // the state the new cycle plans from (s = 0 on a replan, the old plan's s on a stitch)
        double row[PQP_TRAJ_STRIDE] = {};     // the same as the library wrote it: x, y, heading, k, s, v, a, t
        double t_start = 0.0;                 // where the new plan's t = 0 lies in the old time base
        int flags = 0;                        // PQP_STITCH_*
        double lon = 0.0, lat = 0.0, dh = 0.0;
        std::vector<StateT> prefix;           // the piece of the old plan that leads to the start, s = 0 at its last state ...
        std::vector<double> prefix_t;         // ... and their times, 0 at the last
        bool stitched() const { return (flags & PQP_STITCH_STITCHED) != 0; }
        bool usable() const { return (flags & PQP_STITCH_BAD) == 0; }
    };

    // previous: per vehicle the states of its previous plan, state f at time f * dt (PlanSelector::selectBest's winners, PlanSampler::sample's
    // states and Result::dt); a vehicle without one (fewer than two states) is replanned from its measurement.  measured: one per vehicle.
    // false: a GPU error or a bad argument (pqp_last_error()).
    template <class StateT>
    bool stitch(const std::vector<std::vector<StateT>>& previous, double dt, const std::vector<Measured>& measured, std::vector<Result<StateT>>* results) {
        const size_t G = previous.size();
        if (!ok() || !results || G == 0 || measured.size() != G) return false;
        const detail::Packed prev = detail::pack(previous, PQP_TRAJ_STRIDE, detail::TimedTrajRow{dt});
        const size_t m = prev.n;
        std::vector<double> meas(G * 6), t_now(G), state(G * PQP_TRAJ_STRIDE), dev(G * 3), prefix(G * m * PQP_TRAJ_STRIDE);
        std::vector<int32_t> flags(G), idx(G * 3), prefix_n(G);
        for (size_t g = 0; g < G; ++g) {
            const Measured& c = measured[g];
            double* q = &meas[g * 6];
            q[0] = c.x; q[1] = c.y; q[2] = c.heading; q[3] = c.v; q[4] = c.a; q[5] = c.yaw_rate;
            t_now[g] = c.t;
        }
        if (pqp_stitch_trajectory(h_.get(), prm_, keep_, (int)m, (int)G, (int)m, PQP_TRAJ_STRIDE, prev.rows.data(), prev.count.data(),
                                  meas.data(), t_now.data(), (int)G, nullptr, state.data(), flags.data(), dev.data(), idx.data(), prefix.data(),
                                  prefix_n.data(), nullptr, nullptr, nullptr) != PQP_OK)
            return false;
        results->assign(G, Result<StateT>());
        for (size_t g = 0; g < G; ++g) {
            Result<StateT>& out = (*results)[g];
            const double* r = &state[g * PQP_TRAJ_STRIDE];
            for (int c = 0; c < PQP_TRAJ_STRIDE; ++c) out.row[c] = r[c];
            out.start = detail::TrajRow::read<StateT>(r);
            out.t_start = r[7];
            out.flags = flags[g];
            out.lon = dev[g * 3]; out.lat = dev[g * 3 + 1]; out.dh = dev[g * 3 + 2];
            for (int j = 0; j < prefix_n[g]; ++j) {
                const double* p = &prefix[(g * m + j) * PQP_TRAJ_STRIDE];
                out.prefix.push_back(detail::TrajRow::read<StateT>(p));
                out.prefix_t.push_back(p[7]);
            }
        }
        return true;
    }

 private:
    detail::OwnedHandle h_;
    double prm_[PQP_STITCH_PARAMS];
    int keep_ = 20;
};

}  // namespace PathOptimizationNS
