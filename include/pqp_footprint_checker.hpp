// pqp_footprint_checker.hpp — PathOptimizationNS::FootprintChecker: the reference's CollisionChecker (src/tools/collision_checker.cpp:9-58,
// built by PathOptimizer from its map, path_optimizer.cpp:29) over pqp_footprint_check_device.  Header-only over the C ABI and the HIP
// runtime API (link libpqp_hip and libamdhip64).  The checker keeps its own handle and a device copy of one or more distance layers,
// so a check uploads only the states.
//
//   isSingleStateCollisionFree / isSingleStateCollisionFreeImproved   the reference's two methods, one state (a batch of one)
//   checkPaths(paths, &first_collision)                                 every state of many paths in one launch
//
// Layers as pqp_corridor_bounds takes them: [n_maps][cols][rows] float, i.e. grid_map.get("distance").data() of each map laid end to end.
// Not copyable, not thread-safe, no exceptions; without a usable GPU ok() is false and every check reports a collision.
#pragma once
#include <cstdint>
#include <vector>

#include "pqp.h"
#ifndef PQP_USE_REFERENCE_TYPES
#include "pqp_types.hpp"
#endif
#include "pqp_wrapper_device.hpp"

namespace PathOptimizationNS {

class FootprintChecker {
 public:
    // car == nullptr: the reference's flags (pqp_car_default_geometry: car_width 2.0, rear_length -1.0, front_length 3.9)
    FootprintChecker(const float* layers, int n_maps, const pqp_grid_geometry& geom, const pqp_car_geometry* car = nullptr, int device = 0)
        : h_(device, layers && n_maps >= 1), stream_(detail::stream_of(h_)), geom_(geom), n_maps_(n_maps) {
        if (car) car_ = *car; else pqp_car_default_geometry(&car_);
        ok_ = h_.ok() && d_dist_.upload(device, layers, (size_t)n_maps * geom.rows * geom.cols * sizeof(float));
    }
    bool ok() const { return ok_; }

    // collision_checker.cpp:17-39 (map: which of the layers)
    bool isSingleStateCollisionFree(const State& current, int map = 0) { return single(current, PQP_FOOTPRINT_CIRCLES, map); }
    // collision_checker.cpp:41-58
    bool isSingleStateCollisionFreeImproved(const State& current, int map = 0) { return single(current, PQP_FOOTPRINT_BOUNDING_FIRST, map); }

    // Every state of every path, one launch: first_collision[k] = index of path k's first colliding state, its size if none (the reference
    // would call isSingleStateCollisionFree on each state in turn).  map_of: the layer of each path (nullptr: layer 0); free: per state,
    // optional.  false: a GPU error or bad argument (pqp_last_error()); the outputs then say nothing.
    bool checkPaths(const std::vector<std::vector<SlState>>& paths, std::vector<int>* first_collision, int mode = PQP_FOOTPRINT_CIRCLES,
                    const std::vector<int>* map_of = nullptr, std::vector<std::vector<uint8_t>>* free = nullptr) {
        if (!first_collision || paths.empty() || (map_of && map_of->size() != paths.size())) return false;
        const size_t B = paths.size();
        const detail::Packed states = detail::pack(paths, 3, detail::PoseRow());
        const size_t n = states.n;
        std::vector<int32_t> ints(states.count);                      // n_of, map_of, first_collision
        ints.resize(B * 3, 0);
        for (size_t b = 0; b < B; ++b) {
            const int m = map_of ? (*map_of)[b] : 0;
            if (m < 0 || m >= n_maps_) return false;
            ints[B + b] = m;
        }
        std::vector<uint8_t> fr(B * n);
        if (!run((int)B, (int)n, states.rows, ints, mode, fr.data())) return false;
        first_collision->assign(ints.begin() + 2 * B, ints.end());
        if (free) {
            free->assign(B, {});
            for (size_t b = 0; b < B; ++b) (*free)[b].assign(fr.begin() + b * n, fr.begin() + b * n + paths[b].size());
        }
        return true;
    }

 private:
    bool single(const State& s, int mode, int map) {
        if (map < 0 || map >= n_maps_) return false;
        std::vector<double> st(3);
        detail::PoseRow()(s, 0, st.data());
        std::vector<int32_t> ints = {1, map, 0};
        uint8_t fr = 0;
        return run(1, 1, st, ints, mode, &fr) && fr == 1;
    }
    // ints: n_of [batch], map_of [batch], first_collision [batch] (written back)
    bool run(int batch, int n, const std::vector<double>& states, std::vector<int32_t>& ints, int mode, uint8_t* free) {
        if (!ok_) return false;
        const size_t b_st = states.size() * sizeof(double), b_ints = ints.size() * sizeof(int32_t), b_free = (size_t)batch * n;
        if (!d_states_.grow(b_st) || !d_ints_.grow(b_ints) || !d_free_.grow(b_free)) return false;
        int32_t* di = d_ints_.as<int32_t>();
        if (hipMemcpyAsync(d_states_.as<double>(), states.data(), b_st, hipMemcpyHostToDevice, stream_) != hipSuccess ||
            hipMemcpyAsync(di, ints.data(), b_ints, hipMemcpyHostToDevice, stream_) != hipSuccess)
            return false;
        if (pqp_footprint_check_device(h_.get(), batch, n, 3, d_states_.as<double>(), di, d_dist_.as<float>(), di + batch, &geom_, &car_, mode,
                                       d_free_.as<uint8_t>(), di + 2 * batch, nullptr) != PQP_OK)
            return false;
        if (hipMemcpyAsync(free, d_free_.as<uint8_t>(), b_free, hipMemcpyDeviceToHost, stream_) != hipSuccess ||
            hipMemcpyAsync(ints.data() + 2 * batch, di + 2 * batch, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, stream_) != hipSuccess)
            return false;
        return hipStreamSynchronize(stream_) == hipSuccess;
    }

    detail::OwnedHandle h_;
    hipStream_t stream_ = nullptr;
    pqp_grid_geometry geom_;
    pqp_car_geometry car_;
    int n_maps_ = 0;
    bool ok_ = false;
    detail::DeviceArray d_dist_, d_states_, d_ints_, d_free_;          // behind h_: freed before the handle goes
};

}  // namespace PathOptimizationNS
