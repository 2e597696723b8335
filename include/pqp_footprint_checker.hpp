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
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "pqp.h"
#ifndef PQP_USE_REFERENCE_TYPES
#include "pqp_types.hpp"
#endif

namespace PathOptimizationNS {

class FootprintChecker {
 public:
    // car == nullptr: the reference's flags (pqp_car_default_geometry: car_width 2.0, rear_length -1.0, front_length 3.9)
    FootprintChecker(const float* layers, int n_maps, const pqp_grid_geometry& geom, const pqp_car_geometry* car = nullptr, int device = 0)
        : geom_(geom), n_maps_(n_maps) {
        if (car) car_ = *car; else pqp_car_default_geometry(&car_);
        if (!layers || n_maps < 1 || pqp_create(&h_, nullptr, device, 1, 2) != PQP_OK) return;
        void* s = nullptr;
        pqp_get_stream(h_, &s);
        stream_ = (hipStream_t)s;
        const size_t bytes = (size_t)n_maps * geom.rows * geom.cols * sizeof(float);
        if (hipSetDevice(device) != hipSuccess || hipMalloc(&d_dist_, bytes) != hipSuccess) { d_dist_ = nullptr; return; }
        ok_ = hipMemcpy(d_dist_, layers, bytes, hipMemcpyHostToDevice) == hipSuccess;
    }
    FootprintChecker(const FootprintChecker&) = delete;
    FootprintChecker& operator=(const FootprintChecker&) = delete;
    ~FootprintChecker() {
        for (void* p : {d_dist_, d_states_, d_ints_, d_free_}) if (p) (void)hipFree(p);
        if (h_) pqp_destroy(h_);
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
        const int batch = (int)paths.size();
        int n = 1;
        for (const auto& p : paths) n = (int)p.size() > n ? (int)p.size() : n;
        std::vector<double> states((size_t)batch * n * 3, 0.0);
        std::vector<int32_t> ints((size_t)batch * 3, 0);              // n_of, map_of, first_collision
        for (int b = 0; b < batch; ++b) {
            for (size_t i = 0; i < paths[b].size(); ++i) {
                double* s = &states[((size_t)b * n + i) * 3];
                s[0] = paths[b][i].x; s[1] = paths[b][i].y; s[2] = paths[b][i].heading;
            }
            ints[b] = (int32_t)paths[b].size();
            const int m = map_of ? (*map_of)[b] : 0;
            if (m < 0 || m >= n_maps_) return false;
            ints[batch + b] = m;
        }
        std::vector<uint8_t> fr((size_t)batch * n);
        if (!run(batch, n, states, ints, mode, fr.data())) return false;
        first_collision->assign(ints.begin() + 2 * batch, ints.end());
        if (free) {
            free->assign(batch, {});
            for (int b = 0; b < batch; ++b) (*free)[b].assign(fr.begin() + (size_t)b * n, fr.begin() + (size_t)b * n + paths[b].size());
        }
        return true;
    }

 private:
    bool single(const State& s, int mode, int map) {
        if (map < 0 || map >= n_maps_) return false;
        std::vector<double> st = {s.x, s.y, s.heading};
        std::vector<int32_t> ints = {1, map, 0};
        uint8_t fr = 0;
        return run(1, 1, st, ints, mode, &fr) && fr == 1;
    }
    static bool grow(void** p, size_t* have, size_t need) {
        if (need <= *have) return true;
        if (*p) (void)hipFree(*p);
        *p = nullptr; *have = 0;
        if (hipMalloc(p, need) != hipSuccess) { *p = nullptr; return false; }
        *have = need;
        return true;
    }
    // ints: n_of [batch], map_of [batch], first_collision [batch] (written back)
    bool run(int batch, int n, const std::vector<double>& states, std::vector<int32_t>& ints, int mode, uint8_t* free) {
        if (!ok_) return false;
        const size_t b_st = states.size() * sizeof(double), b_ints = ints.size() * sizeof(int32_t), b_free = (size_t)batch * n;
        if (!grow(&d_states_, &cap_states_, b_st) || !grow(&d_ints_, &cap_ints_, b_ints) || !grow(&d_free_, &cap_free_, b_free)) return false;
        int32_t* di = static_cast<int32_t*>(d_ints_);
        if (hipMemcpyAsync(d_states_, states.data(), b_st, hipMemcpyHostToDevice, stream_) != hipSuccess ||
            hipMemcpyAsync(di, ints.data(), b_ints, hipMemcpyHostToDevice, stream_) != hipSuccess)
            return false;
        if (pqp_footprint_check_device(h_, batch, n, 3, static_cast<const double*>(d_states_), di, static_cast<const float*>(d_dist_), di + batch,
                                       &geom_, &car_, mode, static_cast<uint8_t*>(d_free_), di + 2 * batch, nullptr) != PQP_OK)
            return false;
        if (hipMemcpyAsync(free, d_free_, b_free, hipMemcpyDeviceToHost, stream_) != hipSuccess ||
            hipMemcpyAsync(ints.data() + 2 * batch, di + 2 * batch, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, stream_) != hipSuccess)
            return false;
        return hipStreamSynchronize(stream_) == hipSuccess;
    }

    pqp_handle* h_ = nullptr;
    hipStream_t stream_ = nullptr;
    pqp_grid_geometry geom_;
    pqp_car_geometry car_;
    int n_maps_ = 0;
    bool ok_ = false;
    void *d_dist_ = nullptr, *d_states_ = nullptr, *d_ints_ = nullptr, *d_free_ = nullptr;
    size_t cap_states_ = 0, cap_ints_ = 0, cap_free_ = 0;
};

}  // namespace PathOptimizationNS
