// pqp_agent_overlay.hpp — PathOptimizationNS::AgentOverlay: the scenes' standing agents laid over obstacle distance layers, over
// pqp_overlay_agents_device.  Header-only over the C ABI and the HIP runtime API (link libpqp_hip and libamdhip64), in the manner of
// FootprintChecker (pqp_footprint_checker.hpp).  The overlay keeps its own handle and a device copy of the base layers, so a call uploads
// only the agents' rows; the scenes' layers stay on the device, where layers() hands them to callers that go on with *_device calls
// (pqp_optimize_path_device, pqp_corridor_bounds_device, pqp_footprint_check_device: map_of then indexes scenes).  The reference has no
// counterpart: it plans against one static map.  Moving agents are not overlaid: they are the speed stages'.
//
// Layers as pqp_corridor_bounds takes them: [n_maps][cols][rows] float, i.e. grid_map.get("distance").data() of each map laid end to end.
// Not copyable, not thread-safe, no exceptions; without a usable GPU ok() is false and overlay() fails.
#pragma once
#include <cstdint>
#include <vector>

#include "pqp.h"
#include "pqp_wrapper_device.hpp"          // StandingAgent: a rounded oriented rectangle, the row pqp_overlay_agents reads

namespace PathOptimizationNS {

class AgentOverlay {
 public:
    AgentOverlay(const float* layers, int n_maps, const pqp_grid_geometry& geom, int device = 0)
        : h_(device, layers && n_maps >= 1), stream_(detail::stream_of(h_)), geom_(geom), n_maps_(n_maps) {
        ok_ = h_.ok() && d_base_.upload(device, layers, (size_t)n_maps * geom.rows * geom.cols * sizeof(float));
    }
    bool ok() const { return ok_; }

    // agents[s]: scene s's standing agents (the scenes may differ in their counts).  a_of: agents per scene, to count fewer than are
    // given (nullptr: all of a scene's); base_of: the base layer of each scene (nullptr: layer 0 of one, else layer s, which needs as
    // many scenes as layers); inflate: extra room around every agent, in m (negative: pqp_overlay_default_params).  layers, optional:
    // [n_scenes][cols][rows] float, the scenes' layers copied back; flags, optional: PQP_OVERLAY_BAD / PQP_OVERLAY_NONE / 0 per scene.
    // false: a GPU error or bad argument (pqp_last_error()); the outputs then say nothing.
    bool overlay(const std::vector<std::vector<StandingAgent>>& agents, const std::vector<int>* a_of, const std::vector<int>* base_of,
                 double inflate, std::vector<float>* layers, std::vector<int>* flags) {
        if (!ok_ || agents.empty() || (a_of && a_of->size() != agents.size()) || (base_of && base_of->size() != agents.size())) return false;
        const int n_scenes = (int)agents.size();
        const detail::AgentRows host = detail::pack_agents(agents);
        const size_t a_max = host.a_max, cells = (size_t)geom_.rows * geom_.cols, rows = (size_t)n_scenes * a_max;
        std::vector<int32_t> ints(host.a_of);                         // a_of, base_of, flags
        ints.resize((size_t)n_scenes * 3, 0);
        for (int s = 0; s < n_scenes; ++s) {
            if (a_of) ints[s] = (*a_of)[s];
            const int b = base_of ? (*base_of)[s] : 0;
            if (b < 0 || b >= n_maps_) return false;
            ints[n_scenes + s] = b;
        }
        if (inflate < 0.0) pqp_overlay_default_params(&inflate);
        const size_t b_rows = host.rows.size() * sizeof(double), b_ints = ints.size() * sizeof(int32_t);
        if (!d_rows_.grow(b_rows) || !d_frames_.grow(rows * PQP_AGENT_FRAME_STRIDE * sizeof(double)) || !d_ints_.grow(b_ints) ||
            !d_layers_.grow((size_t)n_scenes * cells * sizeof(float)))
            return false;
        int32_t* di = d_ints_.as<int32_t>();
        if ((b_rows && hipMemcpyAsync(d_rows_.as<double>(), host.rows.data(), b_rows, hipMemcpyHostToDevice, stream_) != hipSuccess) ||
            hipMemcpyAsync(di, ints.data(), b_ints, hipMemcpyHostToDevice, stream_) != hipSuccess)
            return false;
        n_scenes_ = 0;
        if (pqp_overlay_agents_device(h_.get(), inflate, n_maps_, &geom_, d_base_.as<float>(), n_scenes, (int)a_max, d_rows_.as<double>(), di,
                                      base_of ? di + n_scenes : nullptr, d_frames_.as<double>(), d_layers_.as<float>(), di + 2 * n_scenes) != PQP_OK)
            return false;
        if (layers) {
            layers->resize((size_t)n_scenes * cells);
            if (hipMemcpyAsync(layers->data(), d_layers_.as<float>(), layers->size() * sizeof(float), hipMemcpyDeviceToHost, stream_) != hipSuccess) return false;
        }
        if (hipMemcpyAsync(ints.data() + 2 * n_scenes, di + 2 * n_scenes, (size_t)n_scenes * sizeof(int32_t), hipMemcpyDeviceToHost, stream_) != hipSuccess ||
            hipStreamSynchronize(stream_) != hipSuccess)
            return false;
        if (flags) flags->assign(ints.begin() + 2 * n_scenes, ints.end());
        n_scenes_ = n_scenes;
        return true;
    }

    // the scenes' layers of the last overlay() that succeeded, on the device: [scenes()][cols][rows] float, valid until the next
    // overlay() or the destructor; nullptr before the first
    const float* layers() const { return n_scenes_ ? d_layers_.as<float>() : nullptr; }
    int scenes() const { return n_scenes_; }
    const pqp_grid_geometry& geometry() const { return geom_; }

 private:
    detail::OwnedHandle h_;
    hipStream_t stream_ = nullptr;
    pqp_grid_geometry geom_;
    int n_maps_ = 0, n_scenes_ = 0;
    bool ok_ = false;
    detail::DeviceArray d_base_, d_rows_, d_frames_, d_ints_, d_layers_;          // behind h_: freed before the handle goes
};

}  // namespace PathOptimizationNS
