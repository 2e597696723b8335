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
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "pqp.h"

namespace PathOptimizationNS {

// a standing agent: a rounded oriented rectangle, the row pqp_overlay_agents reads (half_length < 0 or half_width < 0: absent)
struct StandingAgent {
    double x{}, y{}, heading{}, half_length{}, half_width{}, radius{};
};

class AgentOverlay {
 public:
    AgentOverlay(const float* layers, int n_maps, const pqp_grid_geometry& geom, int device = 0) : geom_(geom), n_maps_(n_maps) {
        if (!layers || n_maps < 1 || pqp_create(&h_, nullptr, device, 1, 2) != PQP_OK) return;
        void* s = nullptr;
        pqp_get_stream(h_, &s);
        stream_ = (hipStream_t)s;
        const size_t bytes = (size_t)n_maps * geom.rows * geom.cols * sizeof(float);
        if (hipSetDevice(device) != hipSuccess || hipMalloc(&d_base_, bytes) != hipSuccess) { d_base_ = nullptr; return; }
        ok_ = hipMemcpy(d_base_, layers, bytes, hipMemcpyHostToDevice) == hipSuccess;
    }
    AgentOverlay(const AgentOverlay&) = delete;
    AgentOverlay& operator=(const AgentOverlay&) = delete;
    ~AgentOverlay() {
        for (void* p : {d_base_, d_rows_, d_frames_, d_ints_, d_layers_}) if (p) (void)hipFree(p);
        if (h_) pqp_destroy(h_);
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
        size_t a_max = 0;
        for (const auto& sc : agents) a_max = sc.size() > a_max ? sc.size() : a_max;
        const size_t cells = (size_t)geom_.rows * geom_.cols, rows = (size_t)n_scenes * a_max;
        std::vector<double> host(rows * PQP_AGENT_STRIDE);
        std::vector<int32_t> ints((size_t)n_scenes * 3, 0);           // a_of, base_of, flags
        for (int s = 0; s < n_scenes; ++s) {
            for (size_t a = 0; a < a_max; ++a) {
                double* r = &host[((size_t)s * a_max + a) * PQP_AGENT_STRIDE];
                if (a < agents[s].size()) {
                    const StandingAgent& g = agents[s][a];
                    r[0] = g.x; r[1] = g.y; r[2] = g.heading; r[3] = g.half_length; r[4] = g.half_width; r[5] = g.radius;
                } else {
                    r[0] = r[1] = r[2] = r[5] = 0.0; r[3] = r[4] = -1.0;
                }
            }
            ints[s] = a_of ? (*a_of)[s] : (int32_t)agents[s].size();
            const int b = base_of ? (*base_of)[s] : 0;
            if (b < 0 || b >= n_maps_) return false;
            ints[n_scenes + s] = b;
        }
        if (inflate < 0.0) pqp_overlay_default_params(&inflate);
        const size_t b_rows = host.size() * sizeof(double), b_ints = ints.size() * sizeof(int32_t);
        if (!grow(&d_rows_, &cap_rows_, b_rows) || !grow(&d_frames_, &cap_frames_, rows * PQP_AGENT_FRAME_STRIDE * sizeof(double)) ||
            !grow(&d_ints_, &cap_ints_, b_ints) || !grow(&d_layers_, &cap_layers_, (size_t)n_scenes * cells * sizeof(float)))
            return false;
        int32_t* di = static_cast<int32_t*>(d_ints_);
        if ((b_rows && hipMemcpyAsync(d_rows_, host.data(), b_rows, hipMemcpyHostToDevice, stream_) != hipSuccess) ||
            hipMemcpyAsync(di, ints.data(), b_ints, hipMemcpyHostToDevice, stream_) != hipSuccess)
            return false;
        n_scenes_ = 0;
        if (pqp_overlay_agents_device(h_, inflate, n_maps_, &geom_, static_cast<const float*>(d_base_), n_scenes, (int)a_max,
                                      static_cast<const double*>(d_rows_), di, base_of ? di + n_scenes : nullptr, static_cast<double*>(d_frames_),
                                      static_cast<float*>(d_layers_), di + 2 * n_scenes) != PQP_OK)
            return false;
        if (layers) {
            layers->resize((size_t)n_scenes * cells);
            if (hipMemcpyAsync(layers->data(), d_layers_, layers->size() * sizeof(float), hipMemcpyDeviceToHost, stream_) != hipSuccess) return false;
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
    const float* layers() const { return n_scenes_ ? static_cast<const float*>(d_layers_) : nullptr; }
    int scenes() const { return n_scenes_; }
    const pqp_grid_geometry& geometry() const { return geom_; }

 private:
    static bool grow(void** p, size_t* have, size_t need) {
        if (need <= *have) return true;
        if (*p) (void)hipFree(*p);
        *p = nullptr; *have = 0;
        if (hipMalloc(p, need) != hipSuccess) { *p = nullptr; return false; }
        *have = need;
        return true;
    }

    pqp_handle* h_ = nullptr;
    hipStream_t stream_ = nullptr;
    pqp_grid_geometry geom_;
    int n_maps_ = 0, n_scenes_ = 0;
    bool ok_ = false;
    void *d_base_ = nullptr, *d_rows_ = nullptr, *d_frames_ = nullptr, *d_ints_ = nullptr, *d_layers_ = nullptr;
    size_t cap_rows_ = 0, cap_frames_ = 0, cap_ints_ = 0, cap_layers_ = 0;
};

}  // namespace PathOptimizationNS
