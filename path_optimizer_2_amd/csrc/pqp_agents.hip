// pqp_agents.hip — the entry points of include/pqp.h around predicted moving agents: sampled trajectories against them
// (pqp_agents_kernels.inc) and those agents' rows from their tracks (pqp_predict_kernels.inc).  Their kernels, launchers and entry
// points, and launch_agent_frames, through which the overlay (pqp_maps.hip) and the speed search (pqp_speed.hip) get their frames.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "pqp_internal.hpp"

using namespace pqp_internal;

#include "pqp_agents_kernels.inc"
#include "pqp_predict_kernels.inc"

int pqp_internal::launch_agent_frames(pqp_handle* h, int n_scenes, int a_max, int m, const double* agents, double* frames) {
    const pqp::AgentFramesArgs fa = {(long long)n_scenes * a_max * m, agents, frames};
    if (fa.rows == 0) return PQP_OK;
    hipLaunchKernelGGL(pqp::agent_frames_kernel, dim3((unsigned)((fa.rows + pqp::kAgentsThreads - 1) / pqp::kAgentsThreads)),
                       dim3(pqp::kAgentsThreads), 0, h->stream, fa);
    PQP_HIP(hipGetLastError());
    return PQP_OK;
}

extern "C" {

// ---- sampled trajectories against predicted moving agents -------------------------------------------------------------------------------------
void pqp_agents_default_params(double* margin) {
    if (!margin) return;
    *margin = 0.0;                  // touching is no hit; this library's choice, the reference has no moving obstacles
}

static const char* const kAgentsRefusal =
    "pqp_agents_check: bad argument (batch >= 1; m >= 1; stride >= 3; n_scenes >= 1; a_max >= 0; n_scenes * a_max * m <= 2^38; margin finite and >= 0; "
    "a finite car geometry)";

static bool agents_ok(pqp_handle* h, double margin, const pqp_car_geometry* car, int batch, int m, int stride, const double* traj,
                      int n_scenes, int a_max, const double* agents, const int32_t* first_hit, const int32_t* hit_agent) {
    return h && traj && first_hit && hit_agent && batch >= 1 && m >= 1 && stride >= 3 && agent_rows_ok(n_scenes, a_max, m, agents) &&
           std::isfinite(margin) && margin >= 0.0 && car_ok(car);
}

int pqp_agents_check_device(pqp_handle* h, double margin, const pqp_car_geometry* car, int batch, int m, int stride,
                            const double* traj, const int32_t* m_of, int n_scenes, int a_max, const double* agents, const int32_t* a_of,
                            const int32_t* scene_of, double* frames, int32_t* first_hit, int32_t* hit_agent, double* clearance) {
    if (!agents_ok(h, margin, car, batch, m, stride, traj, n_scenes, a_max, agents, first_hit, hit_agent) || (!frames && a_max > 0))
        return fail(PQP_ERR_INVALID, kAgentsRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::AgentsArgs a;
    if (const int rc = car_circles_of(car, &a.car)) return rc;
    a.batch = batch; a.m = m; a.stride = stride; a.n_scenes = n_scenes; a.a_max = a_max; a.traj = traj; a.m_of = m_of;
    a.a_of = a_of; a.scene_of = scene_of; a.margin = margin; a.frames = frames; a.first_hit = first_hit; a.hit_agent = hit_agent;
    a.clearance = clearance;
    return h->launch_timed([&]() -> int {
        if (const int rc = launch_agent_frames(h, n_scenes, a_max, m, agents, frames)) return rc;
        const dim3 grid = wave_grid(batch, pqp::kAgentsThreads);
        if (clearance) hipLaunchKernelGGL(pqp::agents_check_kernel<true>, grid, dim3(pqp::kAgentsThreads), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::agents_check_kernel<false>, grid, dim3(pqp::kAgentsThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_agents_check(pqp_handle* h, double margin, const pqp_car_geometry* car, int batch, int m, int stride,
                     const double* traj, const int32_t* m_of, int n_scenes, int a_max, const double* agents, const int32_t* a_of,
                     const int32_t* scene_of, int32_t* first_hit, int32_t* hit_agent, double* clearance) {
    if (!agents_ok(h, margin, car, batch, m, stride, traj, n_scenes, a_max, agents, first_hit, hit_agent)) return fail(PQP_ERR_INVALID, kAgentsRefusal);
    if (const int rc = index_range(scene_of, batch, n_scenes, "pqp_agents_check: scene_of outside [0, n_scenes)")) return rc;
    const size_t bm = (size_t)batch * m;
    Staging st(h);
    const double* d_traj = st.in(traj, bm * stride);
    const int32_t* d_m_of = st.in(m_of, batch);
    const AgentArrays d = stage_agents(st, n_scenes, a_max, m, agents, a_of, scene_of, batch);
    int32_t* d_first = st.out(first_hit, batch);
    int32_t* d_who = st.out(hit_agent, batch);
    double* d_clear = clearance ? st.out(clearance, bm) : nullptr;
    return st.run([&]() -> int {
        return pqp_agents_check_device(h, margin, car, batch, m, stride, d_traj, d_m_of, n_scenes, a_max, d.agents, d.a_of, d.of, d.frames, d_first,
                                       d_who, d_clear);
    });
}

// ---- tracked agents to predicted rows, on the layers' steps and on fine steps -----------------------------------------------------------------
void pqp_predict_default_params(double* prm) {
    if (!prm) return;
    // this library's choice: the reference has no moving obstacles
    prm[PQP_PREDICT_V_CAP] = 40.0;
    prm[PQP_PREDICT_GROW] = 0.0;
    prm[PQP_PREDICT_L_MAX] = 3.0;
}

static const char* const kPredictRefusal =
    "pqp_predict_agents: bad argument (n_scenes >= 1; a_max >= 0; m >= 1; r >= 1; (m - 1) * r + 1 <= INT_MAX; n_scenes * a_max * ((m - 1) * r + 1) <= "
    "2^38; t0 finite and >= 0; dt finite and > 0; v_cap, grow and l_max finite and >= 0; n_lanes >= 0; with n_lanes > 0 lane_m >= 2 and the three "
    "lane arrays)";

static bool predict_ok(pqp_handle* h, const double* prm, double t0, double dt, int m, int r, int n_scenes, int a_max, const double* tracks,
                       int n_lanes, int lane_m, const double* lane_spline, const double* lane_ext, const double* lane_length, const double* agents,
                       const int32_t* flags) {
    if (!(h && prm && m >= 1 && r >= 1 && n_lanes >= 0)) return false;
    const long long M = (long long)(m - 1) * r + 1;
    if (M > INT_MAX || !agent_rows_ok(n_scenes, a_max, (int)M, agents)) return false;             // (the rows written here, as their readers take them)
    if (a_max > 0 && !(tracks && flags)) return false;
    if (!(std::isfinite(t0) && t0 >= 0.0 && std::isfinite(dt) && dt > 0.0)) return false;
    for (int k = 0; k < PQP_PREDICT_PARAMS; ++k)
        if (!(std::isfinite(prm[k]) && prm[k] >= 0.0)) return false;
    return n_lanes == 0 || (lane_m >= 2 && lane_spline && lane_ext && lane_length);
}

int pqp_predict_agents_device(pqp_handle* h, const double* prm, double t0, double dt, int m, int r, int n_scenes, int a_max, const double* tracks,
                              const int32_t* a_of, const int32_t* lane_of, int n_lanes, int lane_m, const double* lane_spline,
                              const double* lane_ext, const double* lane_length, double* agents, double* anchor, int32_t* flags) {
    if (!predict_ok(h, prm, t0, dt, m, r, n_scenes, a_max, tracks, n_lanes, lane_m, lane_spline, lane_ext, lane_length, agents, flags))
        return fail(PQP_ERR_INVALID, kPredictRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::PredictArgs a;
    a.n_scenes = n_scenes; a.a_max = a_max; a.m = m; a.r = r; a.n_lanes = n_lanes; a.lane_m = lane_m; a.t0 = t0; a.dt = dt;
    a.v_cap = prm[PQP_PREDICT_V_CAP]; a.grow = prm[PQP_PREDICT_GROW]; a.l_max = prm[PQP_PREDICT_L_MAX];
    a.tracks = tracks; a.a_of = a_of; a.lane_of = lane_of; a.lane_spl = lane_spline; a.lane_ext = lane_ext; a.lane_len = lane_length;
    a.agents = agents; a.anchor = anchor; a.flags = flags;
    const long long slots = (long long)n_scenes * a_max;
    return h->launch_timed([&]() -> int {
        if (slots == 0) return PQP_OK;
        const long long blocks = (slots + pqp::kPredictThreads / 64 - 1) / (pqp::kPredictThreads / 64);
        hipLaunchKernelGGL(pqp::predict_agents_kernel, dim3((unsigned)std::min(blocks, pqp::kPredictMaxBlocks)), dim3(pqp::kPredictThreads), 0,
                           h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_predict_agents(pqp_handle* h, const double* prm, double t0, double dt, int m, int r, int n_scenes, int a_max, const double* tracks,
                       const int32_t* a_of, const int32_t* lane_of, int n_lanes, int lane_m, const double* lane_spline, const double* lane_ext,
                       const double* lane_length, double* agents, double* anchor, int32_t* flags) {
    if (!predict_ok(h, prm, t0, dt, m, r, n_scenes, a_max, tracks, n_lanes, lane_m, lane_spline, lane_ext, lane_length, agents, flags))
        return fail(PQP_ERR_INVALID, kPredictRefusal);
    const size_t slots = (size_t)n_scenes * a_max, M = (size_t)(m - 1) * r + 1;
    if (lane_of)
        for (size_t k = 0; k < slots; ++k)
            if (lane_of[k] >= n_lanes) return fail(PQP_ERR_INVALID, "pqp_predict_agents: lane_of at or above n_lanes");
    if (slots == 0) return PQP_OK;
    Staging st(h);
    const double* d_tracks = st.in(tracks, slots * PQP_TRACK_STRIDE);
    const int32_t* d_a_of = st.in(a_of, n_scenes);
    const int32_t* d_lane_of = st.in(lane_of, slots);
    const double* d_spl = n_lanes ? st.in(lane_spline, (size_t)n_lanes * 9 * lane_m) : nullptr;
    const double* d_ext = n_lanes ? st.in(lane_ext, (size_t)n_lanes * 4) : nullptr;
    const double* d_len = n_lanes ? st.in(lane_length, n_lanes) : nullptr;
    double* d_agents = st.out(agents, slots * M * PQP_AGENT_STRIDE);
    double* d_anchor = anchor ? st.out(anchor, slots * PQP_ANCHOR_STRIDE) : nullptr;
    int32_t* d_flags = st.out(flags, slots);
    return st.run([&]() -> int {
        return pqp_predict_agents_device(h, prm, t0, dt, m, r, n_scenes, a_max, d_tracks, d_a_of, d_lane_of, n_lanes, lane_m, d_spl, d_ext, d_len,
                                         d_agents, d_anchor, d_flags);
    });
}

}  // extern "C"
