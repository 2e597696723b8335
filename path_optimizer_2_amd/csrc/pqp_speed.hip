// pqp_speed.hip — the entry points of include/pqp.h that give a planned path its speeds: speed profiles along the paths
// (pqp_speed_kernels.inc), samples of those trajectories on a time grid (pqp_sample_kernels.inc), speeds that pass predicted agents in the
// path-time plane (pqp_search_kernels.inc; the agents' frames come through launch_agent_frames, pqp_agents.hip), the speed QP that makes
// such a plan drivable (pqp_refine_kernels.inc; its solve is the banded core's, launched from pqp_smoothers.hip) and those plans on a
// fine time step (pqp_plan_kernels.inc).  Their kernels, launchers and entry points.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "pqp_defaults.hpp"
#include "pqp_internal.hpp"

using namespace pqp_internal;

#include "pqp_speed_kernels.inc"
#include "pqp_sample_kernels.inc"
#include "pqp_search_kernels.inc"
#include "pqp_refine_kernels.inc"
#include "pqp_plan_kernels.inc"

extern "C" {

// ---- planned paths to trajectories: s, v, a, t ---------------------------------------------------------------------------------------------
void pqp_speed_default_params(pqp_speed_params* p) {
    if (!p) return;
    // this library's choice: the reference plans geometry only and has no such flags
    p->v_max = 10.0;
    p->a_max = 1.5;
    p->d_max = 3.0;
    p->a_lat_max = 2.0;
}

static const char* const kSpeedRefusal =
    "pqp_speed_profile: bad argument (batch >= 1; n >= 1; stride >= 6; v_max finite and >= 0; a_max and d_max finite and > 0; a_lat_max > 0)";

static bool speed_ok(pqp_handle* h, const pqp_speed_params* prm, int batch, int n, int stride, const double* paths, const double* v_start,
                     const double* profile, const int32_t* flags) {
    return h && prm && paths && v_start && profile && flags && batch >= 1 && n >= 1 && stride >= 6 && std::isfinite(prm->v_max) &&
           prm->v_max >= 0.0 && std::isfinite(prm->a_max) && prm->a_max > 0.0 && std::isfinite(prm->d_max) && prm->d_max > 0.0 &&
           prm->a_lat_max > 0.0;
}

int pqp_speed_profile_device(pqp_handle* h, const pqp_speed_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                             const int32_t* stop_before, const double* v_limit, const double* v_start, const double* v_end, double* profile,
                             int32_t* flags) {
    if (!speed_ok(h, prm, batch, n, stride, paths, v_start, profile, flags)) return fail(PQP_ERR_INVALID, kSpeedRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::SpeedArgs a;
    a.batch = batch; a.n = n; a.stride = stride; a.paths = paths; a.n_of = n_of; a.stop_before = stop_before; a.v_limit = v_limit;
    a.v_start = v_start; a.v_end = v_end; a.prm = *prm; a.profile = profile; a.flags = flags;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::speed_profile_kernel, wave_grid(batch, pqp::kSpeedThreads), dim3(pqp::kSpeedThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_speed_profile(pqp_handle* h, const pqp_speed_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                      const int32_t* stop_before, const double* v_limit, const double* v_start, const double* v_end, double* profile,
                      int32_t* flags) {
    if (!speed_ok(h, prm, batch, n, stride, paths, v_start, profile, flags)) return fail(PQP_ERR_INVALID, kSpeedRefusal);
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_stop = st.in(stop_before, batch);
    const double* d_limit = st.in(v_limit, bn);
    const double* d_start = st.in(v_start, batch);
    const double* d_end = st.in(v_end, batch);
    double* d_profile = st.out(profile, bn * PQP_SPEED_STRIDE);
    int32_t* d_flags = st.out(flags, batch);
    return st.run([&]() -> int {
        return pqp_speed_profile_device(h, prm, batch, n, stride, d_paths, d_n_of, d_stop, d_limit, d_start, d_end, d_profile, d_flags);
    });
}

// ---- time-stamped trajectories at a fixed time step ------------------------------------------------------------------------------------------
void pqp_sample_default_params(pqp_sample_params* p) {
    if (!p) return;
    // this library's choice, as pqp_speed_default_params: the reference has no time axis
    p->dt = 0.1;
    p->hold_last = 0;
}

static const char* const kSampleRefusal =
    "pqp_sample_trajectory: bad argument (batch >= 1; n >= 1; m >= 1; stride >= 6; dt finite and > 0; hold_last 0 or 1)";

static bool sample_ok(pqp_handle* h, const pqp_sample_params* prm, int batch, int n, int stride, const double* paths, const double* profile, int m,
                      const double* traj, const int32_t* m_of, const int32_t* flags) {
    return h && prm && paths && profile && traj && m_of && flags && batch >= 1 && n >= 1 && m >= 1 && stride >= 6 && std::isfinite(prm->dt) &&
           prm->dt > 0.0 && (prm->hold_last == 0 || prm->hold_last == 1);
}

int pqp_sample_trajectory_device(pqp_handle* h, const pqp_sample_params* prm, int batch, int n, int stride, const double* paths,
                                 const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* t0, int m, double* traj,
                                 int32_t* m_of, int32_t* flags) {
    if (!sample_ok(h, prm, batch, n, stride, paths, profile, m, traj, m_of, flags)) return fail(PQP_ERR_INVALID, kSampleRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::SampleArgs a;
    a.batch = batch; a.n = n; a.stride = stride; a.m = m; a.paths = paths; a.n_of = n_of; a.stop_before = stop_before; a.profile = profile;
    a.t0 = t0; a.prm = *prm; a.traj = traj; a.m_of = m_of; a.flags = flags;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::sample_trajectory_kernel, wave_grid(batch, pqp::kSampleThreads), dim3(pqp::kSampleThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_sample_trajectory(pqp_handle* h, const pqp_sample_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                          const int32_t* stop_before, const double* profile, const double* t0, int m, double* traj, int32_t* m_of,
                          int32_t* flags) {
    if (!sample_ok(h, prm, batch, n, stride, paths, profile, m, traj, m_of, flags)) return fail(PQP_ERR_INVALID, kSampleRefusal);
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_stop = st.in(stop_before, batch);
    const double* d_profile = st.in(profile, bn * PQP_SPEED_STRIDE);
    const double* d_t0 = st.in(t0, batch);
    double* d_traj = st.out(traj, (size_t)batch * m * PQP_TRAJ_STRIDE);
    int32_t* d_m_of = st.out(m_of, batch);
    int32_t* d_flags = st.out(flags, batch);
    return st.run([&]() -> int {
        return pqp_sample_trajectory_device(h, prm, batch, n, stride, d_paths, d_n_of, d_stop, d_profile, d_t0, m, d_traj, d_m_of, d_flags);
    });
}

// ---- speeds past predicted agents: a search in the path-time plane ---------------------------------------------------------------------------
int pqp_search_params_from_speed(const pqp_speed_params* sp, double dt, double ds, pqp_search_params* p) {
    if (!sp || !p || !(std::isfinite(dt) && dt > 0.0) || !(std::isfinite(ds) && ds > 0.0))
        return fail(PQP_ERR_INVALID, "pqp_search_params_from_speed: bad argument (dt and ds finite and > 0)");
    // this library's choice, as pqp_speed_default_params: the reference has no time axis
    const double q_max = std::floor(sp->v_max * dt / ds), q_up = std::floor(sp->a_max * (dt * dt) / ds), q_down = std::floor(sp->d_max * (dt * dt) / ds);
    if (!(q_max >= 0.0 && q_max <= 63.0)) return fail(PQP_ERR_INVALID, "pqp_search_params_from_speed: floor(v_max dt / ds) outside 0 .. 63");
    p->dt = dt;
    p->ds = ds;
    p->w_slow = 1.0;
    p->w_accel = 1.0;
    p->margin = 0.0;
    p->stations = 128;
    p->q_max = (int32_t)q_max;
    p->q_up = (int32_t)std::fmin(std::fmax(q_up, 1.0), 63.0);
    p->q_down = (int32_t)std::fmin(std::fmax(q_down, 1.0), 63.0);
    return PQP_OK;
}

void pqp_search_default_params(pqp_search_params* p) {
    if (!p) return;
    pqp_speed_params sp;
    pqp_speed_default_params(&sp);
    (void)pqp_search_params_from_speed(&sp, 1.0, 0.5, p);
}

static const char* const kSearchRefusal =
    "pqp_speed_search: bad argument (batch >= 1; n >= 1; m >= 1; stride >= 6; dt and ds finite and > 0; w_slow, w_accel and margin finite and >= 0; "
    "stations >= 1; 0 <= q_max <= 63; q_up, q_down >= 0; stations * (q_max + 1) <= 4096; n_scenes >= 1; a_max >= 0; n_scenes * a_max * m <= 2^38; "
    "a finite car geometry)";

static bool search_ok(pqp_handle* h, const pqp_search_params* prm, const pqp_car_geometry* car, int batch, int n, int stride, const double* paths,
                      const double* profile, const double* v_start, int m, int n_scenes, int a_max, const double* agents, const int32_t* steps,
                      const double* traj, const double* cost, const int32_t* reached, const int32_t* flags) {
    if (!(h && prm && paths && profile && v_start && steps && traj && cost && reached && flags && batch >= 1 && n >= 1 && m >= 1 && stride >= 6))
        return false;
    const auto price = [](double v) { return std::isfinite(v) && v >= 0.0; };
    if (!(std::isfinite(prm->dt) && prm->dt > 0.0 && std::isfinite(prm->ds) && prm->ds > 0.0 && price(prm->w_slow) && price(prm->w_accel))) return false;
    if (!(prm->stations >= 1 && prm->q_max >= 0 && prm->q_max <= 63 && prm->q_up >= 0 && prm->q_down >= 0 &&
          (long long)prm->stations * (prm->q_max + 1) <= PQP_SEARCH_MAX_STATES))
        return false;
    return agent_rows_ok(n_scenes, a_max, m, agents) && price(prm->margin) && car_ok(car);
}

int pqp_speed_search_device(pqp_handle* h, const pqp_search_params* prm, const pqp_car_geometry* car, int batch, int n, int stride,
                            const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start,
                            int m, int n_scenes, int a_max, const double* agents, const int32_t* a_of, const int32_t* scene_of, double* frames,
                            int32_t* blocked, uint8_t* parents, int32_t* steps, double* traj, double* cost, int32_t* reached, int32_t* flags) {
    if (!search_ok(h, prm, car, batch, n, stride, paths, profile, v_start, m, n_scenes, a_max, agents, steps, traj, cost, reached, flags) ||
        !blocked || !parents || (!frames && a_max > 0))
        return fail(PQP_ERR_INVALID, kSearchRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::SearchArgs a;
    if (const int rc = car_circles_of(car, &a.car)) return rc;
    a.batch = batch; a.n = n; a.stride = stride; a.m = m; a.n_scenes = n_scenes; a.a_max = a_max; a.paths = paths; a.n_of = n_of;
    a.stop_before = stop_before; a.profile = profile; a.v_start = v_start; a.a_of = a_of; a.scene_of = scene_of; a.prm = *prm; a.frames = frames;
    a.blocked = blocked; a.parents = parents; a.steps = steps; a.traj = traj; a.cost = cost; a.reached = reached; a.flags = flags;
    const long long waves = (long long)batch * ((prm->stations + 63) / 64);
    return h->launch_timed([&]() -> int {
        if (const int rc = launch_agent_frames(h, n_scenes, a_max, m, agents, frames)) return rc;
        hipLaunchKernelGGL(pqp::st_occupancy_kernel, wave_grid(waves, pqp::kAgentsThreads), dim3(pqp::kAgentsThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        hipLaunchKernelGGL(pqp::st_search_kernel, dim3((unsigned)batch), dim3(pqp::kSearchThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_speed_search(pqp_handle* h, const pqp_search_params* prm, const pqp_car_geometry* car, int batch, int n, int stride,
                     const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start, int m,
                     int n_scenes, int a_max, const double* agents, const int32_t* a_of, const int32_t* scene_of, int32_t* blocked,
                     int32_t* steps, double* traj, double* cost, int32_t* reached, int32_t* flags) {
    if (!search_ok(h, prm, car, batch, n, stride, paths, profile, v_start, m, n_scenes, a_max, agents, steps, traj, cost, reached, flags))
        return fail(PQP_ERR_INVALID, kSearchRefusal);
    if (const int rc = index_range(scene_of, batch, n_scenes, "pqp_speed_search: scene_of outside [0, n_scenes)")) return rc;
    const size_t bn = (size_t)batch * n, bm = (size_t)batch * m;
    const size_t words = (size_t)(prm->stations + 31) / 32, states = (size_t)prm->stations * (prm->q_max + 1);
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_stop = st.in(stop_before, batch);
    const double* d_profile = st.in(profile, bn * PQP_SPEED_STRIDE);
    const double* d_start = st.in(v_start, batch);
    const AgentArrays d = stage_agents(st, n_scenes, a_max, m, agents, a_of, scene_of, batch);
    int32_t* d_blocked = st.out(blocked, bm * words);
    uint8_t* d_parents = st.out((uint8_t*)nullptr, bm * states);
    int32_t* d_steps = st.out(steps, bm * 2);
    double* d_traj = st.out(traj, bm * PQP_TRAJ_STRIDE);
    double* d_cost = st.out(cost, batch);
    int32_t* d_reached = st.out(reached, batch);
    int32_t* d_flags = st.out(flags, batch);
    return st.run([&]() -> int {
        return pqp_speed_search_device(h, prm, car, batch, n, stride, d_paths, d_n_of, d_stop, d_profile, d_start, m, n_scenes, a_max, d.agents,
                                       d.a_of, d.of, d.frames, d_blocked, d_parents, d_steps, d_traj, d_cost, d_reached, d_flags);
    });
}

// ---- searched speed plans made drivable: a jerk-limited speed QP ---------------------------------------------------------------------------
void pqp_refine_default_params(double* prm, int* window) {
    if (prm) {
        pqp_speed_params sp;
        pqp_speed_default_params(&sp);
        prm[PQP_REFINE_W_REF] = prm[PQP_REFINE_W_ACCEL] = prm[PQP_REFINE_W_JERK] = 1.0;
        prm[PQP_REFINE_A_MAX] = sp.a_max;
        prm[PQP_REFINE_D_MAX] = sp.d_max;
    }
    if (window) *window = 4;
}

static const char* const kRefineRefusal =
    "pqp_speed_refine: bad argument (batch >= 1; n >= 1; m >= 1; stride >= 6; dt and ds finite and > 0; 1 <= stations <= 4096; the three weights "
    "finite and >= 0, w_ref + w_accel > 0; a_max and d_max finite and > 0; window >= 0)";

static bool refine_ok(pqp_handle* h, const pqp_search_params* grid, const double* prm, int window, int batch, int n, int stride, const double* paths,
                      const double* profile, const double* v_start, int m, const int32_t* blocked, const int32_t* steps, const int32_t* reached,
                      const double* search_traj, const double* traj, const double* cost, const int32_t* status, const int32_t* iters,
                      const int32_t* flags) {
    if (!(h && grid && prm && paths && profile && v_start && blocked && steps && reached && search_traj && traj && cost && status && iters && flags &&
          batch >= 1 && n >= 1 && m >= 1 && stride >= 6 && window >= 0))
        return false;
    const auto weight = [](double v) { return std::isfinite(v) && v >= 0.0; };
    const auto limit = [](double v) { return std::isfinite(v) && v > 0.0; };
    return limit(grid->dt) && limit(grid->ds) && grid->stations >= 1 && grid->stations <= PQP_SEARCH_MAX_STATES && weight(prm[PQP_REFINE_W_REF]) &&
           weight(prm[PQP_REFINE_W_ACCEL]) && weight(prm[PQP_REFINE_W_JERK]) && prm[PQP_REFINE_W_REF] + prm[PQP_REFINE_W_ACCEL] > 0.0 &&
           limit(prm[PQP_REFINE_A_MAX]) && limit(prm[PQP_REFINE_D_MAX]);
}

// the layers the banded core holds in one CU's LDS: sm_generic_fits is monotone in m
static bool refine_fits(int m) { return m < 2 || sm_generic_fits(kBandedRefine, m); }

int pqp_speed_refine_device(pqp_handle* h, const pqp_search_params* grid, const double* prm, int window, int batch, int n, int stride,
                            const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start,
                            int m, const int32_t* blocked, const int32_t* steps, const int32_t* reached, const double* search_traj,
                            double* traj, double* bounds, double* cost, double* excess, int32_t* status, int32_t* iters, int32_t* flags) {
    if (!refine_ok(h, grid, prm, window, batch, n, stride, paths, profile, v_start, m, blocked, steps, reached, search_traj, traj, cost, status, iters, flags))
        return fail(PQP_ERR_INVALID, kRefineRefusal);
    if (!refine_fits(m)) return fail(PQP_ERR_CAPACITY, "pqp_speed_refine: the QP of m layers is beyond what the banded core holds in one CU's LDS");
    PQP_HIP(hipSetDevice(h->device));
    const bool solve = m >= 2;               // m = 1: every path is kept, there is no QP to assemble or solve
    int rc;
    if ((rc = h->rf.bounds.ensure((size_t)batch * m * 3 * 8))) return rc;
    if (solve && (rc = sm_alloc(h, h->rf, kBandedRefine, batch, m))) return rc;
    pqp::RefineArgs a;
    a.batch = batch; a.n = n; a.stride = stride; a.m = m; a.stations = grid->stations; a.window = window;
    a.dt = grid->dt; a.ds = grid->ds; a.w_ref = prm[PQP_REFINE_W_REF]; a.w_accel = prm[PQP_REFINE_W_ACCEL]; a.w_jerk = prm[PQP_REFINE_W_JERK];
    a.a_max = prm[PQP_REFINE_A_MAX]; a.d_max = prm[PQP_REFINE_D_MAX];
    a.paths = paths; a.n_of = n_of; a.stop_before = stop_before; a.profile = profile; a.v_start = v_start; a.blocked = blocked; a.steps = steps;
    a.reached = reached; a.search_traj = search_traj; a.corridor = h->rf.bounds.as<double>();
    a.pband = h->rf.pband.as<double>(); a.q = h->rf.q.as<double>(); a.aval = h->rf.aval.as<double>(); a.lo = h->rf.lo.as<double>();
    a.up = h->rf.up.as<double>(); a.x = h->rf.x.as<double>();
    a.traj = traj; a.bounds = bounds; a.cost = cost; a.excess = excess; a.status = status; a.iters = iters; a.flags = flags;
    // always the exact optimum: the production tolerances with the KKT-verified polish, whatever the handle's path-QP setting
    pqp_params exact;
    pqp::production_params(&exact);
    exact.polish = 1;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::st_corridor_kernel, dim3((unsigned)batch), dim3(pqp::kRefineThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        if (solve) {
            const long long total = (long long)batch * m;
            hipLaunchKernelGGL(pqp::refine_assemble_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, a);
            PQP_HIP(hipGetLastError());
            if (const int rc2 = sm_solve(h, h->rf, exact, kBandedRefine, batch, m, nullptr, status, iters, nullptr, false)) return rc2;
        }
        hipLaunchKernelGGL(pqp::refine_finish_kernel, dim3((unsigned)batch), dim3(pqp::kRefineThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_speed_refine(pqp_handle* h, const pqp_search_params* grid, const double* prm, int window, int batch, int n, int stride,
                     const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start, int m,
                     const int32_t* blocked, const int32_t* steps, const int32_t* reached, const double* search_traj, double* traj,
                     double* bounds, double* cost, double* excess, int32_t* status, int32_t* iters, int32_t* flags) {
    if (!refine_ok(h, grid, prm, window, batch, n, stride, paths, profile, v_start, m, blocked, steps, reached, search_traj, traj, cost, status, iters, flags))
        return fail(PQP_ERR_INVALID, kRefineRefusal);
    if (!refine_fits(m)) return fail(PQP_ERR_CAPACITY, "pqp_speed_refine: the QP of m layers is beyond what the banded core holds in one CU's LDS");
    const size_t bn = (size_t)batch * n, bm = (size_t)batch * m, words = (size_t)(grid->stations + 31) / 32;
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_stop = st.in(stop_before, batch);
    const double* d_profile = st.in(profile, bn * PQP_SPEED_STRIDE);
    const double* d_start = st.in(v_start, batch);
    const int32_t* d_blocked = st.in(blocked, bm * words);
    const int32_t* d_steps = st.in(steps, bm * 2);
    const int32_t* d_reached = st.in(reached, batch);
    const double* d_from = st.in(search_traj, bm * PQP_TRAJ_STRIDE);
    double* d_traj = st.out(traj, bm * PQP_TRAJ_STRIDE);
    double* d_bounds = bounds ? st.out(bounds, bm * 3) : nullptr;
    double* d_cost = st.out(cost, batch);
    double* d_excess = excess ? st.out(excess, batch) : nullptr;
    int32_t* d_status = st.out(status, batch);
    int32_t* d_iters = st.out(iters, batch);
    int32_t* d_flags = st.out(flags, batch);
    return st.run([&]() -> int {
        return pqp_speed_refine_device(h, grid, prm, window, batch, n, stride, d_paths, d_n_of, d_stop, d_profile, d_start, m, d_blocked, d_steps,
                                       d_reached, d_from, d_traj, d_bounds, d_cost, d_excess, d_status, d_iters, d_flags);
    });
}

// ---- speed plans on a fine time step --------------------------------------------------------------------------------------------------------
static const char* const kPlanRefusal =
    "pqp_sample_plan: bad argument (batch >= 1; n >= 1; m >= 1; r >= 1; stride >= 6; dt finite and > 0; linear 0 or 1; (m - 1) * r + 1 <= INT_MAX)";

static bool plan_ok(pqp_handle* h, double dt, int r, int linear, int batch, int n, int stride, const double* paths, const double* profile, int m,
                    const double* plan, const double* fine, const int32_t* m_of, const int32_t* flags) {
    return h && paths && profile && plan && fine && m_of && flags && batch >= 1 && n >= 1 && m >= 1 && r >= 1 && stride >= 6 && std::isfinite(dt) &&
           dt > 0.0 && (linear == 0 || linear == 1) && (long long)(m - 1) * r + 1 <= INT_MAX;
}

int pqp_sample_plan_device(pqp_handle* h, double dt, int r, int linear, int batch, int n, int stride, const double* paths,
                           const int32_t* n_of, const int32_t* stop_before, const double* profile, int m, const double* plan,
                           const int32_t* count_of, const int32_t* refine_flags, double* fine, int32_t* m_of, double* defect,
                           double* excess, int32_t* flags) {
    if (!plan_ok(h, dt, r, linear, batch, n, stride, paths, profile, m, plan, fine, m_of, flags)) return fail(PQP_ERR_INVALID, kPlanRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::PlanArgs a;
    a.batch = batch; a.n = n; a.stride = stride; a.m = m; a.r = r; a.linear = linear; a.dt = dt; a.paths = paths; a.n_of = n_of;
    a.stop_before = stop_before; a.profile = profile; a.plan = plan; a.count_of = count_of; a.refine_flags = refine_flags; a.fine = fine;
    a.m_of = m_of; a.defect = defect; a.excess = excess; a.flags = flags;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::plan_sample_kernel, wave_grid(batch, pqp::kPlanThreads), dim3(pqp::kPlanThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_sample_plan(pqp_handle* h, double dt, int r, int linear, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                    const int32_t* stop_before, const double* profile, int m, const double* plan, const int32_t* count_of,
                    const int32_t* refine_flags, double* fine, int32_t* m_of, double* defect, double* excess, int32_t* flags) {
    if (!plan_ok(h, dt, r, linear, batch, n, stride, paths, profile, m, plan, fine, m_of, flags)) return fail(PQP_ERR_INVALID, kPlanRefusal);
    const size_t bn = (size_t)batch * n, fine_rows = (size_t)batch * ((size_t)(m - 1) * r + 1);
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_stop = st.in(stop_before, batch);
    const double* d_profile = st.in(profile, bn * PQP_SPEED_STRIDE);
    const double* d_plan = st.in(plan, (size_t)batch * m * PQP_TRAJ_STRIDE);
    const int32_t* d_count = st.in(count_of, batch);
    const int32_t* d_rflags = st.in(refine_flags, batch);
    double* d_fine = st.out(fine, fine_rows * PQP_TRAJ_STRIDE);
    int32_t* d_m_of = st.out(m_of, batch);
    double* d_defect = defect ? st.out(defect, batch) : nullptr;
    double* d_excess = excess ? st.out(excess, batch) : nullptr;
    int32_t* d_flags = st.out(flags, batch);
    return st.run([&]() -> int {
        return pqp_sample_plan_device(h, dt, r, linear, batch, n, stride, d_paths, d_n_of, d_stop, d_profile, m, d_plan, d_count, d_rflags, d_fine,
                                      d_m_of, d_defect, d_excess, d_flags);
    });
}

}  // extern "C"
