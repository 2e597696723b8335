// pqp_select.hip — the entry points of include/pqp.h that choose: scores of candidate paths and each group's best
// (pqp_select_kernels.inc), scores of the finished trajectories and each group's best (pqp_rank_kernels.inc), and the start of the next
// cycle on the winner a cycle left (pqp_stitch_kernels.inc), and the braking plans of a group that ends without a winner
// (pqp_fallback_kernels.inc).  Their kernels, launchers and entry points.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "pqp_defaults.hpp"
#include "pqp_internal.hpp"

using namespace pqp_internal;

#include "pqp_select_kernels.inc"
#include "pqp_rank_kernels.inc"
#include "pqp_stitch_kernels.inc"
#include "pqp_fallback_kernels.inc"

extern "C" {

// ---- scores of candidate paths and each group's best ----------------------------------------------------------------------------------
void pqp_select_default_params(pqp_select_params* p) {
    if (!p) return;
    pqp_params d;
    pqp::default_params(&d);
    p->weight_kappa = d.weight_kappa;          // base_solver.cpp:124
    p->weight_dkappa = d.weight_dkappa;        // :125
    p->weight_offset = 0.0;                    // :123: weight_l is 0
    p->weight_length = 0.0;
    p->weight_clearance = 0.0;
    p->clearance_want = d.expected_safety_margin;      // FLAGS_expected_safety_margin, planning_flags.cpp:95
    p->per_waypoint = 0;
    p->require_free = 1;
}

static bool select_ok(pqp_handle* h, const pqp_select_params* prm, int batch, int n, int stride, const double* paths, int groups,
                      const int32_t* group_start, const double* terms, const int32_t* best, const double* best_paths, const int32_t* best_n) {
    return h && prm && paths && group_start && terms && best && batch >= 1 && n >= 1 && n <= (1 << 30) && stride >= 7 && groups >= 0 &&
           (best_paths != nullptr) == (best_n != nullptr);
}

int pqp_select_paths_device(pqp_handle* h, const pqp_select_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                            const int32_t* status, const int32_t* stage, const int32_t* first_collision, const double* margin, int groups,
                            const int32_t* group_start, double* terms, int32_t* best, double* best_paths, int32_t* best_n) {
    if (!select_ok(h, prm, batch, n, stride, paths, groups, group_start, terms, best, best_paths, best_n))
        return fail(PQP_ERR_INVALID, "pqp_select_paths: bad argument (stride >= 7; groups >= 0; best_paths and best_n both or neither)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::SelectArgs a;
    a.batch = batch; a.n = n; a.stride = stride; a.groups = groups; a.paths = paths; a.n_of = n_of; a.status = status; a.stage = stage;
    a.first_collision = first_collision; a.margin = margin; a.group_start = group_start; a.prm = *prm; a.terms = terms; a.best = best;
    a.best_paths = best_paths; a.best_n = best_n;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::path_score_kernel, wave_grid(batch, pqp::kSelectThreads), dim3(pqp::kSelectThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        if (groups > 0) {
            hipLaunchKernelGGL(pqp::group_select_kernel, wave_grid(groups, pqp::kSelectThreads), dim3(pqp::kSelectThreads), 0, h->stream, a);
            PQP_HIP(hipGetLastError());
        }
        return PQP_OK;
    });
}

int pqp_select_paths(pqp_handle* h, const pqp_select_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                     const int32_t* status, const int32_t* stage, const int32_t* first_collision, const double* margin, int groups,
                     const int32_t* group_start, double* terms, int32_t* best, double* best_paths, int32_t* best_n) {
    if (!select_ok(h, prm, batch, n, stride, paths, groups, group_start, terms, best, best_paths, best_n))
        return fail(PQP_ERR_INVALID, "pqp_select_paths: bad argument (stride >= 7; groups >= 0; best_paths and best_n both or neither)");
    for (const double v : {prm->weight_kappa, prm->weight_dkappa, prm->weight_offset, prm->weight_length, prm->weight_clearance, prm->clearance_want})
        if (!std::isfinite(v)) return fail(PQP_ERR_INVALID, "pqp_select_paths: a parameter that is not finite");
    if (const int rc = group_start_ok("pqp_select_paths", group_start, groups, batch)) return rc;
    // (from here on groups >= 1: group_start runs from 0 to batch >= 1)
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_paths = st.in(paths, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const int32_t* d_status = st.in(status, batch);
    const int32_t* d_stage = st.in(stage, batch);
    const int32_t* d_first = st.in(first_collision, batch);
    const double* d_margin = st.in(margin, bn);
    const int32_t* d_start = st.in(group_start, (size_t)groups + 1);
    double* d_terms = st.out(terms, (size_t)batch * PQP_SCORE_STRIDE);
    int32_t* d_best = st.out(best, groups);
    double* d_best_paths = best_paths ? st.out(best_paths, (size_t)groups * n * 7) : nullptr;
    int32_t* d_best_n = best_n ? st.out(best_n, groups) : nullptr;
    return st.run([&]() -> int {
        return pqp_select_paths_device(h, prm, batch, n, stride, d_paths, d_n_of, d_status, d_stage, d_first, d_margin, groups, d_start, d_terms,
                                       d_best, d_best_paths, d_best_n);
    });
}

// ---- scores of finished trajectories and each group's best ---------------------------------------------------------------------------------
void pqp_rank_default_params(double* prm, int* require_free) {
    if (prm) {
        pqp_select_params sel;
        pqp_select_default_params(&sel);
        // this library's choice: the reference has no speed plan to weigh against its path
        prm[PQP_RANK_W_PATH] = prm[PQP_RANK_W_PROGRESS] = prm[PQP_RANK_W_ACCEL] = prm[PQP_RANK_W_JUMP] = prm[PQP_RANK_W_LATERAL] = 1.0;
        prm[PQP_RANK_W_CLEARANCE] = 0.0;
        prm[PQP_RANK_CLEARANCE_WANT] = sel.clearance_want;
    }
    if (require_free) *require_free = 1;
}

static const char* const kRankRefusal =
    "pqp_select_plans: bad argument (batch >= 1; m >= 1; stride >= 8; with paths n >= 1 and path_stride >= 7; groups >= 0; best_traj and best_m "
    "both or neither; best_paths and best_n both or neither, and only with paths; every parameter finite; require_free 0 or 1)";

static bool rank_ok(pqp_handle* h, const double* prm, int require_free, int batch, int m, int stride, const double* traj, int n, int path_stride,
                    const double* paths, int groups, const int32_t* group_start, const double* terms, const int32_t* best, const double* best_traj,
                    const int32_t* best_m, const double* best_paths, const int32_t* best_n) {
    if (!(h && prm && traj && group_start && terms && best && batch >= 1 && m >= 1 && stride >= PQP_TRAJ_STRIDE && groups >= 0)) return false;
    if (paths && !(n >= 1 && n <= (1 << 30) && path_stride >= 7)) return false;
    if ((best_traj != nullptr) != (best_m != nullptr) || (best_paths != nullptr) != (best_n != nullptr) || (best_paths && !paths)) return false;
    for (int k = 0; k < PQP_RANK_PARAMS; ++k)
        if (!std::isfinite(prm[k])) return false;
    return require_free == 0 || require_free == 1;
}

int pqp_select_plans_device(pqp_handle* h, const double* prm, int require_free, int batch, int m, int stride, const double* traj,
                            const int32_t* m_of, const double* path_terms, const int32_t* search_flags, const int32_t* first_hit,
                            const double* clearance, int n, int path_stride, const double* paths, const int32_t* n_of, int groups,
                            const int32_t* group_start, double* terms, int32_t* best, double* best_traj, int32_t* best_m, double* best_paths,
                            int32_t* best_n) {
    if (!rank_ok(h, prm, require_free, batch, m, stride, traj, n, path_stride, paths, groups, group_start, terms, best, best_traj, best_m, best_paths, best_n))
        return fail(PQP_ERR_INVALID, kRankRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::RankArgs a;
    a.batch = batch; a.m = m; a.stride = stride; a.n = n; a.path_stride = path_stride; a.groups = groups; a.require_free = require_free;
    a.traj = traj; a.m_of = m_of; a.path_terms = path_terms; a.search_flags = search_flags; a.first_hit = first_hit; a.clearance = clearance;
    a.paths = paths; a.n_of = n_of; a.group_start = group_start;
    for (int k = 0; k < PQP_RANK_PARAMS; ++k) a.prm[k] = prm[k];
    a.terms = terms; a.best = best; a.best_traj = best_traj; a.best_m = best_m; a.best_paths = best_paths; a.best_n = best_n;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::plan_score_kernel, wave_grid(batch, pqp::kRankThreads), dim3(pqp::kRankThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        if (groups > 0) {
            hipLaunchKernelGGL(pqp::plan_group_kernel, wave_grid(groups, pqp::kRankThreads), dim3(pqp::kRankThreads), 0, h->stream, a);
            PQP_HIP(hipGetLastError());
        }
        return PQP_OK;
    });
}

int pqp_select_plans(pqp_handle* h, const double* prm, int require_free, int batch, int m, int stride, const double* traj, const int32_t* m_of,
                     const double* path_terms, const int32_t* search_flags, const int32_t* first_hit, const double* clearance, int n,
                     int path_stride, const double* paths, const int32_t* n_of, int groups, const int32_t* group_start, double* terms,
                     int32_t* best, double* best_traj, int32_t* best_m, double* best_paths, int32_t* best_n) {
    if (!rank_ok(h, prm, require_free, batch, m, stride, traj, n, path_stride, paths, groups, group_start, terms, best, best_traj, best_m, best_paths, best_n))
        return fail(PQP_ERR_INVALID, kRankRefusal);
    if (const int rc = group_start_ok("pqp_select_plans", group_start, groups, batch)) return rc;
    // (from here on groups >= 1: group_start runs from 0 to batch >= 1)
    const size_t bm = (size_t)batch * m;
    Staging st(h);
    const double* d_traj = st.in(traj, bm * stride);
    const int32_t* d_m_of = st.in(m_of, batch);
    const double* d_path_terms = st.in(path_terms, (size_t)batch * PQP_SCORE_STRIDE);
    const int32_t* d_sflags = st.in(search_flags, batch);
    const int32_t* d_first = st.in(first_hit, batch);
    const double* d_clear = st.in(clearance, bm);
    const double* d_paths = paths ? st.in(paths, (size_t)batch * n * path_stride) : nullptr;
    const int32_t* d_n_of = paths ? st.in(n_of, batch) : nullptr;
    const int32_t* d_start = st.in(group_start, (size_t)groups + 1);
    double* d_terms = st.out(terms, (size_t)batch * PQP_PLAN_SCORE_STRIDE);
    int32_t* d_best = st.out(best, groups);
    double* d_best_traj = best_traj ? st.out(best_traj, (size_t)groups * m * PQP_TRAJ_STRIDE) : nullptr;
    int32_t* d_best_m = best_m ? st.out(best_m, groups) : nullptr;
    double* d_best_paths = best_paths ? st.out(best_paths, (size_t)groups * n * 7) : nullptr;
    int32_t* d_best_n = best_n ? st.out(best_n, groups) : nullptr;
    return st.run([&]() -> int {
        return pqp_select_plans_device(h, prm, require_free, batch, m, stride, d_traj, d_m_of, d_path_terms, d_sflags, d_first, d_clear, n, path_stride,
                                       d_paths, d_n_of, groups, d_start, d_terms, d_best, d_best_traj, d_best_m, d_best_paths, d_best_n);
    });
}

// ---- the start of a cycle from the previous cycle's plan -------------------------------------------------------------------------------------
void pqp_stitch_default_params(double* prm, int* keep) {
    if (prm) {
        // this library's choice: the reference plans from the state it is given
        prm[PQP_STITCH_T_AHEAD] = 0.1;
        prm[PQP_STITCH_LAT_MAX] = 0.5;
        prm[PQP_STITCH_LON_MAX] = 2.5;
        prm[PQP_STITCH_DH_MAX] = 0.5;
        prm[PQP_STITCH_V_STILL] = 0.1;
        prm[PQP_STITCH_V_CAP] = INFINITY;
    }
    if (keep) *keep = 20;
}

static const char* const kStitchRefusal =
    "pqp_stitch_trajectory: bad argument (groups >= 1; m >= 1; stride >= 8; batch >= 0; keep >= 0; with prefix prefix_max >= 1; t_ahead and "
    "v_still finite and >= 0; lat_max, lon_max, dh_max and v_cap >= 0; without group_start and with start, start_k or v_start batch = groups)";

static bool stitch_ok(pqp_handle* h, const double* prm, int keep, int prefix_max, int groups, int m, int stride, const double* prev,
                      const double* meas, const double* t_now, int batch, const int32_t* group_start, const double* state, const int32_t* flags,
                      const double* dev, const int32_t* idx, const double* prefix, const int32_t* prefix_n, const double* start, const double* start_k,
                      const double* v_start) {
    if (!(h && prm && prev && meas && t_now && state && flags && dev && idx && prefix_n)) return false;
    if (!(groups >= 1 && m >= 1 && stride >= PQP_TRAJ_STRIDE && batch >= 0 && keep >= 0 && (!prefix || prefix_max >= 1))) return false;
    for (int k = 0; k < PQP_STITCH_PARAMS; ++k)
        if (!(prm[k] >= 0.0)) return false;                                // (a NaN fails it too)
    if (!(std::isfinite(prm[PQP_STITCH_T_AHEAD]) && std::isfinite(prm[PQP_STITCH_V_STILL]))) return false;
    return group_start || !(start || start_k || v_start) || batch == groups;
}

int pqp_stitch_trajectory_device(pqp_handle* h, const double* prm, int keep, int prefix_max, int groups, int m, int stride, const double* prev,
                                 const int32_t* m_of, const double* meas, const double* t_now, int batch, const int32_t* group_start,
                                 double* state, int32_t* flags, double* dev, int32_t* idx, double* prefix, int32_t* prefix_n, double* start,
                                 double* start_k, double* v_start) {
    if (!stitch_ok(h, prm, keep, prefix_max, groups, m, stride, prev, meas, t_now, batch, group_start, state, flags, dev, idx, prefix, prefix_n, start,
                   start_k, v_start))
        return fail(PQP_ERR_INVALID, kStitchRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::StitchArgs a;
    a.groups = groups; a.m = m; a.stride = stride; a.batch = batch; a.keep = keep; a.prefix_max = prefix ? prefix_max : 0;
    a.t_ahead = prm[PQP_STITCH_T_AHEAD]; a.lat_max = prm[PQP_STITCH_LAT_MAX]; a.lon_max = prm[PQP_STITCH_LON_MAX]; a.dh_max = prm[PQP_STITCH_DH_MAX];
    a.v_still = prm[PQP_STITCH_V_STILL]; a.v_cap = prm[PQP_STITCH_V_CAP];
    a.prev = prev; a.m_of = m_of; a.meas = meas; a.t_now = t_now; a.group_start = group_start;
    a.state = state; a.flags = flags; a.dev = dev; a.idx = idx; a.prefix = prefix; a.prefix_n = prefix_n; a.start = start; a.start_k = start_k;
    a.v_start = v_start;
    return h->launch_timed([&]() -> int {
        const long long blocks = ((long long)groups + pqp::kStitchThreads / 64 - 1) / (pqp::kStitchThreads / 64);
        hipLaunchKernelGGL(pqp::stitch_trajectory_kernel, dim3((unsigned)std::min(blocks, pqp::kStitchMaxBlocks)), dim3(pqp::kStitchThreads), 0,
                           h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_stitch_trajectory(pqp_handle* h, const double* prm, int keep, int prefix_max, int groups, int m, int stride, const double* prev,
                          const int32_t* m_of, const double* meas, const double* t_now, int batch, const int32_t* group_start, double* state,
                          int32_t* flags, double* dev, int32_t* idx, double* prefix, int32_t* prefix_n, double* start, double* start_k,
                          double* v_start) {
    if (!stitch_ok(h, prm, keep, prefix_max, groups, m, stride, prev, meas, t_now, batch, group_start, state, flags, dev, idx, prefix, prefix_n, start,
                   start_k, v_start))
        return fail(PQP_ERR_INVALID, kStitchRefusal);
    if (group_start)
        if (const int rc = group_start_ok("pqp_stitch_trajectory", group_start, groups, batch)) return rc;
    const size_t G = groups;
    Staging st(h);
    const double* d_prev = st.in(prev, G * m * stride);
    const int32_t* d_m_of = st.in(m_of, G);
    const double* d_meas = st.in(meas, G * 6);
    const double* d_t_now = st.in(t_now, G);
    const int32_t* d_start_of = st.in(group_start, G + 1);
    double* d_state = st.out(state, G * PQP_TRAJ_STRIDE);
    int32_t* d_flags = st.out(flags, G);
    double* d_dev = st.out(dev, G * 3);
    int32_t* d_idx = st.out(idx, G * 3);
    double* d_prefix = prefix ? st.out(prefix, G * prefix_max * PQP_TRAJ_STRIDE) : nullptr;
    int32_t* d_prefix_n = st.out(prefix_n, G);
    // (every candidate is in one group here: group_start runs from 0 to batch, or there is none and batch = groups)
    double* d_start = start && batch ? st.out(start, (size_t)batch * 3) : nullptr;
    double* d_start_k = start_k && batch ? st.out(start_k, batch) : nullptr;
    double* d_v_start = v_start && batch ? st.out(v_start, batch) : nullptr;
    return st.run([&]() -> int {
        return pqp_stitch_trajectory_device(h, prm, keep, prefix_max, groups, m, stride, d_prev, d_m_of, d_meas, d_t_now, batch, d_start_of, d_state,
                                            d_flags, d_dev, d_idx, d_prefix, d_prefix_n, d_start, d_start_k, d_v_start);
    });
}

// ---- a plan for every group: braking fallbacks where no candidate wins ------------------------------------------------------------------------
void pqp_fallback_default_params(double* prm, double* levels, int* n_levels) {
    pqp_speed_params sp;
    pqp_speed_default_params(&sp);
    if (prm) prm[PQP_FALLBACK_A_CAP] = sp.a_max;
    if (levels) {
        // this library's choice (include/pqp.h cites it): half of d_max, d_max, twice d_max
        levels[0] = 0.5 * sp.d_max; levels[1] = 2.5;
        levels[2] = sp.d_max;       levels[3] = 5.0;
        levels[4] = 2.0 * sp.d_max; levels[5] = 15.0;
    }
    if (n_levels) *n_levels = PQP_FALLBACK_DEFAULT_LEVELS;
}

static const char* const kFallbackRowsRefusal =
    "pqp_fallback_rows: bad argument (groups >= 1; 1 <= n_levels <= 8 and groups * n_levels within an int; every level's d and j finite and > 0, "
    "d ascending; a_cap >= 0; dt finite and > 0; r >= 1; m >= 1; (m - 1) r + 1 <= INT_MAX - 64; with prev mp >= 1 and stride >= 8; prev_m only with prev)";

static bool fallback_rows_ok(pqp_handle* h, const double* prm, int n_levels, const double* levels, double dt, int r, int m, int groups, int mp,
                             int stride, const double* prev, const int32_t* prev_m, const double* state, const double* rows, const double* stop,
                             const int32_t* stop_row, const int32_t* flags) {
    if (!(h && prm && levels && state && rows && stop && stop_row && flags)) return false;
    if (!(groups >= 1 && n_levels >= 1 && n_levels <= PQP_FALLBACK_MAX_LEVELS && (long long)groups * n_levels <= INT_MAX)) return false;
    if (!(std::isfinite(dt) && dt > 0.0 && r >= 1 && m >= 1 && ((long long)m - 1) * r + 1 <= pqp::kFallbackMaxRows)) return false;
    if (prev ? !(mp >= 1 && stride >= PQP_TRAJ_STRIDE) : prev_m != nullptr) return false;
    if (!(prm[PQP_FALLBACK_A_CAP] >= 0.0)) return false;                       // (a NaN fails it too)
    for (int l = 0; l < n_levels; ++l) {
        const double d = levels[2 * l], j = levels[2 * l + 1];
        if (!(std::isfinite(d) && std::isfinite(j) && d > 0.0 && j > 0.0) || (l > 0 && !(d >= levels[2 * l - 2]))) return false;
    }
    return true;
}

int pqp_fallback_rows_device(pqp_handle* h, const double* prm, int n_levels, const double* levels, double dt, int r, int m, int groups, int mp,
                             int stride, const double* prev, const int32_t* prev_m, const double* state, const int32_t* stitch_flags, double* rows,
                             double* stop, int32_t* stop_row, int32_t* flags) {
    if (!fallback_rows_ok(h, prm, n_levels, levels, dt, r, m, groups, mp, stride, prev, prev_m, state, rows, stop, stop_row, flags))
        return fail(PQP_ERR_INVALID, kFallbackRowsRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::FallbackArgs a;
    a.groups = groups; a.levels = n_levels; a.mp = prev ? mp : 0; a.stride = prev ? stride : PQP_TRAJ_STRIDE; a.r = r; a.M = (m - 1) * r + 1;
    a.dt = dt; a.a_cap = prm[PQP_FALLBACK_A_CAP];
    for (int l = 0; l < PQP_FALLBACK_MAX_LEVELS; ++l) {
        a.level[l][0] = l < n_levels ? levels[2 * l] : 0.0;
        a.level[l][1] = l < n_levels ? levels[2 * l + 1] : 0.0;
    }
    a.prev = prev; a.prev_m = prev_m; a.state = state; a.stitch_flags = stitch_flags;
    a.rows = rows; a.stop = stop; a.stop_row = stop_row; a.flags = flags;
    return h->launch_timed([&]() -> int {
        const long long items = (long long)groups * n_levels;
        const long long blocks = (items + pqp::kFallbackThreads / 64 - 1) / (pqp::kFallbackThreads / 64);
        hipLaunchKernelGGL(pqp::fallback_rows_kernel, dim3((unsigned)std::min(blocks, pqp::kFallbackMaxBlocks)), dim3(pqp::kFallbackThreads), 0,
                           h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_fallback_rows(pqp_handle* h, const double* prm, int n_levels, const double* levels, double dt, int r, int m, int groups, int mp, int stride,
                      const double* prev, const int32_t* prev_m, const double* state, const int32_t* stitch_flags, double* rows, double* stop,
                      int32_t* stop_row, int32_t* flags) {
    if (!fallback_rows_ok(h, prm, n_levels, levels, dt, r, m, groups, mp, stride, prev, prev_m, state, rows, stop, stop_row, flags))
        return fail(PQP_ERR_INVALID, kFallbackRowsRefusal);
    const size_t G = groups, items = G * n_levels, M = (size_t)(m - 1) * r + 1;
    Staging st(h);
    const double* d_prev = prev ? st.in(prev, G * mp * stride) : nullptr;
    const int32_t* d_prev_m = st.in(prev_m, G);
    const double* d_state = st.in(state, G * PQP_TRAJ_STRIDE);
    const int32_t* d_sflags = st.in(stitch_flags, G);
    double* d_rows = st.out(rows, items * M * PQP_TRAJ_STRIDE);
    double* d_stop = st.out(stop, items * 2);
    int32_t* d_stop_row = st.out(stop_row, items);
    int32_t* d_flags = st.out(flags, items);
    return st.run([&]() -> int {
        return pqp_fallback_rows_device(h, prm, n_levels, levels, dt, r, m, groups, mp, stride, d_prev, d_prev_m, d_state, d_sflags, d_rows, d_stop,
                                        d_stop_row, d_flags);
    });
}

static const char* const kFallbackPickRefusal =
    "pqp_fallback_pick: bad argument (groups >= 1; 1 <= n_levels <= 8 and groups * n_levels within an int; 1 <= m_rows <= INT_MAX - 64; best_traj and best_m both "
    "or neither)";

static bool fallback_pick_ok(pqp_handle* h, int groups, int n_levels, int m_rows, const double* best_traj, const int32_t* best_m, const double* rows,
                             const int32_t* row_flags, const double* final_traj, const int32_t* final_m, const int32_t* level, const int32_t* flags) {
    return h && rows && row_flags && final_traj && final_m && level && flags && groups >= 1 && n_levels >= 1 && n_levels <= PQP_FALLBACK_MAX_LEVELS &&
           (long long)groups * n_levels <= INT_MAX && m_rows >= 1 && m_rows <= pqp::kFallbackMaxRows && (best_traj != nullptr) == (best_m != nullptr);
}

int pqp_fallback_pick_device(pqp_handle* h, int groups, int n_levels, int m_rows, const int32_t* best, const double* best_traj, const int32_t* best_m,
                             const double* rows, const int32_t* row_flags, const int32_t* first_hit, const int32_t* first_collision,
                             double* final_traj, int32_t* final_m, int32_t* level, int32_t* flags) {
    if (!fallback_pick_ok(h, groups, n_levels, m_rows, best_traj, best_m, rows, row_flags, final_traj, final_m, level, flags))
        return fail(PQP_ERR_INVALID, kFallbackPickRefusal);
    PQP_HIP(hipSetDevice(h->device));
    pqp::FallbackPickArgs a;
    a.groups = groups; a.levels = n_levels; a.M = m_rows; a.best = best; a.best_traj = best_traj; a.best_m = best_m; a.rows = rows;
    a.row_flags = row_flags; a.first_hit = first_hit; a.first_collision = first_collision; a.final_traj = final_traj; a.final_m = final_m;
    a.level = level; a.flags = flags;
    return h->launch_timed([&]() -> int {
        const long long blocks = ((long long)groups + pqp::kFallbackThreads / 64 - 1) / (pqp::kFallbackThreads / 64);
        hipLaunchKernelGGL(pqp::fallback_pick_kernel, dim3((unsigned)std::min(blocks, pqp::kFallbackMaxBlocks)), dim3(pqp::kFallbackThreads), 0,
                           h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_fallback_pick(pqp_handle* h, int groups, int n_levels, int m_rows, const int32_t* best, const double* best_traj, const int32_t* best_m,
                      const double* rows, const int32_t* row_flags, const int32_t* first_hit, const int32_t* first_collision, double* final_traj,
                      int32_t* final_m, int32_t* level, int32_t* flags) {
    if (!fallback_pick_ok(h, groups, n_levels, m_rows, best_traj, best_m, rows, row_flags, final_traj, final_m, level, flags))
        return fail(PQP_ERR_INVALID, kFallbackPickRefusal);
    const size_t G = groups, items = G * n_levels, cells = (size_t)m_rows * PQP_TRAJ_STRIDE;
    Staging st(h);
    const int32_t* d_best = st.in(best, G);
    const double* d_best_traj = st.in(best_traj, G * cells);
    const int32_t* d_best_m = st.in(best_m, G);
    const double* d_rows = st.in(rows, items * cells);
    const int32_t* d_rflags = st.in(row_flags, items);
    const int32_t* d_hit = st.in(first_hit, items);
    const int32_t* d_col = st.in(first_collision, items);
    double* d_final = st.out(final_traj, G * cells);
    int32_t* d_final_m = st.out(final_m, G);
    int32_t* d_level = st.out(level, G);
    int32_t* d_flags = st.out(flags, G);
    return st.run([&]() -> int {
        return pqp_fallback_pick_device(h, groups, n_levels, m_rows, d_best, d_best_traj, d_best_m, d_rows, d_rflags, d_hit, d_col, d_final, d_final_m,
                                        d_level, d_flags);
    });
}

}  // extern "C"
