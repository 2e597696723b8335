// pqp_rank_kernels.inc — instantiated by pqp_select.hip behind pqp_select_kernels.inc, whose group_rows and group_least it uses;
// includes nothing of its own.  Scores of finished trajectories - a path and the speed plan on it - and each group's best
// (pqp_select_plans): the last stage of the path-speed decoupled planner, behind pqp_speed_refine,
// pqp_sample_plan and the fine pqp_agents_check on the same stream.  The reference plans one path per call and has no time axis; it has
// nothing to rank.  include/pqp.h states the definition operation by operation.
// plan_score_kernel: one wavefront per candidate, four per workgroup, lanes striding over its samples; a wavefront's 64 rows are one
// contiguous span of `traj`, lane i also reads row i + 1's a and t for the differences.  Every lane adds its own samples in ascending order
// and the 64 partial sums meet in wave_sum, so the order of the additions depends on the candidate's count alone: the same candidate gives
// the same bits wherever it stands in whatever batch.  plan_group_kernel: one wavefront per group over the 80-byte records the first kernel
// wrote, by group_select_kernel's rule (group_rows, group_least of pqp_select_kernels.inc), then the two gathers of the winner's rows.
// No LDS, no scratch, nothing but plain stores.

namespace pqp {

constexpr int kRankThreads = 256;

struct RankArgs {
    int batch, m, stride, n, path_stride, groups, require_free;
    const double* traj;              // [batch][m][stride]  k, s, v, a, t at offsets 3 .. 7
    const int32_t* m_of;             // [batch] or nullptr: all have m
    const double* path_terms;        // [batch][PQP_SCORE_STRIDE] or nullptr
    const int32_t* search_flags;     // [batch] or nullptr
    const int32_t* first_hit;        // [batch] or nullptr
    const double* clearance;         // [batch][m] or nullptr
    const double* paths;             // [batch][n][path_stride] or nullptr
    const int32_t* n_of;             // [batch] or nullptr
    const int32_t* group_start;      // [groups + 1]
    double prm[PQP_RANK_PARAMS];
    double* terms;                   // [batch][PQP_PLAN_SCORE_STRIDE]
    int32_t* best;                   // [groups]
    double* best_traj;               // [groups][m][PQP_TRAJ_STRIDE] or nullptr
    int32_t* best_m;                 // [groups] or nullptr
    double* best_paths;              // [groups][n][7] or nullptr
    int32_t* best_n;                 // [groups] or nullptr
};

__global__ void __launch_bounds__(kRankThreads) plan_score_kernel(const RankArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kRankThreads / 64) + (threadIdx.x >> 6)));
    if (b >= a.batch) return;
    const int c = clamped_count(a.m_of, b, a.m);
    double* rec = a.terms + (size_t)b * PQP_PLAN_SCORE_STRIDE;
    if (c < 1) {
        if (lane < PQP_PLAN_SCORE_STRIDE) rec[lane] = 0.0;
        return;
    }
    const double* __restrict__ p = a.traj + (size_t)b * a.m * a.stride;
    const double* __restrict__ cl = a.clearance ? a.clearance + (size_t)b * a.m : nullptr;
    const double want = a.prm[PQP_RANK_CLEARANCE_WANT];
    double s_acc = 0.0, s_jump = 0.0, s_lat = 0.0, s_cl = 0.0, neg_least = -INFINITY;
    bool clear_nan = false;
    for (int f = lane; f < c; f += 64) {
        const double* r = p + (size_t)f * a.stride;
        const double k = r[3], v = r[5], acc = r[6], t = r[7];
        double h = 0.0;
        if (f + 1 < c) {
            const double jump = r[a.stride + 6] - acc, kvv = k * (v * v);
            h = r[a.stride + 7] - t;
            s_acc += (acc * acc) * h;
            s_jump += jump * jump;
            s_lat += (kvv * kvv) * h;
        }
        if (cl) {
            const double d = cl[f], short_of = fmax(0.0, want - d);
            clear_nan = clear_nan || d != d;
            neg_least = fmax(neg_least, -d);
            if (f + 1 < c) s_cl += (short_of * short_of) * h;
        }
    }
    const double t_acc = wave_sum(s_acc), t_jump = wave_sum(s_jump), t_lat = wave_sum(s_lat), t_cl = cl ? wave_sum(s_cl) : 0.0;
    double least = 0.0;
    if (cl) least = __ballot(clear_nan) ? NAN : -wave_max(neg_least);
    const double* last = p + (size_t)(c - 1) * a.stride;
    const double progress = last[4] - p[4], duration = last[7] - p[7];
    const double* pt = a.path_terms ? a.path_terms + (size_t)b * PQP_SCORE_STRIDE : nullptr;
    const double path_score = pt ? pt[0] : 0.0;
    const double score = a.prm[PQP_RANK_W_PATH] * path_score - a.prm[PQP_RANK_W_PROGRESS] * progress + a.prm[PQP_RANK_W_ACCEL] * t_acc +
                         a.prm[PQP_RANK_W_JUMP] * t_jump + a.prm[PQP_RANK_W_LATERAL] * t_lat + a.prm[PQP_RANK_W_CLEARANCE] * t_cl;
    const bool eligible = (!a.search_flags || (a.search_flags[b] & (PQP_SEARCH_NO_PLAN | PQP_SEARCH_EMPTY | PQP_SEARCH_NOT_FINITE)) == 0) &&
                          (!a.first_hit || !a.require_free || a.first_hit[b] == c) && (!pt || pt[7] != 0.0) && isfinite(score);
    // one 80-byte record: lanes 0 .. 9 hold its entries
    const double v = lane == 0 ? score : lane == 1 ? progress : lane == 2 ? t_acc : lane == 3 ? t_jump : lane == 4 ? t_lat : lane == 5 ? least :
                     lane == 6 ? t_cl : lane == 7 ? path_score : lane == 8 ? duration : (eligible ? 1.0 : 0.0);
    if (lane < PQP_PLAN_SCORE_STRIDE) rec[lane] = v;
}

__global__ void __launch_bounds__(kRankThreads) plan_group_kernel(const RankArgs a) {
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kRankThreads / 64) + (threadIdx.x >> 6)));
    if (g >= a.groups) return;
    int lo, hi;
    group_rows(a.group_start, g, a.batch, &lo, &hi);
    const int winner = group_least<PQP_PLAN_SCORE_STRIDE, 9>(a.terms, lo, hi, lane);
    if (lane == 0) a.best[g] = winner;
    if (a.best_traj) {
        const int count = winner >= 0 ? clamped_count(a.m_of, winner, a.m) : 0;
        if (lane == 0) a.best_m[g] = count;
        const double* __restrict__ src = winner >= 0 ? a.traj + (size_t)winner * a.m * a.stride : nullptr;
        double* dst = a.best_traj + (size_t)g * a.m * PQP_TRAJ_STRIDE;
        const long long total = (long long)a.m * PQP_TRAJ_STRIDE;
        for (long long e = lane; e < total; e += 64) {
            const int row = (int)(e / PQP_TRAJ_STRIDE), col = (int)(e - (long long)row * PQP_TRAJ_STRIDE);
            dst[e] = row < count ? src[(size_t)row * a.stride + col] : 0.0;
        }
    }
    if (a.best_paths) {
        const int count = winner >= 0 ? clamped_count(a.n_of, winner, a.n) : 0;
        if (lane == 0) a.best_n[g] = count;
        const double* __restrict__ src = winner >= 0 ? a.paths + (size_t)winner * a.n * a.path_stride : nullptr;
        double* dst = a.best_paths + (size_t)g * a.n * 7;
        const long long total = (long long)a.n * 7;
        for (long long e = lane; e < total; e += 64) {
            const int row = (int)(e / 7), col = (int)(e - (long long)row * 7);
            dst[e] = row < count ? src[(size_t)row * a.path_stride + col] : 0.0;
        }
    }
}

}  // namespace pqp
