// pqp_select_kernels.inc — instantiated by pqp_select.hip; includes pqp_driven_path.hpp.  Scores of candidate paths and each group's best
// (pqp_select_paths).  The reference plans one path per call and has nothing to rank; the default weights are the path QP's own
//   weight_kappa 20, weight_dkappa 100, weight_l 0          src/solver/base_solver.cpp:123-147 (the diagonal of P)
//   clearance_want 0.6                                       src/config/planning_flags.cpp:95 (FLAGS_expected_safety_margin)
// so the default score is twice that QP's objective without its slack terms.
// path_score_kernel: one wavefront per candidate, four per workgroup, lanes striding over its waypoints; a wavefront's 64 rows are one
// contiguous span of `paths`, lane i also reads row i + 1's x, y for the chord.  Every lane adds its own waypoints in ascending order and
// the 64 partial sums meet in wave_sum, so the order of the additions depends on the candidate's count alone: the same candidate gives the
// same bits wherever it stands in whatever batch.  group_select_kernel: one wavefront per group over the 64-byte records the first kernel
// wrote; its reading of group_start and its choice of the winner are device functions that pqp_rank_kernels.inc uses too.  No atomics, no LDS.

#include "pqp_driven_path.hpp"

namespace pqp {

constexpr int kSelectThreads = 256;

struct SelectArgs {
    int batch, n, stride, groups;
    const double* paths;             // [batch][n][stride]  x, y, heading, l, d_heading, k, dk at offsets 0 .. 6
    const int32_t* n_of;             // [batch] or nullptr: all have n
    const int32_t* status;           // [batch] or nullptr
    const int32_t* stage;            // [batch] or nullptr
    const int32_t* first_collision;  // [batch] or nullptr
    const double* margin;            // [batch][n] or nullptr
    const int32_t* group_start;      // [groups + 1]
    pqp_select_params prm;
    double* terms;                   // [batch][PQP_SCORE_STRIDE]
    int32_t* best;                   // [groups]
    double* best_paths;              // [groups][n][7] or nullptr
    int32_t* best_n;                 // [groups] or nullptr
};

__global__ void __launch_bounds__(kSelectThreads) path_score_kernel(const SelectArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kSelectThreads / 64) + (threadIdx.x >> 6)));
    if (b >= a.batch) return;
    const int count = clamped_count(a.n_of, b, a.n);
    double* rec = a.terms + (size_t)b * PQP_SCORE_STRIDE;
    if (count < 2) {
        if (lane < PQP_SCORE_STRIDE) rec[lane] = 0.0;
        return;
    }
    const double* __restrict__ p = a.paths + (size_t)b * a.n * a.stride;
    const double* __restrict__ mg = a.margin ? a.margin + (size_t)b * a.n : nullptr;
    double s_k = 0.0, s_dk = 0.0, s_l = 0.0, s_len = 0.0, s_cl = 0.0, neg_least = -INFINITY;
    bool margin_nan = false;
    for (int i = lane; i < count; i += 64) {
        const double* r = p + (size_t)i * a.stride;
        const double x = r[0], y = r[1], l = r[3], k = r[5], dk = r[6];
        s_k += k * k;
        s_l += l * l;
        if (i + 1 < count) {
            const double dx = r[a.stride] - x, dy = r[a.stride + 1] - y;
            s_dk += dk * dk;
            s_len += sqrt(dx * dx + dy * dy);
        }
        if (mg) {
            const double m = mg[i], short_of = a.prm.clearance_want - m;
            margin_nan = margin_nan || m != m;
            neg_least = fmax(neg_least, -m);
            s_cl += short_of > 0.0 ? short_of * short_of : (short_of != short_of ? short_of : 0.0);
        }
    }
    double t_k = wave_sum(s_k), t_dk = wave_sum(s_dk), t_l = wave_sum(s_l), t_cl = mg ? wave_sum(s_cl) : 0.0;
    const double t_len = wave_sum(s_len);
    double least = 0.0;
    if (mg) least = __ballot(margin_nan) ? NAN : -wave_max(neg_least);
    if (a.prm.per_waypoint) {
        const double c = (double)count;
        t_k = t_k / c; t_dk = t_dk / c; t_l = t_l / c; t_cl = t_cl / c;
    }
    const double score = a.prm.weight_kappa * t_k + a.prm.weight_dkappa * t_dk + a.prm.weight_offset * t_l + a.prm.weight_length * t_len +
                         a.prm.weight_clearance * t_cl;
    const bool eligible = (!a.status || a.status[b] == PQP_STATUS_SOLVED) && (!a.stage || a.stage[b] == PQP_CHAIN_OK) &&
                          (!a.first_collision || !a.prm.require_free || a.first_collision[b] == count) && isfinite(score);
    // one 64-byte record: lanes 0 .. 7 hold its entries
    const double v = lane == 0 ? score : lane == 1 ? t_k : lane == 2 ? t_dk : lane == 3 ? t_l : lane == 4 ? t_len : lane == 5 ? least :
                     lane == 6 ? t_cl : (eligible ? 1.0 : 0.0);
    if (lane < PQP_SCORE_STRIDE) rec[lane] = v;
}

// What group_select_kernel and plan_group_kernel (pqp_rank_kernels.inc) share: the rows of group g, and the group's winner.
// group_start is the caller's: whatever it holds, the rows read stay inside [0, batch); a descending pair is an empty group
__device__ __forceinline__ void group_rows(const int32_t* group_start, int g, int batch, int* lo, int* hi) {
    *lo = min(max(group_start[g], 0), batch);
    *hi = min(max(group_start[g + 1], 0), batch);
}

// the row in [lo, hi) of the least score (entry 0 of a record of STRIDE doubles) among those whose entry ELIGIBLE is not 0, the lowest row
// among equal scores, -1 when there is none; the same value in every lane.  Called by the whole wavefront
template <int STRIDE, int ELIGIBLE>
__device__ __forceinline__ int group_least(const double* terms, int lo, int hi, int lane) {
    double least = INFINITY;
    int at = INT_MAX;
    for (int b = lo + lane; b < hi; b += 64) {
        const double* rec = terms + (size_t)b * STRIDE;
        const double score = rec[0];
        if (rec[ELIGIBLE] != 0.0 && score < least) { least = score; at = b; }   // ascending b: the lane keeps the lowest index of its least
    }
    const double wave_least = -wave_max(-least);
    const int cand = (at != INT_MAX && least == wave_least) ? at : INT_MAX;
    const int winner_or_max = (int)-wave_max(-(double)cand);                     // an index is exact in a double
    return winner_or_max == INT_MAX ? -1 : winner_or_max;
}

__global__ void __launch_bounds__(kSelectThreads) group_select_kernel(const SelectArgs a) {
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kSelectThreads / 64) + (threadIdx.x >> 6)));
    if (g >= a.groups) return;
    int lo, hi;
    group_rows(a.group_start, g, a.batch, &lo, &hi);
    const int winner = group_least<PQP_SCORE_STRIDE, 7>(a.terms, lo, hi, lane);
    if (lane == 0) a.best[g] = winner;
    if (!a.best_paths) return;
    const int count = winner >= 0 ? clamped_count(a.n_of, winner, a.n) : 0;
    if (lane == 0) a.best_n[g] = count;
    const double* __restrict__ src = winner >= 0 ? a.paths + (size_t)winner * a.n * a.stride : nullptr;
    double* dst = a.best_paths + (size_t)g * a.n * 7;
    const long long total = (long long)a.n * 7;
    for (long long e = lane; e < total; e += 64) {
        const int row = (int)(e / 7), col = (int)(e - (long long)row * 7);
        dst[e] = row < count ? src[(size_t)row * a.stride + col] : 0.0;
    }
}

}  // namespace pqp
