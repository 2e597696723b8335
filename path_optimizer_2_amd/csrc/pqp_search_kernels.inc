// pqp_search_kernels.inc — instantiated by pqp_speed.hip; includes pqp_car_circles.hpp and pqp_agent_frames.hpp.  Speeds past predicted agents (pqp_speed_search): the
// occupancy of every path's path-time plane, station against layer, by the footprint test of pqp_agents_check, and a layered dynamic
// program through its free cells.  The reference has no counterpart.  include/pqp.h states the definition operation by operation.
//
// agent_frames_kernel (pqp_agents_kernels.inc, through launch_agent_frames) runs first, as it is.
// st_occupancy_kernel: one wavefront per (path, tile of 64 stations), four per workgroup, one station per lane, no LDS, no atomics.
//   1  tiles of 64 waypoints: every value below the driven count is judged (row_not_finite of pqp_driven_path.hpp, and v_start), and the
//      maximum of the s column is M_{c-1}
//   2  the lanes' segments, by the walk pqp_sample_trajectory takes (walk_tile), here on the s column and from tile 0; then the pose on
//      the chord (chord_pose), its sincos once, the six centres in registers (local_to_global), and qenv_j, which goes as a byte into
//      layer 0 of `parents` - the search has no parents at layer 0 - because the search kernel's LDS is full
//   3  the loops over layers and agents are wave-uniform: a frame row's address is the same for the whole wavefront.  A layer's 64 answers
//      are one ballot, stored as two words by lane 0.  An agent is left out by pqp_agents_check's broad phase (agent_out_of_reach),
//      which changes no output.
// st_search_kernel: one workgroup of 256 per path, the two cost layers [S][Q + 1] ping-pong in 64 KiB of LDS, one barrier per layer.
//   qref_j, a byte per station, goes behind qenv into layer 0 of `parents`.  A lane runs over the states (j, q) of a layer and pulls from
//   (j - q, q'); the swept range test is a mask over at most three words of `blocked`.  Every lane keeps the best state, by the terminal rule, of the last layer in which one of its own states lived: the
//   last living layer and its cheapest state are then one reduction behind the loop (wave_max, and one LDS step across the wavefronts in
//   a cost layer that is free by then), whatever the ping-pong has overwritten.  One lane walks back through the parents, then the
//   wavefronts place the planned stations on the path as step 2 does and a lane per layer writes its traj row.

#include "pqp_car_circles.hpp"
#include "pqp_agent_frames.hpp"

namespace pqp {

constexpr int kSearchThreads = 256;
constexpr int kSearchStates = PQP_SEARCH_MAX_STATES;

struct SearchArgs {
    int batch, n, stride, m, n_scenes, a_max;
    const double* paths;             // [batch][n][stride]  x, y, heading at 0, 1, 2 and k at 5
    const int32_t* n_of;             // [batch] or nullptr
    const int32_t* stop_before;      // [batch] or nullptr
    const double* profile;           // [batch][n][PQP_SPEED_STRIDE]
    const double* v_start;           // [batch]
    const int32_t* a_of;             // [n_scenes] or nullptr
    const int32_t* scene_of;         // [batch] or nullptr
    pqp_search_params prm;
    CarCircles car;
    const double* frames;            // [n_scenes][a_max][m][PQP_AGENT_FRAME_STRIDE]
    int32_t* blocked;                // [batch][m][W]
    uint8_t* parents;                // [batch][m][S][Q + 1]
    int32_t* steps;                  // [batch][m][2]
    double* traj;                    // [batch][m][PQP_TRAJ_STRIDE]
    double* cost;                    // [batch]
    int32_t* reached;                // [batch]
    int32_t* flags;                  // [batch]
};

// step 1, by a whole wavefront: whether a value read below the driven count is not what it must be, and M_{c-1}
__device__ __forceinline__ bool st_judge(const SearchArgs& a, long long b, int c, int lane, double* m_last) {
    const double* __restrict__ p = a.paths + (size_t)b * a.n * a.stride;
    const double* __restrict__ prof = a.profile + (size_t)b * a.n * PQP_SPEED_STRIDE;
    const double v0 = a.v_start[b];
    bool bad = !(v0 >= 0.0 && v0 < INFINITY);
    double top = -INFINITY;
    for (int w = 0; w * 64 < c; ++w) {
        const int i = w * 64 + lane;
        double s = -INFINITY;
        if (i < c) {
            const double* r = p + (size_t)i * a.stride;
            const double* o = prof + (size_t)i * PQP_SPEED_STRIDE;
            s = o[0];
            bad = bad || row_not_finite(r, o);
        }
        top = fmax(top, wave_max(s));
    }
    *m_last = top;
    return __ballot(bad) != 0;
}

// #{ i' < c : M_i' <= sigma } for the sigma of every lane, by a whole wavefront (lanes with nothing to place pass -inf): the s column
// walked from tile 0 until a tile ends above every lane's sigma
__device__ __forceinline__ int st_count(const double* __restrict__ prof, int c, double sigma, int lane) {
    const double sigma_hi = wave_max(sigma);
    int cnt = 0;
    double carry = -INFINITY;
    for (int w = 0; w * 64 < c; ++w) {
        cnt += walk_tile(prof, 0, c, w, carry, sigma, lane, &carry);
        if (!(carry <= sigma_hi)) break;
    }
    return cnt;
}

// the pose at sigma, cnt waypoints at or in front of it, and *w, the envelope's v^2 there
__device__ __forceinline__ PathPose st_pose(const double* __restrict__ p, const double* __restrict__ prof, int stride, int c, int cnt, double sigma,
                                            double* w) {
#pragma clang fp contract(off)
    const int i = max(cnt - 1, 0);
    if (i < c - 1) {
        const double* o0 = prof + (size_t)i * PQP_SPEED_STRIDE;
        const double s0 = o0[0], v0 = o0[1], a0 = o0[2];
        double e;
        const PathPose o = chord_pose(p + (size_t)i * stride, stride, sigma - s0, &e);
        *w = v0 * v0 + (2.0 * a0) * e;
        return o;
    }
    const double v = prof[(size_t)(c - 1) * PQP_SPEED_STRIDE + 1];
    *w = v * v;
    return waypoint_pose(p + (size_t)(c - 1) * stride);
}

__global__ void __launch_bounds__(kAgentsThreads) st_occupancy_kernel(const SearchArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int S = a.prm.stations, Q1 = a.prm.q_max + 1, W = (S + 31) / 32, tiles = (S + 63) / 64;
    const long long wave = (long long)blockIdx.x * (kAgentsThreads / 64) + (threadIdx.x >> 6);
    const long long b = __builtin_amdgcn_readfirstlane((int)(wave / tiles));
    const int tile = __builtin_amdgcn_readfirstlane((int)(wave % tiles));
    if (b >= a.batch) return;
    const int c = driven_count(clamped_count(a.n_of, b, a.n), a.stop_before, b);
    int32_t* __restrict__ blk = a.blocked + (size_t)b * a.m * W + 2 * tile;               // this tile's word pair of layer 0
    const bool second = 2 * tile + 1 < W;
    double m_last = -INFINITY;
    if (c == 0 || st_judge(a, b, c, lane, &m_last)) {
        for (int k = lane; k < a.m; k += 64) {
            blk[(size_t)k * W] = 0;
            if (second) blk[(size_t)k * W + 1] = 0;
        }
        return;
    }
    const double* __restrict__ p = a.paths + (size_t)b * a.n * a.stride;
    const double* __restrict__ prof = a.profile + (size_t)b * a.n * PQP_SPEED_STRIDE;
    const int j = tile * 64 + lane;
    const double sigma = (double)j * a.prm.ds;
    const bool on = j < S && sigma <= m_last;
    const int cnt = st_count(prof, c, on ? sigma : -INFINITY, lane);
    bool always = false;                                     // a pose that is not finite: blocked at every layer
    double gx[6], gy[6];
    Point2 bc = {0.0, 0.0};                                  // the bounding circle's centre
    if (on) {
        double w;
        const PathPose o = st_pose(p, prof, a.stride, c, cnt, sigma, &w);
        const double venv = sqrt(fmax(w, 0.0));
        a.parents[(size_t)b * a.m * S * Q1 + j] = (uint8_t)(int)fmin(floor(venv * a.prm.dt / a.prm.ds), (double)a.prm.q_max);
        always = !(isfinite(o.x) && isfinite(o.y) && isfinite(o.heading));
        double sh, ch;
        sincos(always ? 0.0 : o.heading, &sh, &ch);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const Point2 g = local_to_global(a.car.cx[q], a.car.cy[q], sh, ch, o.x, o.y);
            gx[q] = g.x; gy[q] = g.y;
        }
        bc = local_to_global(a.car.cx[6], a.car.cy[6], sh, ch, o.x, o.y);
    } else {
#pragma unroll
        for (int q = 0; q < 6; ++q) gx[q] = gy[q] = 0.0;
    }
    int A;
    const double* __restrict__ frames = scene_frames(a, b, &A);
    const double margin = a.prm.margin;
    for (int k = 0; k < a.m; ++k) {
        bool hit = always;
        const double* f = frames + (size_t)k * PQP_AGENT_FRAME_STRIDE;
        for (int ag = 0; ag < A; ++ag, f += (size_t)a.m * PQP_AGENT_FRAME_STRIDE) {
            const double ax = f[0], ay = f[1], reach = f[7];                              // wave-uniform
            if (agent_absent(reach)) continue;
            if (agent_bad(reach)) { hit = true; continue; }                               // every station of the layer
            if (!on || hit) continue;
            if (agent_out_of_reach(a.car.rb, reach, margin, bc.x, bc.y, ax, ay)) continue;
            if (agent_clear(gx, gy, a.car.cr, ax, ay, f[2], f[3], f[4], f[5], f[6]) < margin) hit = true;
        }
        const uint64_t bits = __ballot(hit && on);
        if (lane == 0) {
            blk[(size_t)k * W] = (int32_t)(uint32_t)bits;
            if (second) blk[(size_t)k * W + 1] = (int32_t)(uint32_t)(bits >> 32);
        }
    }
}

// whether a station of lo .. hi (hi - lo <= 63) is blocked in one layer's words
__device__ __forceinline__ bool st_swept(const int32_t* __restrict__ row, int lo, int hi) {
    const int w0 = lo >> 5, w1 = hi >> 5;
    uint32_t any = 0;
    for (int w = w0; w <= w1; ++w) {
        uint32_t mask = 0xffffffffu;
        if (w == w0) mask &= 0xffffffffu << (lo & 31);
        if (w == w1) mask &= 0xffffffffu >> (31 - (hi & 31));
        any |= (uint32_t)row[w] & mask;
    }
    return any != 0;
}

// the terminal rule: the cheaper state, then the larger j, then the smaller q
__device__ __forceinline__ bool st_better(double cost, int j, int q, double than_cost, int than_j, int than_q) {
    return cost < than_cost || (cost == than_cost && (j > than_j || (j == than_j && q < than_q)));
}

__global__ void __launch_bounds__(kSearchThreads) st_search_kernel(const SearchArgs a) {
#pragma clang fp contract(off)
    __shared__ double layer[2][kSearchStates];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long b = blockIdx.x;
    const int S = a.prm.stations, Q = a.prm.q_max, Q1 = Q + 1, W = (S + 31) / 32, states = S * Q1, m = a.m;
    const int c = driven_count(clamped_count(a.n_of, b, a.n), a.stop_before, b);
    double m_last = -INFINITY;
    const bool bad = c > 0 && st_judge(a, b, c, lane, &m_last);                            // every wavefront for itself: nothing to share
    if (c == 0 || bad) {
        int32_t* __restrict__ steps = a.steps + (size_t)b * m * 2;
        double* __restrict__ traj = a.traj + (size_t)b * m * PQP_TRAJ_STRIDE;
        const double fill = bad ? NAN : 0.0;
        for (long long e = tid; e < (long long)m * PQP_TRAJ_STRIDE; e += kSearchThreads) traj[e] = fill;
        for (int e = tid; e < 2 * m; e += kSearchThreads) steps[e] = -1;
        if (tid == 0) { a.cost[b] = bad ? NAN : INFINITY; a.reached[b] = 0; a.flags[b] = bad ? PQP_SEARCH_NOT_FINITE : PQP_SEARCH_EMPTY; }
        return;
    }
    double ds = a.prm.ds, dt = a.prm.dt, w_slow = a.prm.w_slow, w_accel = a.prm.w_accel;
    // kept in vector registers, of which this kernel has plenty: as scalars they are carried through the layers and two of them spill
    asm volatile("" : "+v"(ds), "+v"(dt), "+v"(w_slow), "+v"(w_accel));
    const int q_up = min(a.prm.q_up, 64), q_down = min(a.prm.q_down, 64);                 // beyond Q they change nothing
    int J = 0;                                               // #{ j < S : sigma_j <= M_{c-1} }: sigma ascends
    for (int lo = 0, hi = S; ; ) {
        if (lo == hi) { J = lo; break; }
        const int mid = (lo + hi) >> 1;
        if ((double)mid * ds <= m_last) lo = mid + 1; else hi = mid;
    }
    const bool grid_short = m_last > (double)(S - 1) * ds;
    const int32_t* __restrict__ blk = a.blocked + (size_t)b * m * W;
    uint8_t* __restrict__ par = a.parents + (size_t)b * m * S * Q1;
    const uint8_t* qenv = par;                               // layer 0 of the parents: st_occupancy_kernel's qenv_j
    uint8_t* qref = par + (Q > 0 ? S : 0);                   // behind it, where Q >= 1 leaves room: qref_j (Q = 0: every qref is 0, as qenv is)
    const int q0 = (int)fmin(fmax(rint(a.v_start[b] * dt / ds), 0.0), (double)Q);
    const bool start = J > 0 && !(blk[0] & 1);
    if (Q > 0)
        for (int j = tid; j < J; j += kSearchThreads) {
            const int here = qenv[j];
            int top = 0;
            for (int r = 1; r <= min(Q, J - 1 - j); ++r) top = max(top, min(r, max(here, (int)qenv[j + r])));
            qref[j] = (uint8_t)top;
        }

    // ---- the layers ------------------------------------------------------------------------------------------------------------------------
    for (int e = tid; e < states; e += kSearchThreads) {
        layer[0][e] = (start && e == q0) ? 0.0 : INFINITY;
        layer[1][e] = INFINITY;
    }
    // No living state of layer k has a step above q_hi or a station above j_hi - the start's, grown by q_up a layer.  The states beyond
    // are not visited: both cost layers start at +inf, the bounds only grow, so what is skipped now was never written.
    int q_hi = q0, j_hi = 0;
    int my_k = -1, my_j = 0, my_q = 0;                       // the best of this lane's own states in the last layer where one lived
    double my_cost = INFINITY;
    if (start && tid == (q0 & (kSearchThreads - 1))) { my_k = 0; my_q = q0; my_cost = 0.0; }
    __syncthreads();
    for (int k = 1; k < m; ++k) {
        const double* __restrict__ prev = layer[(k - 1) & 1];
        double* __restrict__ cur = layer[k & 1];
        const int32_t* row0 = blk + (size_t)(k - 1) * W;
        const int32_t* row1 = row0 + W;
        uint8_t* pk = par + (size_t)k * states;
        q_hi = min(Q, q_hi + q_up);
        j_hi = min(J - 1, j_hi + q_hi);
        const int visited = (j_hi + 1) * Q1;
        for (int e = tid; e < visited; e += kSearchThreads) {
            const int j = e / Q1, q = e - j * Q1, jp = j - q;
            double best = INFINITY;
            int from = 255;
            if (q <= q_hi && jp >= 0) {
                const int qe = max((int)qenv[jp], (int)qenv[j]);
                if (q <= qe && !st_swept(row0, jp, j) && !st_swept(row1, jp, j)) {
                    const double slow = w_slow * (double)((int)qref[jp] - q);                         // q <= qe gives q <= qref_j'
                    const double* from_row = prev + jp * Q1;
                    for (int qp = max(q - q_up, 0); qp <= min(q + q_down, Q); ++qp) {
                        const double cp = from_row[qp];
                        if (!(cp < INFINITY)) continue;
                        const int dq = q - qp;
                        const double cand = cp + (w_accel * (double)(dq * dq) + slow);
                        if (cand < best) { best = cand; from = qp; }
                    }
                    if (!(best < INFINITY)) from = 255;
                }
            }
            cur[e] = best;
            pk[e] = (uint8_t)from;
            if (best < INFINITY && (k > my_k || st_better(best, j, q, my_cost, my_j, my_q))) { my_k = k; my_cost = best; my_j = j; my_q = q; }
        }
        __syncthreads();
    }

    // ---- the last living layer and its cheapest state: within the wavefront, then across them in layer 0's LDS -------------------------------
    const int k_wave = (int)wave_max((double)my_k);
    const double cost_wave = -wave_max(my_k == k_wave ? -my_cost : -INFINITY);
    const bool in_cost = my_k == k_wave && my_cost == cost_wave;
    const int j_wave = (int)wave_max(in_cost ? (double)my_j : -1.0);
    const int q_wave = -(int)wave_max(in_cost && my_j == j_wave ? -(double)my_q : -INFINITY);
    double* share = layer[0];                                // free: the loop ended on a barrier
    if (lane == 0) { share[4 * wv] = (double)k_wave; share[4 * wv + 1] = cost_wave; share[4 * wv + 2] = (double)j_wave; share[4 * wv + 3] = (double)q_wave; }
    __syncthreads();
    int k_end = -1, j_end = 0, q_end = 0;
    double cost_end = INFINITY;
    for (int w = 0; w < kSearchThreads / 64; ++w) {
        const int kw = (int)share[4 * w], jw = (int)share[4 * w + 2], qw = (int)share[4 * w + 3];
        const double cw = share[4 * w + 1];
        if (kw >= 0 && (kw > k_end || (kw == k_end && st_better(cw, jw, qw, cost_end, j_end, q_end)))) { k_end = kw; cost_end = cw; j_end = jw; q_end = qw; }
    }
    const int reached = k_end + 1;

    // ---- back through the parents, one lane -----------------------------------------------------------------------------------------------
    int32_t* steps = a.steps + (size_t)b * m * 2;            // (addresses taken here, not in front of the loop: they would be carried through it)
    double* __restrict__ traj = a.traj + (size_t)b * m * PQP_TRAJ_STRIDE;
    if (tid == 0) {
        int j = j_end, q = q_end;
        for (int k = k_end; k >= 0; --k) {
            steps[2 * k] = j; steps[2 * k + 1] = q;
            if (k > 0) {
                const int from = par[(size_t)k * states + j * Q1 + q];
                j -= q; q = from;
            }
        }
        a.cost[b] = cost_end;
        a.reached[b] = reached;
        a.flags[b] = (reached < m ? PQP_SEARCH_NO_PLAN : 0) | (reached == 0 ? PQP_SEARCH_START_BLOCKED : 0) | (grid_short ? PQP_SEARCH_GRID_SHORT : 0) |
                     (reached > 0 && j_end == J - 1 && !grid_short ? PQP_SEARCH_ARRIVED : 0);
    }
    __syncthreads();

    // ---- the rows: a lane per layer ---------------------------------------------------------------------------------------------------------
    const double* __restrict__ p = a.paths + (size_t)b * a.n * a.stride;
    const double* __restrict__ prof = a.profile + (size_t)b * a.n * PQP_SPEED_STRIDE;
    for (int k0 = wv * 64; k0 < m; k0 += kSearchThreads) {
        const int k = k0 + lane;
        const bool planned = k < reached;
        const int j = planned ? steps[2 * k] : 0, q = planned ? steps[2 * k + 1] : 0;
        const int q_next = (planned && k + 1 < reached) ? steps[2 * k + 3] : q;
        const double sigma = (double)j * ds;
        const int cnt = st_count(prof, c, planned ? sigma : -INFINITY, lane);
        double row[PQP_TRAJ_STRIDE] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (planned) {
            double w;                                        // (the envelope is not asked for here)
            const PathPose o = st_pose(p, prof, a.stride, c, cnt, sigma, &w);
            row[0] = o.x; row[1] = o.y; row[2] = o.heading; row[3] = o.k; row[4] = sigma;
            row[5] = (double)q * ds / dt;
            row[6] = (double)(q_next - q) * ds / (dt * dt);
            row[7] = (double)k * dt;
        }
        if (k < m) {
            double* o = traj + (size_t)k * PQP_TRAJ_STRIDE;
#pragma unroll
            for (int t = 0; t < PQP_TRAJ_STRIDE; ++t) o[t] = row[t];
            if (!planned) { steps[2 * k] = -1; steps[2 * k + 1] = -1; }
        }
    }
}

}  // namespace pqp
