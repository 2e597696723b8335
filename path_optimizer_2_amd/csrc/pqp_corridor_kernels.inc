// pqp_corridor_kernels.inc — included by pqp_lines.hip (SplineView, obstacle_distance ...: pqp_line_device.hpp).  Corridor bounds of every waypoint from the obstacle distance map
// (SURVEY.md §8f rank 1): the step that produces the `bounds` input of the path QP.
//   ReferencePathImpl::updateBoundsImproved            src/data_struct/reference_path_impl.cpp:177-230
//   ReferencePathImpl::getClearanceWithDirectionStrict src/data_struct/reference_path_impl.cpp:232-312
//   Map::getObstacleDistance                           src/tools/Map.cpp:16-22   (grid_map_core isInside + atPosition(INTER_LINEAR))
//   getDirectionalProjectionByNewton                   src/tools/tools.cpp:156-189
//   tk::spline::operator() / deriv                     src/tools/spline.cpp:251-318
// One workgroup per scenario, one lane per (waypoint, circle): circle 0 = front, 1 = rear, 2 = centre.  Every lane walks its
// own ray through the distance map (<= 2 x (20 + 5) bilinear samples of 4 floats, L2-resident map), so the kernel is a
// latency-bound gather; the arithmetic is kept in the reference's operation order with FMA contraction off, so that apart
// from sin/cos (ocml vs libm) every sample position, hence every step count, is the reference's.

namespace pqp {

struct CorridorArgs {
    int batch, n, m;                 // scenarios, waypoints, spline knots
    int tile;                        // waypoints the kernel holds in LDS at a time (n when a whole scenario fits; long paths go through in tiles)
    const double* ref;               // [batch][n][5]  s, k, heading, x, y
    const double* spl;               // [batch][9][m]  knots; y, a, b, c of x(s); y, a, b, c of y(s)
    const double* spl_ext;           // [batch][4]     b0, c0 of x(s); b0, c0 of y(s)   (left extrapolation)
    const float* dist;               // [n_maps][cols][rows]  the "distance" layer, column major like Eigen::MatrixXf
    const int32_t* map_of;           // [batch] map index per scenario, or nullptr: all scenarios use map 0
    pqp_grid_geometry g;
    pqp_corridor_params p;
    const int32_t* n_of;             // [batch] waypoints of each scenario (<= n), or nullptr: all have n
    double* bounds;                  // [batch][n][6]  f_lb f_ub r_lb r_ub c_lb c_ub
    int32_t* n_valid;                // [batch] index of the first blocked waypoint (its own count: none)
};

struct RefStatesArgs {
    int batch, n_max, m;
    const double* spl;               // [batch][9][m]
    const double* spl_ext;           // [batch][4]
    const double* max_s;             // [batch] length of the reference line
    const double* start;             // [batch][3] vehicle start state x, y, heading, or nullptr
    double ds_small, ds_large;
    int dynamic;
    double* ref;                     // [batch][n_max][5]  s, k, heading, x, y
    int32_t* count;                  // [batch] states the loop produces (may exceed n_max: then only n_max rows were written)
    double* init_err;                // [batch][2] initial offset, initial heading error (needs start), or nullptr
    // dynamic == 2: ReferencePathSmoother::segmentRawReference (reference_path_smoother.cpp:48-85): abscissae 0, ds, 2 ds, ... up to
    // and including the first one >= max_s; curvature with pow(., 1.5); outputs as the five lists the smoother QPs take
    double *lx, *ly, *ls, *langle, *lk;          // [batch][n_max] each (only when dynamic == 2)
};

// The long forms of the line-geometry kernels (PQP_OPT_LONG_LINES, pqp.h).  The LDS kernels below stage a line's spline table (9 doubles per
// knot) and their per-element arrays in one CU's LDS, which caps the line they take (DESIGN.md 8.3).  Each of them has a long form (long_*_kernel)
// with what does not fit moved out of the LDS and nothing else changed - the same expressions in the same order, so the same bits:
//   - the spline table is read where it lies, in HBM: the binary search of spline_segment touches ~log2(m) knots per evaluation, its first
//     levels shared by every lane of a wavefront (L1 / L2 hits), and the walks in s move through the table in order;
//   - abscissae and points a kernel writes to its outputs anyway are read back from there instead of from an LDS copy;
//   - the rest (the spline fit's seven sweep arrays, the DP's per-layer arrays and parents, the B-spline's knot vector) goes to a workspace
//     of the handle (pqp_handle::line_ws), one slice per workgroup.
// A kernel and its long form are one source text: a pqp_*_body.inc included into both with PQP_LINE_LONG = 0 / 1 (the corridor pair:
// pqp_corridor_body.inc, which says why an included text), reference_length_body<kLong> for the one pair where a function gives the same code.
// The __global__ functions keep names of their own, the long ones such that no other kernel's name is a substring of theirs:
// tests/test_kernel_resources.py finds kernels by substring.
// Layout of the kernel's dynamic LDS in doubles; n = waypoints held at a time (CorridorArgs::tile), tasks = (waypoint, circle)
struct CorridorLds {
    int m, n;
    __host__ __device__ int spl() const { return 0; }                      // [9][m]   the scenario's spline table
    __host__ __device__ int acc() const { return 9 * m; }                  // [32]     delta_s added j + 1 times (the reference accumulates)
    __host__ __device__ int org() const { return acc() + 32; }             // [3n][8]  probe origin x, y; offset; cos, sin of the left normal; of the right; ok
    __host__ __device__ int cend() const { return org() + 3 * n * 8; }     // [3n][2]  bound after the coarse walk, per side
    __host__ __device__ int first() const { return cend() + 3 * n * 2; }   // int [3n][2]  first failing coarse step, then first failing fine step
    __host__ __device__ size_t total_bytes() const { return (size_t)first() * 8 + (size_t)3 * n * 2 * 4; }
};

// ReferencePathImpl::updateBoundsOnInputStates (src/data_struct/reference_path_impl.cpp:118-175) is the same walk, with the front and rear
// circle centres moved to where the planned heading error d_heading of input state i puts them (states_bounds_kernel below).
//
// One workgroup per scenario.  The reference walks every ray sample by sample (the first sample closer than 0.5 m to an obstacle
// ends the walk); here all candidate samples of all rays of the scenario are gathered in parallel and the first failing one is
// found with an LDS atomicMin: about twice the samples, but one gather latency per round instead of a chain of up to 25.  Every
// sample position is the reference's expression of the same accumulated step lengths, so the result is the walk's.
__global__ void __launch_bounds__(1024) corridor_bounds_kernel(const CorridorArgs a) {
#define PQP_CORRIDOR_ON_STATES 0
#include "pqp_corridor_body.inc"
#undef PQP_CORRIDOR_ON_STATES
}

// states [batch][a.n][stride]: d_heading at offset 4 (a path solve's `out` in place with stride 7); a.n_of: the states of each scenario.
// (named apart from corridor_bounds_kernel: tests/test_kernel_resources.py finds that one by a substring of its name)
__global__ void __launch_bounds__(1024) states_bounds_kernel(const CorridorArgs a, const double* __restrict__ states, int stride) {
#define PQP_CORRIDOR_ON_STATES 1
#include "pqp_corridor_body.inc"
#undef PQP_CORRIDOR_ON_STATES
}

// ... and the two with the table in HBM (PQP_OPT_LONG_LINES): the LDS holds the probes of a tile of waypoints alone
__global__ void __launch_bounds__(1024) long_corridor_kernel(const CorridorArgs a) {
#define PQP_CORRIDOR_ON_STATES 0
#define PQP_CORRIDOR_LONG 1
#include "pqp_corridor_body.inc"
#undef PQP_CORRIDOR_LONG
#undef PQP_CORRIDOR_ON_STATES
}

__global__ void __launch_bounds__(1024) long_states_kernel(const CorridorArgs a, const double* __restrict__ states, int stride) {
#define PQP_CORRIDOR_ON_STATES 1
#define PQP_CORRIDOR_LONG 1
#include "pqp_corridor_body.inc"
#undef PQP_CORRIDOR_LONG
#undef PQP_CORRIDOR_ON_STATES
}

// Reference states from the spline of the reference line + the initial error of the vehicle (SURVEY.md 8f rank 2):
//   ReferencePathImpl::buildReferenceFromSpline  src/data_struct/reference_path_impl.cpp:314-338   (sequential in s: the next
//       step length depends on the curvature just computed -> one lane per scenario walks its own line)
//   PathOptimizer::processInitState              src/path_optimizer.cpp:73-85
// One wavefront per scenario: the spline table is staged in LDS, lane 0 walks s (it only needs the curvature at each step),
// then all lanes evaluate the states of the walk's abscissae in parallel and write them coalesced.
// Long form: the walk's abscissae go straight to their output column (s of a reference state / the `s` list), where the lanes read them back.
__global__ void __launch_bounds__(64) reference_states_kernel(const RefStatesArgs a) {
#define PQP_LINE_LONG 0
#include "pqp_ref_states_body.inc"
#undef PQP_LINE_LONG
}
__global__ void __launch_bounds__(64) long_ref_states_kernel(const RefStatesArgs a) {
#define PQP_LINE_LONG 1
#include "pqp_ref_states_body.inc"
#undef PQP_LINE_LONG
}

// ReferencePathSmoother::bSpline (src/reference_path_smoother/reference_path_smoother.cpp:490-521): the input points are the control
// points of a clamped B-spline (tinyspline::BSpline(n, 2, degree), degree 3 / 4 / 5 by the points' average spacing), sampled at
// t = 0, 1/length, 2/length, ... while t < 1 and at t = 1; s = accumulated chord length.  tinyspline is not part of the reference
// tree: its clamped knot vector and de Boor evaluation are restated from its published behaviour (oracle/corridor_oracle.py says
// what that is and that this parity is unpinned).  One wavefront per scenario: lane 0 walks t (the accumulation is sequential as
// written), all lanes evaluate the samples in parallel, lane 0 accumulates the chord lengths in the reference's order.
struct BsplineArgs {
    int batch, p_max, n_max;
    const double* pts;               // [batch][p_max][2] input points x, y
    const int32_t* n_pts;            // [batch] points of each scenario (4 .. p_max; fewer: count = 0, the reference's "Few reference points")
    double *x, *y, *s;               // [batch][n_max]
    int32_t* count;                  // [batch] samples the loop produces (when it exceeds n_max only n_max were written)
};

template <int DEG>
__device__ __forceinline__ void de_boor(const double* ctrl, const double* knots, int n, double u, double& ox, double& oy) {
#pragma clang fp contract(off)
    int k = DEG;
    while (k + 1 < n && knots[k + 1] <= u) ++k;                // knots[k] <= u < knots[k + 1]
    double dx[DEG + 1], dy[DEG + 1];
#pragma unroll
    for (int j = 0; j <= DEG; ++j) { dx[j] = ctrl[2 * (j + k - DEG)]; dy[j] = ctrl[2 * (j + k - DEG) + 1]; }
#pragma unroll
    for (int r = 1; r <= DEG; ++r) {
#pragma unroll
        for (int j = DEG; j >= r; --j) {
            const int i = j + k - DEG;
            const double a = (u - knots[i]) / (knots[i + DEG - r + 1] - knots[i]);
            dx[j] = (1.0 - a) * dx[j - 1] + a * dx[j];
            dy[j] = (1.0 - a) * dy[j - 1] + a * dy[j];
        }
    }
    ox = dx[DEG]; oy = dy[DEG];
}

// Long form: the points are read from the input, the knot vector is in the workspace (ws = [batch][p_max + 6]), t in the `s` output until the
// chord lengths overwrite it, and the samples are read back from the x / y outputs.
__global__ void __launch_bounds__(64) bspline_resample_kernel(const BsplineArgs a) {
#define PQP_LINE_LONG 0
#include "pqp_bspline_body.inc"
#undef PQP_LINE_LONG
}
__global__ void __launch_bounds__(64) long_bspline_kernel(const BsplineArgs a, double* __restrict__ ws) {
#define PQP_LINE_LONG 1
#include "pqp_bspline_body.inc"
#undef PQP_LINE_LONG
}

// PathOptimizer::setReferencePathLength (src/path_optimizer.cpp:87-104): when the target state lies behind the end of the reference
// line (its x in the end state's frame is <= 0), the line is cut at the target's projection.  One wavefront per scenario (the spline
// table goes through LDS as in the other kernels; the projection's coarse scan runs one sample per lane).
struct RefLengthArgs {
    int batch, m;
    const double* spl;               // [batch][9][m]
    const double* spl_ext;           // [batch][4]
    const double* length;            // [batch] ReferencePath::getLength()
    const double* target;            // [batch][3] target state x, y, heading
    double* length_out;              // [batch]
};

template <bool kLong>
__device__ __forceinline__ void reference_length_body(const RefLengthArgs& a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];          // [9][m]
    const int qp = blockIdx.x;
    const int n = a.m;
    const double* tab = a.spl + (size_t)qp * 9 * n;
    if constexpr (!kLong) {
        for (int k = threadIdx.x; k < 9 * n; k += blockDim.x) lds[k] = tab[k];
        __syncthreads();
        tab = lds;
    }
    const double* ext = a.spl_ext + (size_t)qp * 4;
    const SplineView sx{tab, tab + n, tab + 2 * n, tab + 3 * n, tab + 4 * n, ext[0], ext[1], n};
    const SplineView sy{tab, tab + 5 * n, tab + 6 * n, tab + 7 * n, tab + 8 * n, ext[2], ext[3], n};
    const double L = a.length[qp];
    const double tx = a.target[3 * qp], ty = a.target[3 * qp + 1];
    double ex, dx, ddx, ey, dy, ddy;
    spline_eval3(sx, L, ex, dx, ddx); spline_eval3(sy, L, ey, dy, ddy);
    const double eh = atan2(dy, dx);
    const double local_x = (tx - ex) * cos(eh) + (ty - ey) * sin(eh);          // global2Local(end_ref_state, target).x   tools.cpp:57-64
    const double out = local_x > 0.0 ? L : spline_projection_wave(sx, sy, tx, ty, L);     // (local_x is the same in every lane)
    if (threadIdx.x == 0) a.length_out[qp] = out;
}
__global__ void __launch_bounds__(64) reference_length_kernel(const RefLengthArgs a) { reference_length_body<false>(a); }
__global__ void __launch_bounds__(64) long_ref_length_kernel(const RefLengthArgs a) { reference_length_body<true>(a); }

// The tail of ReferencePathSmoother::postSmooth (src/reference_path_smoother/reference_path_smoother.cpp:559-573): the QP's lateral
// offsets at the layers' abscissae become points x = x_s(s) + l cos(heading + pi/2), y = y_s(s) + l sin(heading + pi/2) with the
// accumulated chord length as their new abscissa - the knots of the final reference line's splines (:574-576, pqp_spline_fit).
// One wavefront per scenario: the lanes evaluate the points, lane 0 accumulates the chord lengths in the reference's order.
struct OffsetsArgs {
    int batch, m_spl, m;
    const double* spl;               // [batch][9][m_spl]
    const double* spl_ext;           // [batch][4]
    const double* at_s;              // [batch][m] abscissae on the line (layers_s_list_)
    const double* l;                 // [batch][m] lateral offsets (QPSolution(i))
    const int32_t* m_of;             // [batch] points of each scenario, or nullptr (all m)
    double *x, *y, *s;               // [batch][m]
};

// Long form: the points are read back from the x / y outputs for the chord lengths.
__global__ void __launch_bounds__(64) offsets_to_points_kernel(const OffsetsArgs a) {
#define PQP_LINE_LONG 0
#include "pqp_offsets_body.inc"
#undef PQP_LINE_LONG
}
__global__ void __launch_bounds__(64) long_offsets_kernel(const OffsetsArgs a) {
#define PQP_LINE_LONG 1
#include "pqp_offsets_body.inc"
#undef PQP_LINE_LONG
}

// Natural cubic spline through (s_i, v_i) - what tk::spline::set_points computes (src/tools/spline.cpp:161-249: behaviour, not text), the
// refit that glues the smoother QPs, the reference states and the path QP together (SURVEY.md 8f rank 3; called at
// tension_smoother.cpp:36-38, reference_path_smoother.cpp:58-59,574-576, reference_path_impl.cpp:349-350).
// Formulation (round 6, written from the textbook moment equations, independent of the reference's band-matrix LU): with h_i = s_{i+1} - s_i,
// d_i = (v_{i+1} - v_i) / h_i and the moments M_i = f''(s_i), M_0 = M_{n-1} = 0 (the reference never calls set_boundary),
//     h_{i-1} M_{i-1} + 2 (h_{i-1} + h_i) M_i + h_i M_{i+1} = 6 (d_i - d_{i-1}),   i = 1 .. n-2,
// solved by the Thomas recurrence (forward: pivot reciprocal, modified super-diagonal and right-hand side; backward: substitution), FMA
// contraction allowed; the table's coefficients of f = a (s - s_i)^3 + b (s - s_i)^2 + c (s - s_i) + v_i follow from the moments:
// b_i = M_i / 2, a_i = (M_{i+1} - M_i) / (6 h_i), c_i = d_i - h_i (2 M_i + M_{i+1}) / 6.  Agreement with the reference's compiled
// tk::spline (oracle/_ref/libref_spline.so): a few ulp of the largest coefficient of a row (tests/test_gpu_corridor.py).
// The recurrence is a chain in the knot index, so one wavefront fits one coordinate of one scenario: the lanes stage knots and values in
// LDS, compute h, d and the right-hand sides in parallel and write the coefficient rows back coalesced; lane 0 runs the two sweeps.
struct SplineFitArgs {
    int batch, m;
    const int32_t* m_of;             // [batch] knots of each scenario (3 .. m; m is then the array stride) or nullptr: all have m
    const double* s;                 // [batch][m] knots
    const double* vx;                // [batch][m] x values
    const double* vy;                // [batch][m] y values
    double* spl;                     // [batch][9][m]
    double* spl_ext;                 // [batch][4]
};

// Long form: the seven arrays of a (scenario, coordinate) are its slice of the workspace (ws = [2 batch][7][m]); the two sweeps stream through it.
__global__ void __launch_bounds__(64) spline_fit_kernel(const SplineFitArgs a) {
#define PQP_LINE_LONG 0
#include "pqp_spline_fit_body.inc"
#undef PQP_LINE_LONG
}
__global__ void __launch_bounds__(64) long_fit_kernel(const SplineFitArgs a, double* __restrict__ ws) {
#define PQP_LINE_LONG 1
#include "pqp_spline_fit_body.inc"
#undef PQP_LINE_LONG
}

// Layered DP corridor search between the smoother QP and the postSmooth QP (SURVEY.md 8f rank 4):
//   ReferencePathSmoother::graphSearchDp    src/reference_path_smoother/reference_path_smoother.cpp:142-295
//   ReferencePathSmoother::calculateCostAt  :107-140        getProjection / getProjectionByNewton  src/tools/tools.cpp:66-126
// One workgroup of four wavefronts per scenario.  Layers are sequential (the cost of a node needs the costs of the previous layer).
// Within a layer the lanes of the first wavefront are the lateral samples (34 with the default +-10 m / 0.6 m): each samples the
// distance map and decides feasibility; then ALL 256 lanes evaluate the (node, predecessor) edges - 34 x 34 atan2-heavy costs, the
// kernel's whole arithmetic, 4-5 per lane instead of 34 in a row - into LDS, and the node lanes pick their cheapest predecessor
// (first one on ties, as the reference's strict `<` scan does).  Parents are kept per (layer, lane); lane 0 walks them back, then
// the lanes refine the bounds of the chosen node of every layer in parallel (0.2 m steps along the normal, as the reference does).
struct DpArgs {
    int batch, m, max_layers;
    const double* spl;               // [batch][9][m]
    const double* spl_ext;           // [batch][4]
    const double* length;            // [batch] reference->getLength()
    const double* start;             // [batch][3] start_state_ x, y, heading
    const float* dist;
    const int32_t* map_of;
    pqp_grid_geometry g;
    pqp_dp_params p;
    double* layers_s;                // [batch][max_layers]
    double* lb;                      // [batch][max_layers]
    double* ub;                      // [batch][max_layers]
    int32_t* count;                  // [batch] layers of the corridor; 0: graphSearchDp returns false / nothing reachable; -1: more than max_layers
    double* vehicle_l;               // [batch] vehicle_l_wrt_smoothed_ref_
};

constexpr int kDpChunk = 32;        // layers whose nodes are prepared at once (bounds the LDS table whatever max_layers is)
// The kernel's arrays in the order they lie in, offsets in doubles.  The LDS kernel has them all in its dynamic LDS, DpBlock<true, true>.
// The long form splits that block in two, each in the same order: the arrays that grow with the layers (`per`) in the scenario's slice of
// the workspace, DpBlock<true, false>, the others (`fix`: the two node rows, the lateral offsets, the per-chunk cost tables) in the LDS,
// DpBlock<false, true>, whatever the line's length; the table, which only the one block holds, stays in HBM.
template <bool kPer, bool kFix> struct DpBlock {
    int m, lmax, nlat;
    using Off = std::conditional_t<kFix, int, size_t>;         // offsets in the LDS: 32 bits; in the workspace: 64
    __host__ __device__ Off per(Off len) const { return kPer ? len : 0; }
    __host__ __device__ Off fix(Off len) const { return kFix ? len : 0; }
    __host__ __device__ Off spl() const { return 0; }                          // [9][m]
    __host__ __device__ Off s_layer() const { return kPer && kFix ? 9 * m : 0; }       // per [lmax]
    __host__ __device__ Off node() const { return s_layer() + per(lmax); }     // fix [2][64][2]  dir, cost of the previous / current layer's nodes
    __host__ __device__ Off misc() const { return node() + fix(2 * 64 * 2); }  // fix [8]
    __host__ __device__ Off mask() const { return misc() + fix(8); }           // per unsigned long long [lmax]  feasibility of a layer's nodes
    __host__ __device__ Off ltab() const { return mask() + per(lmax); }        // fix [64] lateral offset of sample j
    __host__ __device__ Off lay() const { return ltab() + fix(64); }           // per [lmax][8]  rx, ry, rh, cos, sin of the normal, rk, 1/rk of a layer
    __host__ __device__ Off self() const { return lay() + per(8 * (Off)lmax); }     // fix [kDpChunk + 1][nlat] own cost of a node (< 0: infeasible), ring of layers
    __host__ __device__ Off edge() const { return self() + fix((kDpChunk + 1) * nlat); }   // fix [nlat][nlat] cost of reaching node j through predecessor jp
    __host__ __device__ Off edir() const { return edge() + fix(nlat * nlat); } // fix [nlat][nlat] direction of that edge (the node phase takes its parent's from here instead of a second atan2)
    __host__ __device__ Off parent() const { return edir() + fix(nlat * nlat); }       // per unsigned char [lmax][nlat] (255: none)
    __host__ __device__ size_t parent_bytes() const { return kPer ? (((size_t)lmax * nlat + 7) / 8) * 8 : 0; }
    __host__ __device__ Off path() const { return parent() + (Off)(parent_bytes() / 8); }  // per int [lmax]
    __host__ __device__ size_t total_bytes() const { return (size_t)parent() * 8 + parent_bytes() + (size_t)per(lmax) * 4; }
    __host__ __device__ size_t doubles() const { return path() + ((size_t)per(lmax) + 1) / 2; }    // a scenario's slice of the workspace
};
constexpr int kDpThreads = 256;
// lateral samples per layer: -range, -range + spacing, ... while <= range, as the reference accumulates them (at most 64)
__host__ __device__ inline int dp_lateral_samples(double range, double spacing) {
    int nlat = 0;
    double c = -range;
    while (c <= range && nlat < 64) { c += spacing; nlat += 1; }
    return nlat;
}

__device__ __forceinline__ double dp_dist(const float* __restrict__ dist, const pqp_grid_geometry& g, double x, double y) {
#pragma clang fp contract(off)
    const double tx = -(x - g.pos_x - 0.5 * g.length_x), ty = -(y - g.pos_y - 0.5 * g.length_y);
    const bool inside = tx >= 0.0 && ty >= 0.0 && tx < g.length_x && ty < g.length_y;
    return inside ? obstacle_distance(dist, g, x, y) : -1.0;                   // isInside ? getObstacleDistance : -1   (:191)
}

// Long form: ws = [batch][DpBlock<true, false>::doubles()].
__global__ void __launch_bounds__(kDpThreads) dp_corridor_kernel(const DpArgs a) {
#define PQP_LINE_LONG 0
#include "pqp_dp_body.inc"
#undef PQP_LINE_LONG
}
__global__ void __launch_bounds__(kDpThreads) long_dp_kernel(const DpArgs a, double* __restrict__ ws) {
#define PQP_LINE_LONG 1
#include "pqp_dp_body.inc"
#undef PQP_LINE_LONG
}

}  // namespace pqp
