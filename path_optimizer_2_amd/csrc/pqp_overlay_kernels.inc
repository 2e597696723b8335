// pqp_overlay_kernels.inc — instantiated by pqp_maps.hip; includes pqp_agent_frames.hpp.  Standing agents laid over the obstacle distance layers
// (pqp_overlay_agents): layer(scene) = min(base layer, distance to the scene's standing agents), so that every reader of a layer - the
// corridor bounds, the DP search, the footprint check - goes round a parked agent as it goes round an obstacle.  The reference has no
// counterpart: it plans against one static map.  include/pqp.h states the definition operation by operation.
//
// The frames are agent_frames_kernel's (pqp_agents_kernels.inc, through launch_agent_frames) with one step per agent: the sincos is taken
// once per agent.
// overlay_kernel: one wavefront per tile of a scene's layer, four per workgroup: 64 consecutive i (the contiguous axis, a cell per lane per
//   column) times kOverlayCols columns j.  Every global access of a wavefront is one contiguous 256 B line, the base layer in and the
//   scene's layer out; the base layers are shared by many scenes and stay in L2.  The scene's frame rows are wave-uniform: the address is
//   built from blockIdx and a readfirstlane alone and every store stands behind the last load, so they come through scalar loads.  The
//   loop over agents is wave-uniform.  No LDS, no scratch, no atomics; ragged edges are lanes that load nothing and store nothing.
//   The broad phase: an agent whose rounded rectangle stays further from every cell centre of the tile than the tile's largest base value
//   (overlay_out_of_reach, whose slack is orders above the rounding of the exact distance) cannot undercut a cell and is left out; a tile
//   with a NaN base value takes no such shortcut.  None of that changes an output.

#include "pqp_agent_frames.hpp"

namespace pqp {

constexpr int kOverlayThreads = 256;
constexpr int kOverlayCols = 8;                                 // columns j of a tile

struct OverlayArgs {
    int n_maps, n_scenes, a_max;
    pqp_grid_geometry g;
    double inflate;
    const float* dist;               // [n_maps][cols][rows]
    const int32_t* a_of;             // [n_scenes] or nullptr: all a_max
    const int32_t* base_of;          // [n_scenes] or nullptr: layer 0 of one, else layer s
    const double* frames;            // [n_scenes][a_max][PQP_AGENT_FRAME_STRIDE]
    float* out;                      // [n_scenes][cols][rows]; may be dist itself where every scene reads its own layer
    int32_t* flags;                  // [n_scenes]
    unsigned tiles_i, tiles_j;       // tiles along i and along j
    unsigned scenes_y;               // gridDim.y: scene = blockIdx.z * scenes_y + blockIdx.y
};

// the broad phase: the agent's rounded rectangle (inside the circle of radius `reach` about (ax, ay)), grown by `inflate`, stays further
// than `most` + the slack from every point within `half_diag` of (tx, ty).  most: the tile's largest base value; with a negative `far`
// no shortcut is taken.
__device__ __forceinline__ bool overlay_out_of_reach(double most, double half_diag, double reach, double inflate, double tx, double ty, double ax,
                                                     double ay) {
#pragma clang fp contract(off)
    const double ux = tx - ax, uy = ty - ay;
    const double far = most + half_diag + reach + inflate + kAgentsSlack + kAgentsSlackRel * (fabs(tx) + fabs(ty) + fabs(ax) + fabs(ay));
    return far >= 0.0 && ux * ux + uy * uy > far * far;
}

__global__ void __launch_bounds__(kOverlayThreads) overlay_kernel(const OverlayArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const unsigned tile = blockIdx.x * (kOverlayThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long s = (long long)blockIdx.z * a.scenes_y + blockIdx.y;
    if (s >= a.n_scenes || tile >= a.tiles_i * a.tiles_j) return;
    const int rows = a.g.rows, cols = a.g.cols;
    const int i = (int)(tile % a.tiles_i) * 64 + lane, i_first = (int)(tile % a.tiles_i) * 64;
    const int j0 = (int)(tile / a.tiles_i) * kOverlayCols;
    const long long base = a.base_of ? min(max(a.base_of[s], 0), a.n_maps - 1) : (a.n_maps == 1 ? 0 : s);
    const size_t cells = (size_t)rows * cols;
    const float* src = a.dist + (size_t)base * cells + (size_t)j0 * rows + i;
    float* dst = a.out + (size_t)s * cells + (size_t)j0 * rows + i;

    float b[kOverlayCols];
    double most = -INFINITY;                                                              // of the loaded base values
    bool nan = false;
    // (the loads first, nothing read of them in between: the columns' lines are in flight together)
#pragma unroll
    for (int q = 0; q < kOverlayCols; ++q) b[q] = i < rows && j0 + q < cols ? src[(size_t)q * rows] : 0.0f;
#pragma unroll
    for (int q = 0; q < kOverlayCols; ++q)
        if (i < rows && j0 + q < cols) { most = fmax(most, (double)b[q]); nan = nan || b[q] != b[q]; }
    most = wave_max(most);
    const bool shortcut = __ballot(nan) == 0;

    // the scene's rows: a bad one is seen before anything is left out
    const int A = clamped_count(a.a_of, s, a.a_max);
    const double* __restrict__ frames = a.frames + (size_t)s * a.a_max * PQP_AGENT_FRAME_STRIDE;
    bool bad = false, some = false;
    for (int ag = 0; ag < A; ++ag) {
        const double reach = frames[(size_t)ag * PQP_AGENT_FRAME_STRIDE + 7];
        if (agent_bad(reach)) bad = true;
        else if (!agent_absent(reach)) some = true;
    }

    double dmin[kOverlayCols];
#pragma unroll
    for (int q = 0; q < kOverlayCols; ++q) dmin[q] = INFINITY;
    if (!bad && some) {
        const double res = a.g.resolution, inflate = a.inflate;
        const double cx = cell_centre(a.g.pos_x, a.g.length_x, res, i);
        double cy[kOverlayCols];
#pragma unroll
        for (int q = 0; q < kOverlayCols; ++q) cy[q] = cell_centre(a.g.pos_y, a.g.length_y, res, j0 + q);
        // the tile's bounding circle: its centre between the first and the last cell centre, whether those cells are in the map or not
        const double tx = 0.5 * (cell_centre(a.g.pos_x, a.g.length_x, res, i_first) + cell_centre(a.g.pos_x, a.g.length_x, res, i_first + 63));
        const double ty = 0.5 * (cy[0] + cy[kOverlayCols - 1]);
        const double half_diag = 0.5 * (res * sqrt(63.0 * 63.0 + (double)((kOverlayCols - 1) * (kOverlayCols - 1))));
        const double* f = frames;
        for (int ag = 0; ag < A; ++ag, f += PQP_AGENT_FRAME_STRIDE) {
            const double ax = f[0], ay = f[1], reach = f[7];                              // wave-uniform
            if (agent_absent(reach)) continue;
            if (shortcut && overlay_out_of_reach(most, half_diag, reach, inflate, tx, ty, ax, ay)) continue;
            const double c = f[2], sn = f[3], hl = f[4], hw = f[5], radius = f[6];
#pragma unroll
            for (int q = 0; q < kOverlayCols; ++q) {
                const double d = agent_point_distance(cx, cy[q], ax, ay, c, sn, hl, hw, radius);
                dmin[q] = fmin(dmin[q], fmax(d - inflate, 0.0));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kOverlayCols; ++q)
        if (i < rows && j0 + q < cols) dst[(size_t)q * rows] = bad ? 0.0f : (dmin[q] < (double)b[q] ? (float)dmin[q] : b[q]);
    if (tile == 0 && lane == 0) a.flags[s] = bad ? PQP_OVERLAY_BAD : (some ? 0 : PQP_OVERLAY_NONE);
}

}  // namespace pqp
