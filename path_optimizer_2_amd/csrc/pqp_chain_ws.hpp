// pqp_chain_ws.hpp — the device workspace of pqp_optimize_path_device (pqp_chain.hip): doubles and int32 carved out of two buffers.
// Host only and free of HIP, so that a plain C++ program can check the layout (tests/cpp/chain_ws_check.cpp).
//
// PQP_CHAIN_WS_ARRAYS is the one description of the arrays: element type, name, elements per scenario in terms of the capacities
// R (raw_max), S (sample_max), L (layer_max), N (n_max), and whether the array exists only with second_pass = BOUNDS_ON_STATES.  The struct's
// members, the pointers and the byte counts all come from it: an array added here is sized and placed, nothing else has to follow.
// Arrays lie in the order of the list, the doubles in one buffer and the ints in the other, [batch][elements] each; those of the second
// pass come last, so they lie behind the plain chain's in both buffers and the plain chain's layout does not depend on them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#ifndef PQP_HIDDEN
#define PQP_HIDDEN __attribute__((visibility("hidden")))      // (as pqp_internal.hpp: nothing behind the C ABI is exported)
#endif
namespace pqp_internal PQP_HIDDEN {

#define PQP_CHAIN_WS_ARRAYS(X)                                                                                                    \
    /* raw line: bSpline points, spline table, extent, length */                                                                  \
    X(double, rx, R, 0) X(double, ry, R, 0) X(double, rs, R, 0) X(double, raw_tab, 9 * R, 0) X(double, raw_ext, 4, 0) X(double, raw_len, 1, 0) \
    /* its 1 m samples (x, y, s, angle, k), their clearance */                                                                    \
    X(double, gx, S, 0) X(double, gy, S, 0) X(double, gs, S, 0) X(double, ga, S, 0) X(double, gk, S, 0) X(double, clr, S, 0)      \
    /* smoothed line */                                                                                                           \
    X(double, sx, S, 0) X(double, sy, S, 0) X(double, ss, S, 0) X(double, sm_tab, 9 * S, 0) X(double, sm_ext, 4, 0) X(double, sm_len, 1, 0) \
    /* DP corridor: layers, bounds, the vehicle's offset, postSmooth's offsets */                                                 \
    X(double, ls, L, 0) X(double, lb, L, 0) X(double, ub, L, 0) X(double, vl, 1, 0) X(double, pl, L, 0)                           \
    /* final reference line */                                                                                                    \
    X(double, px, L, 0) X(double, py, L, 0) X(double, ps, L, 0) X(double, fin_tab, 9 * L, 0) X(double, fin_ext, 4, 0) X(double, fin_len, 1, 0) \
    X(double, max_s, 1, 0)                                                                                                        \
    /* the path QP's inputs */                                                                                                    \
    X(double, ref, 5 * N, 0) X(double, err, 2, 0) X(double, bounds, 6 * N, 0) X(double, scal, 6, 0)                               \
    /* counts and statuses of the steps (*_fit: the count clamped into the next step's capacity) */                               \
    X(int32_t, raw_count, 1, 0) X(int32_t, raw_fit, 1, 0) X(int32_t, sample_count, 1, 0) X(int32_t, sample_fit, 1, 0)             \
    X(int32_t, sm_status, 1, 0) X(int32_t, sm_iters, 1, 0) X(int32_t, layer_count, 1, 0) X(int32_t, layer_fit, 1, 0)              \
    X(int32_t, ps_status, 1, 0) X(int32_t, ps_iters, 1, 0) X(int32_t, ref_count, 1, 0) X(int32_t, ref_fit, 1, 0)                  \
    X(int32_t, n_valid, 1, 0) X(int32_t, qp_status, 1, 0)                                                                         \
    /* second_pass = BOUNDS_ON_STATES only */                                                                                     \
    X(double, lin, 3 * N, 1)                                                                                                      \
    X(int32_t, n_valid2, 1, 1) X(int32_t, n_of2, 1, 1) X(int32_t, qp_status2, 1, 1) X(int32_t, iters1, 1, 1) X(int32_t, iters2, 1, 1) \
    X(int32_t, n_valid_out, 1, 1) X(int32_t, status_out, 1, 1)

struct ChainDims { int R, S, L, N; bool second; };

struct ChainWs {
#define PQP_CHAIN_WS_MEMBER(type, name, per, second_only) type* name = nullptr;
    PQP_CHAIN_WS_ARRAYS(PQP_CHAIN_WS_MEMBER)
#undef PQP_CHAIN_WS_MEMBER
};

// visit(name, pointer member, elements per scenario) for every array that exists with these dimensions, in layout order
template <class V> void chain_ws_arrays(ChainWs& w, const ChainDims& c, V&& visit) {
    const size_t R = (size_t)c.R, S = (size_t)c.S, L = (size_t)c.L, N = (size_t)c.N;
#define PQP_CHAIN_WS_VISIT(type, name, per, second_only) if (!(second_only) || c.second) visit(#name, w.name, (size_t)(per));
    PQP_CHAIN_WS_ARRAYS(PQP_CHAIN_WS_VISIT)
#undef PQP_CHAIN_WS_VISIT
}

// The arrays of `batch` scenarios placed into the two buffers; returns the elements they take of each.  With null buffers it only
// measures (every pointer stays null): the caller sizes the buffers by that and carves again.
struct ChainWsSize { size_t doubles = 0, ints = 0; };
inline ChainWsSize carve(ChainWs& w, const ChainDims& c, size_t batch, double* d, int32_t* i) {
    w = ChainWs{};
    ChainWsSize used;
    chain_ws_arrays(w, c, [&](const char*, auto*& p, size_t per) {
        if constexpr (std::is_same_v<decltype(p), double*&>) { p = d ? d + used.doubles : nullptr; used.doubles += batch * per; }
        else { p = i ? i + used.ints : nullptr; used.ints += batch * per; }
    });
    return used;
}

}  // namespace pqp_internal
