// pqp_kernels.hip — gfx950 (MI355X / CDNA4) kernels and the C ABI of include/pqp.h.
//
//   path_solve_kernel     the lane-per-waypoint path-QP kernel lives in pqp_path_solve.hip (one translation unit per workgroup width);
//                         this file holds its launcher, path_solve_impl.
//   path_assemble_kernel  BaseSolver::setCost/setConstraints in the REFERENCE numbering: CSC values of A,
//                         diagonal of P, l, u; staged through LDS and written with contiguous, coalesced
//                         stores (base_solver.cpp:119-261).
//   path_pattern_kernel   the value-independent CSC pattern (integer index maps, base_solver.cpp:154-209).
//   path_gather_solution  lane layout -> reference numbering of the primal / dual solution.
//
// No CPU fallback: every entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>

#include "pqp_defaults.hpp"
#include "pqp_path_lane.hpp"
#include "pqp_banded_qp.hpp"
#include "pqp_path_lq_abi.hpp"
#include <vector>

#include "pqp_wave.hpp"

namespace pqp {

// -------------------------------------------------------------------------------------------------------
// reference numbering helpers (base_solver.cpp:22-37,154-158)
// -------------------------------------------------------------------------------------------------------
struct RefIndex {
    int n, precise;
    __host__ __device__ int state() const { return 3 * n; }
    __host__ __device__ int control() const { return n - 1; }
    __host__ __device__ int vars() const { return 3 * n + n - 1 + precise + n; }
    __host__ __device__ int cons() const { return 4 * n + precise + n + 2; }
    __host__ __device__ int kappa_idx() const { return 3 * n; }
    __host__ __device__ int precise_idx() const { return 4 * n; }
    __host__ __device__ int rough_idx() const { return 4 * n + 2 * precise; }
    __host__ __device__ int end_idx() const { return 4 * n + 2 * precise + n - precise; }
    __host__ __device__ int slack_col(int i, int which) const {
        return i < precise ? 4 * n - 1 + 2 * i + which : 4 * n - 1 + 2 * precise + (i - precise);
    }
    __host__ __device__ int nnz_a() const { return 3 * n + 7 * (n - 1) + n + 6 * precise + 2 * (n - precise) + 2; }
    __host__ __device__ int nnz_p() const { return n + n - 1 + precise + n; }
    // CSC offset of the first entry of column 3i (state column block of waypoint i)
    __host__ __device__ int state_col_offset(int i) const {
        // per waypoint j < n-1: precise -> 5+5+4 = 14 entries, rough -> 4+3+4 = 11
        const int np = i < precise ? i : precise;
        return 14 * np + 11 * (i - np);
    }
    __host__ __device__ int control_col_offset() const {
        // all state columns: waypoints 0..n-2 full, last waypoint has no outgoing transition (-2 per column)
        // but two end rows (+1 on l and psi): l: 1 + (2|1) + 1, psi: 1 + (2|0) + 1, k: 1 + 1
        const bool last_precise = (n - 1) < precise;
        return state_col_offset(n - 1) + (last_precise ? 4 + 4 + 2 : 3 + 2 + 2);
    }
    __host__ __device__ int slack_col_offset() const { return control_col_offset() + (n - 1); }
};

// pattern: rows[nnz_a], colptr[vars+1], pcols[nnz_p]; one thread per waypoint
__global__ void path_pattern_kernel(RefIndex R, int32_t* rows, int32_t* colptr, int32_t* pcols) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = R.n;
    if (i >= n) return;
    const bool precise = i < R.precise, has_next = i < n - 1, last = i == n - 1;
    int o = R.state_col_offset(i);
    // column l_i
    colptr[3 * i] = o;
    rows[o++] = 3 * i;
    if (has_next) { rows[o++] = 3 * (i + 1); rows[o++] = 3 * (i + 1) + 1; }
    if (precise) { rows[o++] = R.precise_idx() + 2 * i; rows[o++] = R.precise_idx() + 2 * i + 1; }
    else rows[o++] = R.rough_idx() + (i - R.precise);
    if (last) rows[o++] = R.end_idx();
    // column psi_i
    colptr[3 * i + 1] = o;
    rows[o++] = 3 * i + 1;
    if (has_next) { rows[o++] = 3 * (i + 1); rows[o++] = 3 * (i + 1) + 1; }
    if (precise) { rows[o++] = R.precise_idx() + 2 * i; rows[o++] = R.precise_idx() + 2 * i + 1; }
    if (last) rows[o++] = R.end_idx() + 1;
    // column k_i
    colptr[3 * i + 2] = o;
    rows[o++] = 3 * i + 2;
    if (has_next) { rows[o++] = 3 * (i + 1) + 1; rows[o++] = 3 * (i + 1) + 2; }
    rows[o++] = R.kappa_idx() + i;
    // control column u_i
    if (has_next) {
        const int oc = R.control_col_offset() + i;
        colptr[R.state() + i] = oc;
        rows[oc] = 3 * (i + 1) + 2;
    }
    // slack columns
    const int os = R.slack_col_offset();
    if (precise) {
        colptr[R.slack_col(i, 0)] = os + 2 * i;
        colptr[R.slack_col(i, 1)] = os + 2 * i + 1;
        rows[os + 2 * i] = R.precise_idx() + 2 * i;
        rows[os + 2 * i + 1] = R.precise_idx() + 2 * i + 1;
    } else {
        const int li = i - R.precise;
        colptr[R.slack_col(i, 0)] = os + 2 * R.precise + li;
        rows[os + 2 * R.precise + li] = R.rough_idx() + li;
    }
    if (last) colptr[R.vars()] = R.nnz_a();
    // P diagonal columns (base_solver.cpp:127-143), ascending: k_i, then u_i, then slacks
    pcols[i] = 3 * i + 2;
    if (has_next) pcols[n + i] = R.state() + i;
    if (precise) { pcols[2 * n - 1 + 2 * i] = R.slack_col(i, 0); pcols[2 * n - 1 + 2 * i + 1] = R.slack_col(i, 1); }
    else pcols[2 * n - 1 + 2 * R.precise + (i - R.precise)] = R.slack_col(i, 0);
}

// assemble in the reference numbering.  One workgroup per QP; values are staged in LDS in their final
// order and then streamed out with unit-stride stores.
__global__ void __launch_bounds__(256) path_assemble_kernel(RefIndex R, int batch, const double* __restrict__ ref,
                                                            const double* __restrict__ lin, const double* __restrict__ bounds,
                                                            const double* __restrict__ scal, pqp_params prm,
                                                            double* __restrict__ a_val, double* __restrict__ p_val,
                                                            double* __restrict__ lower, double* __restrict__ upper,
                                                            int stage_in_lds) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int n = R.n, nnz_a = R.nnz_a(), nnz_p = R.nnz_p(), cons = R.cons();
    for (int qp = blockIdx.x; qp < batch; qp += gridDim.x) {
        double* va = stage_in_lds ? smem : a_val + (size_t)qp * nnz_a;
        double* vp = stage_in_lds ? smem + nnz_a : p_val + (size_t)qp * nnz_p;
        double* vl = stage_in_lds ? smem + nnz_a + nnz_p : lower + (size_t)qp * cons;
        double* vu = stage_in_lds ? smem + nnz_a + nnz_p + cons : upper + (size_t)qp * cons;
        const double* rq = ref + (size_t)qp * n * PQP_REF_STRIDE;
        const double* lq = lin ? lin + (size_t)qp * n * PQP_LIN_STRIDE : nullptr;
        const double* bq = bounds + (size_t)qp * n * PQP_BOUNDS_STRIDE;
        const double* sc = scal + (size_t)qp * PQP_SCAL_STRIDE;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const bool precise = i < R.precise, has_next = i < n - 1, last = i == n - 1;
            double a[6] = {0, 0, 0, 0, 0, 0}, c3[3] = {0, 0, 0};
            if (has_next) {   // outgoing transition i -> i+1 fills the columns of waypoint i
                double lp[3];
                double knext;
                if (lq) { lp[0] = lq[3 * i]; lp[1] = lq[3 * i + 1]; lp[2] = lq[3 * i + 2]; knext = lq[3 * (i + 1) + 2]; }
                else { lp[0] = 0.0; lp[1] = 0.0; lp[2] = rq[5 * i + 1]; knext = rq[5 * (i + 1) + 1]; }
                transition_block(lp, knext, rq[5 * i], rq[5 * (i + 1)], rq[5 * i + 1], a, c3);
            }
            int o = R.state_col_offset(i);
            // column l_i
            va[o++] = -1.0;
            if (has_next) { va[o++] = a[0]; va[o++] = a[2]; }
            if (precise) { va[o++] = 1.0; va[o++] = 1.0; } else va[o++] = 1.0;
            if (last) va[o++] = 1.0;
            // column psi_i
            va[o++] = -1.0;
            if (has_next) { va[o++] = a[1]; va[o++] = a[3]; }
            if (precise) { va[o++] = prm.front_length; va[o++] = prm.rear_length; }
            if (last) va[o++] = 1.0;
            // column k_i
            va[o++] = -1.0;
            if (has_next) { va[o++] = a[4]; va[o++] = 1.0; }
            va[o++] = 1.0;
            if (has_next) va[R.control_col_offset() + i] = a[5];
            const int os = R.slack_col_offset();
            if (precise) { va[os + 2 * i] = 1.0; va[os + 2 * i + 1] = 1.0; }
            else va[os + 2 * R.precise + (i - R.precise)] = 1.0;
            // P diagonal (base_solver.cpp:123-143)
            vp[i] = prm.weight_kappa;
            if (has_next) vp[n + i] = prm.weight_dkappa;
            if (precise) { vp[2 * n - 1 + 2 * i] = prm.weight_slack; vp[2 * n - 1 + 2 * i + 1] = prm.weight_slack; }
            else vp[2 * n - 1 + 2 * R.precise + (i - R.precise)] = prm.weight_slack;
            // bounds (base_solver.cpp:212-260)
            if (i == 0) {
                for (int k = 0; k < 3; ++k) { vl[k] = -sc[k]; vu[k] = -sc[k]; }
            }
            if (has_next) {
                for (int k = 0; k < 3; ++k) { vl[3 * (i + 1) + k] = -c3[k]; vu[3 * (i + 1) + k] = -c3[k]; }
            }
            const double kappa_limit = tan(sc[5]) / prm.wheel_base;
            vl[R.kappa_idx() + i] = -kappa_limit;
            vu[R.kappa_idx() + i] = kappa_limit;
            double lo, up;
            if (precise) {
                soft_bounds(bq[6 * i], bq[6 * i + 1], prm.expected_safety_margin, prm.min_clearance, lo, up);
                vl[R.precise_idx() + 2 * i] = lo; vu[R.precise_idx() + 2 * i] = up;
                soft_bounds(bq[6 * i + 2], bq[6 * i + 3], prm.expected_safety_margin, prm.min_clearance, lo, up);
                vl[R.precise_idx() + 2 * i + 1] = lo; vu[R.precise_idx() + 2 * i + 1] = up;
            } else {
                soft_bounds(bq[6 * i + 4], bq[6 * i + 5], prm.expected_safety_margin, prm.min_clearance, lo, up);
                vl[R.rough_idx() + (i - R.precise)] = lo; vu[R.rough_idx() + (i - R.precise)] = up;
            }
            if (last) {
                vl[R.end_idx()] = -prm.end_l_bound; vu[R.end_idx()] = prm.end_l_bound;
                double el = -kInfty, eu = kInfty;
                if (prm.constraint_end_heading && sc[4] == 0.0) {
                    const double end_psi = constrain_angle(sc[3] - rq[5 * i + 2]);
                    if (end_psi < prm.end_psi_max) { el = end_psi - prm.end_psi_tol; eu = end_psi + prm.end_psi_tol; }
                }
                vl[R.end_idx() + 1] = el; vu[R.end_idx() + 1] = eu;
            }
        }
        if (stage_in_lds) {
            __syncthreads();
            double* ga = a_val + (size_t)qp * nnz_a;
            double* gp = p_val + (size_t)qp * nnz_p;
            double* gl = lower + (size_t)qp * cons;
            double* gu = upper + (size_t)qp * cons;
            for (int k = threadIdx.x; k < nnz_a; k += blockDim.x) ga[k] = smem[k];
            for (int k = threadIdx.x; k < nnz_p; k += blockDim.x) gp[k] = smem[nnz_a + k];
            for (int k = threadIdx.x; k < cons; k += blockDim.x) gl[k] = smem[nnz_a + nnz_p + k];
            for (int k = threadIdx.x; k < cons; k += blockDim.x) gu[k] = smem[nnz_a + nnz_p + cons + k];
            __syncthreads();
        }
    }
}

// lane layout (handle's warm state) -> reference numbering (OsqpEigen getSolution order)
__global__ void path_gather_solution(RefIndex R, int batch, const double* __restrict__ wx, const double* __restrict__ wy,
                                     const double* __restrict__ wye, double* __restrict__ x, double* __restrict__ y) {
    const int n = R.n;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * n) return;
    const int qp = idx / n, i = idx - qp * n;
    const double* sx = wx + (size_t)idx * 6;
    const double* sy = wy + (size_t)idx * 6;
    if (x) {
        double* xo = x + (size_t)qp * R.vars();
        xo[3 * i] = sx[0]; xo[3 * i + 1] = sx[1]; xo[3 * i + 2] = sx[2];
        if (i > 0) xo[R.state() + i - 1] = sx[3];
        xo[R.slack_col(i, 0)] = sx[4];
        if (i < R.precise) xo[R.slack_col(i, 1)] = sx[5];
    }
    if (y) {
        double* yo = y + (size_t)qp * R.cons();
        yo[3 * i] = sy[0]; yo[3 * i + 1] = sy[1]; yo[3 * i + 2] = sy[2];
        yo[R.kappa_idx() + i] = sy[3];
        if (i < R.precise) { yo[R.precise_idx() + 2 * i] = sy[4]; yo[R.precise_idx() + 2 * i + 1] = sy[5]; }
        else yo[R.rough_idx() + (i - R.precise)] = sy[4];
        if (i == n - 1) { yo[R.end_idx()] = wye[2 * qp]; yo[R.end_idx() + 1] = wye[2 * qp + 1]; }
    }
}

// constrainAngle (include/tools/tools.hpp:24-35) as the kernels of this library evaluate it: what pqp_constrain_angle_device exposes
__global__ void constrain_angle_kernel(int count, const double* __restrict__ in, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = constrain_angle(in[i]);
}

}  // namespace pqp

#include "pqp_smoother_kernels.inc"
#include "pqp_corridor_kernels.inc"
#include "pqp_distance_kernels.inc"
#include "pqp_footprint_kernels.inc"
#include "pqp_select_kernels.inc"
#include "pqp_project_kernels.inc"

// =========================================================================================================
// C ABI
// =========================================================================================================
namespace {
thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
#define PQP_HIP(call)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return fail(PQP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// every (re)allocation of a device buffer of the library: captured hipGraphs of the chain hold device pointers and are only replayed
// while this has not moved (pqp_chain.inc)
std::atomic<unsigned long long> g_alloc_generation{0};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int ensure(size_t need) {
        if (need <= bytes) return PQP_OK;
        g_alloc_generation.fetch_add(1, std::memory_order_relaxed);
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        PQP_HIP(hipMalloc(&p, need));
        bytes = need;
        // No call ever reads uninitialised device memory (warm state of skipped QPs, info rows).  hipMemset runs on the NULL stream and
        // may return before the fill has executed; the handles' streams are non-blocking, i.e. NOT ordered behind the NULL stream, so a
        // fill still queued there could land on the buffer milliseconds later, after kernels of the handle have written it (seen: a
        // whole smoother batch solved on zeroed problem data).  Allocation is rare: wait for the fill.
        PQP_HIP(hipMemset(p, 0, need));
        PQP_HIP(hipStreamSynchronize(nullptr));
        return PQP_OK;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// one CU's LDS on gfx950: the most dynamic LDS a workgroup can have
constexpr size_t kLdsPerCu = 160 * 1024;

// the static LDS of kernel `fn`: its __shared__ variables, padded to the alignment of the dynamic LDS that follows them (the compiler's
// "LDS Size" remark; 16 bytes for a single int in front of an aligned(16) array).  Looked up once per kernel.
int static_lds(const void* fn, size_t* out) {
    static std::mutex mu;
    static std::vector<std::pair<const void*, size_t>> known;
    std::lock_guard<std::mutex> lock(mu);
    for (const auto& k : known)
        if (k.first == fn) { *out = k.second; return PQP_OK; }
    hipFuncAttributes fa{};
    PQP_HIP(hipFuncGetAttributes(&fa, fn));
    known.emplace_back(fn, fa.sharedSizeBytes);
    *out = fa.sharedSizeBytes;
    return PQP_OK;
}

// `bytes` of dynamic LDS for kernel `fn`: PQP_ERR_CAPACITY (message `who`) when they and the kernel's static LDS exceed one CU's LDS, the
// opt-in beyond the 48 KiB any kernel may use.  The attribute takes the dynamic bytes alone (the runtime adds the static ones to it).
int lds_opt_in(const void* fn, size_t bytes, const char* who) {
    size_t fixed = 0;
    if (const int rc = static_lds(fn, &fixed)) return rc;
    if (bytes > kLdsPerCu - fixed) return fail(PQP_ERR_CAPACITY, who);
    if (fixed + bytes > 48 * 1024) PQP_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return PQP_OK;
}

// PQP_OPT_LONG_LINES = `opt`: whether a launch of the LDS kernel `fn` with `bytes` of dynamic LDS goes to its long form
// (long_*_kernel, pqp_corridor_kernels.inc) - never (0), where the LDS kernel does not fit one CU (1), always (2)
int long_form(int opt, const void* fn, size_t bytes, bool* out) {
    *out = opt == 2;
    if (opt != 1) return PQP_OK;
    size_t fixed = 0;
    if (const int rc = static_lds(fn, &fixed)) return rc;
    *out = bytes > kLdsPerCu - fixed;
    return PQP_OK;
}
}  // namespace

struct pqp_handle {
    int device = 0;
    pqp_params prm;
    hipStream_t stream = nullptr;
    // HIP events around the dominant kernel of every call, on the stream it is launched on: a ring of the last kEvRing launches,
    // read back (after the work is done) by pqp_last_kernel_ms / pqp_kernel_ms_history without putting a sync between launches.
    // One slot more than the history: the one launch_timed records into, which a launch that fails may leave half recorded.
    static constexpr int kEvRing = 256, kEvSlots = kEvRing + 1;
    hipEvent_t evs0[kEvSlots] = {}, evs1[kEvSlots] = {};
    long long ev_count = 0;          // launches recorded so far
    bool timed = false;              // the last of them is what pqp_last_kernel_ms reports
    static constexpr int kMarks = 8;
    static constexpr int kChainMarks = 2;      // + two events of pqp_optimize_path_device's own
    hipEvent_t marks[kMarks + kChainMarks] = {};   // pqp_mark / pqp_wait_mark: ordering between the streams of two handles
    // the launches of one call between the next pair of the ring's events, which count only once the launches were accepted: a call that
    // fails leaves the timing of the previous one.  No events inside a graph capture.
    template <class F> int launch_timed(F&& launch) {
        if (capturing) return launch();
        const int slot = (int)(ev_count % kEvSlots);
        PQP_HIP(hipEventRecord(evs0[slot], stream));
        if (const int rc = launch()) return rc;
        PQP_HIP(hipEventRecord(evs1[slot], stream));
        ev_count += 1;
        timed = true;
        return PQP_OK;
    }
    // PQP_OPT_CHAIN_GRAPH: pqp_optimize_path_device captured as hipGraphs (pqp_chain.inc).  capturing: the handle's stream is in capture
    // mode - no timing events, the path solve resets its ticket counter inside the graph
    bool capturing = false;
    int opt_chain_graph = 0;
    struct ChainGraph { std::vector<unsigned char> key; hipGraphExec_t exec = nullptr; bool failed = false; bool lane_launch = false; long long lane_launches = 0; int path_kernel = 0; unsigned long long ticket_after = 0; };
    std::vector<ChainGraph> chain_graphs;
    int warm_batch = 0, warm_n = 0;
    bool warm_stored = false;                   // the last solve wrote its final iterate to wx / wy / wye
    DevBuf wx, wy, wye, wrho, wsave, wscale;    // warm state (lane layout) + polish save area, parked Ruiz vectors (per workgroup slot)
    // work distribution of the solve kernel: ticket counter (never reset: a launch uses batch + grid tickets), cost bins of the
    // last solve and the ticket -> QP order derived from them
    DevBuf ticket, cost_key, cost_hist, order;
    DevBuf chain_d, chain_i;                    // workspace of pqp_optimize_path_device
    unsigned long long ticket_next = 0;
    long long solves = 0;                       // solve launches so far (parity selects the cost histogram being filled)
    int hist_batch = 0, hist_n = 0;             // shape of the solve whose costs cost_key / cost_hist hold (0: none)
    int opt_store_warm = 1, opt_order_by_cost = 0, opt_reserve_cus = 0, opt_stream_batch = -1, opt_carry = 0, opt_stream_staged = -1;      // (opt_stream_batch < 0: stream_batch_auto(n))
    int opt_long_lines = 0;                            // PQP_OPT_LONG_LINES: 0 LDS forms only, 1 long form where the LDS form does not fit, 2 long forms
    DevBuf line_ws;                                    // workspace of the long forms of the line kernels (one launch at a time on the stream)
    int stream_last_batch = 0, stream_last_n = 0;      // shape of the last path_stream_kernel launch (what its workspace still holds)
    int last_path_kernel = 0;                          // pqp_path_kernel of the last pqp_path_solve* launch (pqp_last_path_kernel)
    DevBuf sm_act[2];                                  // final active sets of the exact TensionSmoother / postSmooth kernels (PQP_OPT_CARRY_CYCLES)
    int sm_act_batch[2] = {0, 0}, sm_act_n[2] = {0, 0};
    DevBuf stream_ws;                           // workspace of path_stream_kernel
    DevBuf stream_key, stream_hist, stream_order;      // PQP_OPT_ORDER_BY_COST on that kernel: phase keys, key histogram, two slot -> QP maps
    long long stream_solves = 0;                // ordered launches so far (parity selects the map being read)
    int stream_order_batch = 0, stream_order_n = 0;    // shape the map being read was built for (0: none)
    int num_cu = 0;
    int blocks_per_cu[8] = {0, 0, 0, 0, 0, 0, 0, 0};    // occupancy of the solve kernel variants [log2(nw)][cert]
    static constexpr int kStage = 12;
    DevBuf stage[kStage];                       // device copies of the arrays of a host-pointer entry point (Staging), in argument order
    // smoother QPs: banded problem data + shared sparsity (cached per type and size)
    DevBuf b_pband, b_q, b_aval, b_lo, b_up, b_x, b_y, b_acol, b_trow, b_tslot;
    int b_struct_type = -1, b_struct_n = -1;
};

namespace {
int hip_ok(hipError_t e, const char* what) { return e == hipSuccess ? PQP_OK : fail(PQP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

// The host-pointer form of an entry point: device copies of its arrays from the handle's pool, in argument order.  in() copies a host array in
// (nullptr stays nullptr); out() hands out a device array, first set to the byte `fill` if that is not negative, which run() copies back when
// the host pointer is not null.  The first failure is kept and every later step skipped.  What was enqueued reads or writes the caller's
// memory, so no return leaves it queued: run() synchronises after the copies back, the destructor on any other return.
class Staging {
  public:
    explicit Staging(pqp_handle* h) : h_(h) { rc_ = hip_ok(hipSetDevice(h->device), "hipSetDevice"); }
    ~Staging() { if (pending_) (void)hipStreamSynchronize(h_->stream); }
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    template <class T> T* in(const T* host, size_t count) { return host ? static_cast<T*>(take(count * sizeof(T), host, nullptr, -1)) : nullptr; }
    template <class T> T* out(T* host, size_t count, int fill = -1) { return static_cast<T*>(take(count * sizeof(T), nullptr, host, fill)); }
    // the device form on the staged arrays, then the copies back
    template <class F> int run(F&& device_form) {
        if (rc_ || (rc_ = device_form())) return rc_;
        for (int k = 0; k < n_back_ && !rc_; ++k)
            rc_ = hip_ok(hipMemcpyAsync(back_[k].host, back_[k].dev, back_[k].bytes, hipMemcpyDeviceToHost, h_->stream), "hipMemcpyAsync(device to host)");
        if (!rc_ && !(rc_ = hip_ok(hipStreamSynchronize(h_->stream), "hipStreamSynchronize"))) pending_ = false;
        return rc_;
    }

  private:
    void* take(size_t bytes, const void* src, void* host_out, int fill) {
        if (rc_) return nullptr;
        if (used_ == pqp_handle::kStage) { rc_ = fail(PQP_ERR_INVALID, "staging: more arrays than the handle's pool holds"); return nullptr; }
        DevBuf& b = h_->stage[used_++];
        if ((rc_ = b.ensure(bytes))) return nullptr;
        pending_ = true;
        if (src) rc_ = hip_ok(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, h_->stream), "hipMemcpyAsync(host to device)");
        else if (fill >= 0) rc_ = hip_ok(hipMemsetAsync(b.p, fill, bytes, h_->stream), "hipMemsetAsync");
        if (host_out) back_[n_back_++] = {host_out, b.p, bytes};
        return rc_ ? nullptr : b.p;
    }
    struct Back { void* host; const void* dev; size_t bytes; };
    pqp_handle* h_;
    int rc_ = PQP_OK, used_ = 0, n_back_ = 0;
    bool pending_ = false;
    Back back_[pqp_handle::kStage];
};
}  // namespace

// PQP_OPT_CARRY_CYCLES for an exact smoother kernel (slot 0: TensionSmoother, 1: postSmooth): the active set every scenario ended with is kept
// on the handle; a solve of the shape of the previous one (and the buffer still where it was) starts from it (carry = 1)
static int sm_carry_slot(pqp_handle* h, int slot, int batch, int n, signed char*& act_io, int& carry) {
    act_io = nullptr;
    carry = 0;
    if (!h->opt_carry) return PQP_OK;
    const void* before = h->sm_act[slot].p;
    int rc;
    if ((rc = h->sm_act[slot].ensure((size_t)batch * n))) return rc;
    act_io = h->sm_act[slot].as<signed char>();
    carry = (h->sm_act_batch[slot] == batch && h->sm_act_n[slot] == n && before == h->sm_act[slot].p) ? 1 : 0;
    h->sm_act_batch[slot] = batch; h->sm_act_n[slot] = n;
    return PQP_OK;
}

// One launch of an exact smoother kernel (tension_exact_kernel / post_exact_kernel) on n elements per scenario: launch(K, ws) with K = the fewest
// chunks of 64 per lane that hold them (SmRegs<K>), or K = 0 beyond 1024 with `arrays` workspace arrays per scenario in HBM (SmHbm, ws).
// (twelve / sixteen per lane: the lane state no longer fits the registers - S2 1.8 / 3.3 KB of scratch per lane - but lines that long are rare,
//  a point per metre of reference line, and the recursion down the lanes, not the spills, is what their time goes to)
template <class F>
static int sm_exact_launch(pqp_handle* h, int batch, int n, int arrays, F&& launch) {
    int rc;
    if (n > 1024 && (rc = h->b_pband.ensure((size_t)batch * arrays * (64 * (((size_t)n + 63) / 64)) * 8))) return rc;
    double* ws = n > 1024 ? h->b_pband.as<double>() : nullptr;
    return h->launch_timed([&]() -> int {
        if (n <= 64) launch(std::integral_constant<int, 1>(), ws);
        else if (n <= 128) launch(std::integral_constant<int, 2>(), ws);
        else if (n <= 256) launch(std::integral_constant<int, 4>(), ws);
        else if (n <= 384) launch(std::integral_constant<int, 6>(), ws);
        else if (n <= 512) launch(std::integral_constant<int, 8>(), ws);
        else if (n <= 768) launch(std::integral_constant<int, 12>(), ws);
        else if (n <= 1024) launch(std::integral_constant<int, 16>(), ws);
        else launch(std::integral_constant<int, 0>(), ws);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

// One launch of a line-geometry kernel under PQP_OPT_LONG_LINES: the LDS kernel `fn` with `lds` bytes of dynamic LDS, refused with `who` where
// they exceed one CU's, or - by long_form() - its long form, with `ws_bytes` of the handle's workspace if it takes one.  launch(go_long, ws)
// enqueues the one (std::false_type) or the other (std::true_type).  long_fn / long_lds / long_who: the long form's own dynamic LDS (the DP's).
template <class F>
static int line_launch(pqp_handle* h, const void* fn, size_t lds, const char* who, size_t ws_bytes, F&& launch, const void* long_fn = nullptr,
                       size_t long_lds = 0, const char* long_who = nullptr) {
    bool go_long = false;
    int rc = long_form(h->opt_long_lines, fn, lds, &go_long);
    if (!rc && !go_long) rc = lds_opt_in(fn, lds, who);
    if (!rc && go_long && long_fn) rc = lds_opt_in(long_fn, long_lds, long_who);
    if (!rc && go_long && ws_bytes) rc = h->line_ws.ensure(ws_bytes);
    if (rc) return rc;
    double* ws = h->line_ws.as<double>();
    return h->launch_timed([&]() -> int {
        if (go_long) launch(std::true_type(), ws);
        else launch(std::false_type(), ws);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

extern "C" {

void pqp_default_params(pqp_params* p) { if (p) pqp::default_params(p); }
void pqp_production_params(pqp_params* p) { if (p) pqp::production_params(p); }
const char* pqp_last_error(void) { return g_last_error.c_str(); }
void pqp_set_last_error(const char* msg) { g_last_error = msg ? msg : ""; }      // for the other translation units of the library
const char* pqp_version(void) { return "pqp-hip 0.1 (gfx950)"; }

int pqp_create(pqp_handle** out, const pqp_params* params, int device, int max_batch, int max_n) {
    if (!out) return fail(PQP_ERR_INVALID, "pqp_create: null handle pointer");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PQP_ERR_NO_DEVICE, "pqp_create: no HIP device (this library has no CPU fallback)");
    if (device < 0 || device >= count) return fail(PQP_ERR_INVALID, "pqp_create: bad device ordinal");
    PQP_HIP(hipSetDevice(device));
    pqp_handle* h = new (std::nothrow) pqp_handle();
    if (!h) return fail(PQP_ERR_INVALID, "pqp_create: out of host memory");
    h->device = device;
    if (params) h->prm = *params; else pqp::default_params(&h->prm);
    // (a failure below destroys what was built so far: pqp_destroy tolerates a partially built handle)
    auto build = [&]() -> int {
        PQP_HIP(hipDeviceGetAttribute(&h->num_cu, hipDeviceAttributeMultiprocessorCount, device));
        PQP_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        for (int k = 0; k < pqp_handle::kEvSlots; ++k) { PQP_HIP(hipEventCreate(&h->evs0[k])); PQP_HIP(hipEventCreate(&h->evs1[k])); }
        for (int k = 0; k < pqp_handle::kMarks + pqp_handle::kChainMarks; ++k) PQP_HIP(hipEventCreateWithFlags(&h->marks[k], hipEventDisableTiming));
        int rc;
        if ((rc = h->ticket.ensure(8)) || (rc = h->cost_hist.ensure(2 * pqp::kCostBins * 4))) return rc;
        if (max_batch > 0 && max_n > 0) {
            const size_t bn = (size_t)max_batch * max_n;
            if ((rc = h->wx.ensure(bn * 6 * 8)) || (rc = h->wy.ensure(bn * 6 * 8)) || (rc = h->wye.ensure((size_t)max_batch * 2 * 8)) ||
                (rc = h->wrho.ensure((size_t)max_batch * 8)))
                return rc;
        }
        return PQP_OK;
    };
    const int rc = build();
    if (rc != PQP_OK) { (void)pqp_destroy(h); return rc; }
    *out = h;
    return PQP_OK;
}

int pqp_destroy(pqp_handle* h) {
    if (!h) return PQP_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    // (captured chains of OTHER handles may hold this handle's workspaces and events - the smoother handle of a pair: their keys carry the
    //  allocation generation, so none of them is replayed after this)
    g_alloc_generation.fetch_add(1, std::memory_order_relaxed);
    for (auto& g : h->chain_graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    h->chain_graphs.clear();
    for (int k = 0; k < pqp_handle::kEvSlots; ++k) { if (h->evs0[k]) (void)hipEventDestroy(h->evs0[k]); if (h->evs1[k]) (void)hipEventDestroy(h->evs1[k]); }
    for (int k = 0; k < pqp_handle::kMarks + pqp_handle::kChainMarks; ++k) if (h->marks[k]) (void)hipEventDestroy(h->marks[k]);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;           // (its DevBufs free themselves)
    return PQP_OK;
}

int pqp_set_params(pqp_handle* h, const pqp_params* params) {
    if (!h || !params) return fail(PQP_ERR_INVALID, "pqp_set_params: null argument");
    if (params->scaling < -64 || params->scaling > 64) return fail(PQP_ERR_INVALID, "pqp_set_params: |scaling| (equilibration passes) beyond 64");
    h->prm = *params;
    return PQP_OK;
}

int pqp_set_option(pqp_handle* h, int option, int value) {
    if (!h) return fail(PQP_ERR_INVALID, "pqp_set_option: null handle");
    switch (option) {
        case PQP_OPT_STORE_WARM: h->opt_store_warm = value ? 1 : 0; return PQP_OK;
        case PQP_OPT_ORDER_BY_COST: h->opt_order_by_cost = value ? 1 : 0; h->hist_batch = 0; h->stream_order_batch = 0; return PQP_OK;
        case PQP_OPT_RESERVE_CUS: h->opt_reserve_cus = value < 0 ? 0 : value; return PQP_OK;
        case PQP_OPT_STREAM_BATCH: h->opt_stream_batch = value < 0 ? -1 : value; return PQP_OK;
        case PQP_OPT_STREAM_STAGED: h->opt_stream_staged = value < 0 ? -1 : (value ? 1 : 0); h->stream_last_batch = 0; return PQP_OK;      // (another layout: nothing to carry)
        case PQP_OPT_CARRY_CYCLES: h->opt_carry = value < 0 ? 0 : (value > 64 ? 64 : value); h->stream_last_batch = 0; h->sm_act_batch[0] = h->sm_act_batch[1] = 0; return PQP_OK;
        case PQP_OPT_CHAIN_GRAPH: h->opt_chain_graph = value == 2 ? 2 : (value ? 1 : 0); return PQP_OK;
        case PQP_OPT_LONG_LINES: h->opt_long_lines = value >= 2 ? 2 : (value == 1 ? 1 : 0); return PQP_OK;
        default: return fail(PQP_ERR_INVALID, "pqp_set_option: unknown option");
    }
}

int pqp_get_stream(pqp_handle* h, void** s) {
    if (!h || !s) return fail(PQP_ERR_INVALID, "pqp_get_stream: null argument");
    *s = (void*)h->stream;
    return PQP_OK;
}

int pqp_stream_wait(pqp_handle* h, void* other_stream) {
    if (!h) return fail(PQP_ERR_INVALID, "pqp_stream_wait: null handle");
    PQP_HIP(hipSetDevice(h->device));
    hipEvent_t ev;
    PQP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, (hipStream_t)other_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, ev, 0);
    (void)hipEventDestroy(ev);                 // released once the wait has completed
    if (e != hipSuccess) return fail(PQP_ERR_HIP, std::string("pqp_stream_wait: ") + hipGetErrorString(e));
    return PQP_OK;
}

int pqp_mark(pqp_handle* h, int slot) {
    if (!h || slot < 0 || slot >= pqp_handle::kMarks) return fail(PQP_ERR_INVALID, "pqp_mark: bad handle or slot (0..7)");
    PQP_HIP(hipSetDevice(h->device));
    PQP_HIP(hipEventRecord(h->marks[slot], h->stream));
    return PQP_OK;
}

int pqp_wait_mark(pqp_handle* h, pqp_handle* other, int slot) {
    if (!h || !other || slot < 0 || slot >= pqp_handle::kMarks) return fail(PQP_ERR_INVALID, "pqp_wait_mark: bad handle or slot (0..7)");
    PQP_HIP(hipSetDevice(h->device));
    PQP_HIP(hipStreamWaitEvent(h->stream, other->marks[slot], 0));       // (a mark never recorded counts as complete)
    return PQP_OK;
}

int pqp_sync(pqp_handle* h) {
    if (!h) return fail(PQP_ERR_INVALID, "pqp_sync: null handle");
    PQP_HIP(hipSetDevice(h->device));
    PQP_HIP(hipStreamSynchronize(h->stream));
    return PQP_OK;
}

int pqp_path_sizes(const pqp_params* params, int n, const double* s, pqp_sizes* out) {
    if (!out || n < 2) return fail(PQP_ERR_INVALID, "pqp_path_sizes: need n >= 2 and an output struct");
    pqp_params def;
    if (!params) { pqp::default_params(&def); params = &def; }
    int precise = n;   // base_solver.cpp:24-34
    if (params->rough_constraints_far_away) {
        if (!s) return fail(PQP_ERR_INVALID, "pqp_path_sizes: rough_constraints_far_away needs the arclengths");
        int lo = 0, hi = n;   // std::lower_bound(s, precise_planning_length)
        while (lo < hi) { const int mid = (lo + hi) / 2; if (s[mid] < params->precise_planning_length) lo = mid + 1; else hi = mid; }
        precise = lo;
    }
    pqp::RefIndex R{n, precise};
    out->n = n; out->state = 3 * n; out->control = n - 1; out->precise = precise; out->slack = precise + n;
    out->vars = R.vars(); out->cons = R.cons(); out->nnz_a = R.nnz_a(); out->nnz_p = R.nnz_p();
    return PQP_OK;
}

int pqp_path_pattern(pqp_handle* h, int n, int precise, int32_t* rows, int32_t* colptr, int32_t* pcols) {
    if (!h || !rows || !colptr || !pcols || n < 2 || precise < 0 || precise > n)
        return fail(PQP_ERR_INVALID, "pqp_path_pattern: bad argument");
    pqp::RefIndex R{n, precise};
    Staging st(h);
    int32_t* d_rows = st.out(rows, R.nnz_a(), 0xff);
    int32_t* d_colptr = st.out(colptr, R.vars() + 1, 0xff);
    int32_t* d_pcols = st.out(pcols, R.nnz_p(), 0xff);
    return st.run([&]() -> int {
        hipLaunchKernelGGL(pqp::path_pattern_kernel, dim3((n + 127) / 128), dim3(128), 0, h->stream, R, d_rows, d_colptr, d_pcols);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

static bool assemble_ok(pqp_handle* h, int batch, int n, int precise, const double* ref, const double* bounds, const double* scal, const double* a_val,
                        const double* p_val, const double* lower, const double* upper) {
    return h && ref && bounds && scal && a_val && p_val && lower && upper && batch >= 1 && n >= 2 && precise >= 0 && precise <= n;
}

int pqp_path_assemble_device(pqp_handle* h, int batch, int n, int precise, const double* ref, const double* lin,
                             const double* bounds, const double* scal, double* a_val, double* p_val, double* lower,
                             double* upper) {
    if (!assemble_ok(h, batch, n, precise, ref, bounds, scal, a_val, p_val, lower, upper)) return fail(PQP_ERR_INVALID, "pqp_path_assemble: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    pqp::RefIndex R{n, precise};
    const size_t lds = ((size_t)R.nnz_a() + R.nnz_p() + 2 * (size_t)R.cons()) * 8;
    const int stage = lds <= 150 * 1024 ? 1 : 0;
    int rc;
    if (stage && (rc = lds_opt_in((const void*)pqp::path_assemble_kernel, lds, "pqp_path_assemble: LDS"))) return rc;
    const int grid = batch < 4096 ? batch : 4096;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::path_assemble_kernel, dim3(grid), dim3(256), stage ? lds : 0, h->stream, R, batch, ref, lin, bounds,
                           scal, h->prm, a_val, p_val, lower, upper, stage);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_path_assemble(pqp_handle* h, int batch, int n, int precise, const double* ref, const double* lin,
                      const double* bounds, const double* scal, double* a_val, double* p_val, double* lower, double* upper) {
    if (!assemble_ok(h, batch, n, precise, ref, bounds, scal, a_val, p_val, lower, upper)) return fail(PQP_ERR_INVALID, "pqp_path_assemble: bad argument");
    pqp::RefIndex R{n, precise};
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double *d_ref = st.in(ref, bn * 5), *d_lin = st.in(lin, bn * 3), *d_bounds = st.in(bounds, bn * 6), *d_scal = st.in(scal, (size_t)batch * 6);
    double *d_a = st.out(a_val, (size_t)batch * R.nnz_a()), *d_p = st.out(p_val, (size_t)batch * R.nnz_p());
    double *d_l = st.out(lower, (size_t)batch * R.cons()), *d_u = st.out(upper, (size_t)batch * R.cons());
    return st.run([&]() -> int { return pqp_path_assemble_device(h, batch, n, precise, d_ref, d_lin, d_bounds, d_scal, d_a, d_p, d_l, d_u); });
}

extern "C" hipError_t pqp_stream_launch(const pqp::lq::Args* a, int waves, void* stream);

// Large batches (PQP_OPT_STREAM_BATCH): one lane per QP, state streamed through HBM (pqp_path_lq.hpp).  Same optimum as the
// lane-per-waypoint kernel's KKT-verified polish; no warm state is kept (warm == 1 and pqp_path_get_solution need the other kernel).
static int path_stream_impl(pqp_handle* h, int batch, int n, const int32_t* n_of, const double* ref, const double* lin, const double* bounds,
                            const double* scal, int passes, double* out, int32_t* status, int32_t* iters, double* info) {
    const int waves = (batch + 63) / 64;
    int rc;
    const void* ws_before = h->stream_ws.p;
    if ((rc = h->stream_ws.ensure((size_t)waves * n * pqp::lq::kBlockDoubles * 64 * 8))) return rc;
    pqp::lq::Args a;
    std::memset(&a, 0, sizeof(a));
    a.batch = batch; a.n = n; a.passes = passes; a.n_of = n_of; a.ref = ref; a.lin = lin; a.bounds = bounds; a.scal = scal; a.out = out;
    a.status = status; a.iters = iters; a.info = info; a.ws = h->stream_ws.as<double>(); a.prm = h->prm;
    // Which of the kernel's two workspace layouts (pqp_path_lq_abi.hpp): a launch that leaves SIMDs idle - fewer than 768 wavefronts - waits for its loads, not for
    // HBM's throughput: the sweeps' records staged in LDS two waypoints ahead, +29 ... 33 % at 24 576 / 32 768 QPs of 80 waypoints; a launch that fills the chip
    // loses 3-4 % with them (profiles/r06au_*) and keeps the [field][lane] layout and the register prefetch.  A function of the shape alone: what PQP_OPT_CARRY_CYCLES
    // finds in the workspace was left there in the same layout.
    a.staged = h->opt_stream_staged >= 0 ? h->opt_stream_staged : (waves < 3 * h->num_cu ? 1 : 0);
    // PQP_OPT_CARRY_CYCLES: the workspace still holds, slot by slot, the optimum of the previous launch of this very shape
    a.carry = (h->opt_carry && !lin && h->stream_last_batch == batch && h->stream_last_n == n && h->stream_ws.p == ws_before) ? 1 : 0;       // (lin == NULL: pqp.h)
    // PQP_OPT_ORDER_BY_COST: wavefronts of QPs that ran the same phases in the handle's previous solve of the shape.  Only where it pays - batches that
    // put a wavefront on (nearly) every SIMD: below that a launch lasts as long as one wavefront's sweeps whatever its lanes do (profiles/r05g_*) - and
    // not with PQP_OPT_CARRY_CYCLES (a slot's workspace then holds the previous optimum of the QP that sat there) or inside a graph capture (host-side parity).
    const bool ordered = h->opt_order_by_cost && !h->opt_carry && !h->capturing && waves >= 3 * h->num_cu;
    if (ordered) {
        if ((rc = h->stream_key.ensure((size_t)batch * 4)) || (rc = h->stream_hist.ensure(((size_t)pqp::lq::kOrderBins + 1) * 4)) ||
            (rc = h->stream_order.ensure((size_t)2 * batch * 4)))
            return rc;
        if (h->stream_order_batch != batch || h->stream_order_n != n) {          // a shape change: stale counts, no map yet
            PQP_HIP(hipMemsetAsync(h->stream_hist.p, 0, ((size_t)pqp::lq::kOrderBins + 1) * 4, h->stream));
            a.order = nullptr;
        } else {
            a.order = h->stream_order.as<int32_t>() + (size_t)(h->stream_solves & 1) * batch;
        }
        a.key_out = h->stream_key.as<int32_t>();
        a.hist = h->stream_hist.as<int32_t>();
        a.order_next = h->stream_order.as<int32_t>() + (size_t)((h->stream_solves + 1) & 1) * batch;
    }
    // (path_stream_kernel lives in its own translation unit, pqp_path_stream.hip)
    if ((rc = h->launch_timed([&]() -> int { PQP_HIP(pqp_stream_launch(&a, waves, (void*)h->stream)); return PQP_OK; }))) return rc;
    if (ordered) { h->stream_solves += 1; h->stream_order_batch = batch; h->stream_order_n = n; }
    h->stream_last_batch = batch; h->stream_last_n = n;
    h->warm_batch = batch; h->warm_n = n;
    h->warm_stored = false;
    h->last_path_kernel = PQP_KERNEL_LANE_PER_QP;
    return PQP_OK;
}

// PQP_OPT_STREAM_BATCH "auto": the batch size from which the lane-per-QP kernel is the faster one, by measurement on one MI355X
// (profiles/r05a_crossover_n80.txt, r05a_crossover_n120.txt: 18.7 k QPs at 80 waypoints, ~45 k at 120).  A lone wavefront of that kernel
// takes sweeps x n waypoint steps whatever the batch (5.5 ms at n = 80, 10.5 ms at n = 120), the lane-per-waypoint kernel's time per QP hardly
// depends on n: the crossover grows like n^2.
// Beyond 256 waypoints the lane-per-waypoint kernel runs two wavefronts per SIMD on half the registers and takes 4.1 ... 4.9 us per QP instead
// of 1.0: the crossover is back at 16.7 k / 22.5 k / 32 k QPs at 300 / 400 / 512 waypoints (profiles/r05t_crossover_long_paths.txt): 64 n.
// the lane-per-waypoint kernels, by wavefronts per QP (pqp_path_solve.hip compiled with -DPQP_NW=1 / 2 / 4 / 8); cert: with the in-loop
// infeasibility certificate
extern "C" {
const void* pqp_path_solve_fn_nw1(int cert);
const void* pqp_path_solve_fn_nw2(int cert);
const void* pqp_path_solve_fn_nw4(int cert);
const void* pqp_path_solve_fn_nw8(int cert);
}

// PQP_OPT_STREAM_BATCH's default: where the lane-per-QP kernel overtakes the lane-per-waypoint kernel, one launch after the other on one MI355X, remeasured on
// round 6's kernels (profiles/r06ay_crossover_hybrid.txt, r06az_crossover_other_n.txt).  The lane-per-waypoint kernel's rate steps down with its workgroup width
// (3.5 M paths/s up to 128 waypoints, ~1.1 M up to 256, 0.2 M beyond), a lone wavefront of the other takes sweeps x n waypoint steps: measured crossovers
// 15 k QPs at 80 waypoints, 20 k at 100, 29 k at 120 | 13 k at 160, 34 k at 200, 49 k at 256 | 11.5 k at 300, 24.5 k at 512.
static int stream_batch_auto(int n) {
    if (n > 256) return 48 * n;
    if (n > 128) return (int)(0.75 * n * n);
    const double r = n > 80 ? (double)n / 80.0 : 1.0;
    return (int)(15360.0 * r * sqrt(r));
}
extern "C" int pqp_stream_batch_default(int n) { return n < 2 ? 0 : stream_batch_auto(n); }

static bool path_solve_ok(pqp_handle* h, int batch, int n, const double* ref, const double* bounds, const double* scal, int passes, const double* out) {
    return h && ref && bounds && scal && out && batch >= 1 && n >= 2 && passes >= 0;
}

static int path_solve_impl(pqp_handle* h, int batch, int n, const int32_t* n_of, const double* ref, const double* lin, const double* bounds,
                           const double* scal, int passes, int warm, double* out, int32_t* status, int32_t* iters, double* info) {
    if (!path_solve_ok(h, batch, n, ref, bounds, scal, passes, out)) return fail(PQP_ERR_INVALID, "pqp_path_solve: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    // lane-per-QP kernel: large batches of a caller that keeps no warm state (PQP_OPT_STREAM_BATCH), and every path of more than 512
    // waypoints (the lane-per-waypoint kernel's workgroup ends there; a reference path of 80 m at 0.15 m spacing has 530:
    // reference_path_impl.cpp:321-336) - those with any batch size and without warm state
    // (warm == 1 beyond 512 waypoints: the QP around `lin` is solved cold - its optimum is unique, a warm start only saves iterations -
    //  so BaseSolver::solve + updateProblemFormulationAndSolve work at any size; and there also a handle in the reference's ADMM setting
    //  gets the exact optimum: zero residuals meet OSQP's termination test at any eps)
    const int stream_from = h->opt_stream_batch < 0 ? stream_batch_auto(n) : h->opt_stream_batch;
    if ((n > 512 && (!warm || lin)) || (h->prm.polish != 0 && !warm && !h->opt_store_warm && stream_from > 0 && batch >= stream_from))
        return path_stream_impl(h, batch, n, n_of, ref, lin, bounds, scal, passes, out, status, iters, info);
    // PQP_OPT_CARRY_CYCLES on this kernel: a cold call (warm == 0, lin == NULL) of the shape of the handle's previous solve starts from
    // the final iterate, equilibration and active set that solve left in the warm state - the same scenarios one planning cycle later.
    // (With waypoint counts per QP the state is kept per waypoint: a path that grew or shrank by a few waypoints since the previous cycle
    //  starts its common waypoints from where they were and the new ones from whatever the slot last held there - zero at first.)
    // (only on a handle whose polish returns the exact optimum: with polish == 0 - the reference's ADMM setting - a promoted call would end at an
    //  eps-accurate point that depends on the slot's previous QP, and pqp.h promises the cold solve's optimum to the 1e-7 of the KKT test)
    // (value k >= 2, "tails": only the QPs that were among the most expensive 1 / k of the previous launch - by the cost keys PQP_OPT_ORDER_BY_COST
    //  keeps - start from there, the others start cold: what bounds a launch is its slowest QPs)
    int carry_tails = 0;
    if (h->opt_carry && h->prm.polish != 0 && !warm && !lin && h->warm_stored && h->warm_batch == batch && h->warm_n == n &&
        (h->opt_carry < 2 || (h->opt_order_by_cost && h->hist_batch == batch && h->hist_n == n))) { warm = 1; carry_tails = h->opt_carry >= 2 ? h->opt_carry : 0; }
    if (n > 512) return fail(PQP_ERR_CAPACITY, "pqp_path_solve: warm == 1 beyond 512 waypoints needs the linearisation point (`lin`): the lane-per-QP kernel keeps no warm state");
    if (warm && (h->warm_batch != batch || h->warm_n != n || !h->warm_stored))
        return fail(PQP_ERR_INVALID, "pqp_path_solve: warm == 1 needs a previous solve with the same batch and n (with PQP_OPT_STORE_WARM on)");
    const size_t bn = (size_t)batch * n;
    int rc;
    if (!warm) {
        if ((rc = h->wx.ensure(bn * 6 * 8)) || (rc = h->wy.ensure(bn * 6 * 8)) || (rc = h->wye.ensure((size_t)batch * 2 * 8)) ||
            (rc = h->wrho.ensure((size_t)batch * 8)))
            return rc;
    }
    pqp::PathSolveArgs a;
    std::memset(&a, 0, sizeof(a));
    a.batch = batch; a.n = n; a.n_of = n_of; a.passes = passes; a.warm = warm ? 1 : 0;
    a.ref = ref; a.lin = lin; a.bounds = bounds; a.scal = scal; a.out = out;
    a.status = status; a.iters = iters; a.info = info;
    a.wx = h->wx.as<double>(); a.wy = h->wy.as<double>(); a.wye = h->wye.as<double>(); a.wrho = h->wrho.as<double>();
    a.prm = h->prm;
    // Long paths: the polished point's residuals in the transition rows add up along the path - the rows are a discrete double integrator, an error of
    // 1e-9 per row in (psi, kappa) is 1e-4 in l after 300 waypoints - so an accepted point gets one more refinement solve per pass beyond 128 waypoints, three beyond 256 (each shrinks the error ~10x: 4.6e-3 -> 4.4e-4 -> 4.1e-5 -> 3.3e-6 on
    // the worst path of 300 waypoints; the kernels of up to 128 waypoints do not compile the feature in: Ctx::kFinalRefine) (a 100x
    // tighter acceptance test instead leaves a few QPs in 30 000 unverifiable: 350-1000 solves, configs[4] halved).  Measured against the converged C oracle over 32 768 QPs per shape (profiles/r05o_*): before, 7 paths of 200 waypoints
    // and 117 of 300 were 3e-5 ... 4.6e-3 off (the lane-per-QP kernel, whose roll-out satisfies the rows exactly: 5e-6).
    // ... and the production setting's intervals by path length (pqp_defaults.hpp)
    pqp::resolve_path_params(&a.prm, n);
    int nw = 1, lg = 0;
    while (64 * nw < n) { nw *= 2; lg += 1; }           // one waypoint per lane: T = 64 * nw >= n threads per QP
    const int T_lanes = 64 * nw;
    const bool save_lds = nw <= pqp::kSaveLdsMaxNw;
    const size_t lds = (size_t)pqp::ShLayout{T_lanes}.total(save_lds, save_lds) * 8;
    // two variants of every kernel: with and without OSQP's primal infeasibility certificate (prm.eps_prim_inf > 0)
    const bool cert = h->prm.eps_prim_inf > 0.0 && h->prm.prim_inf_after <= 0;
    const void* fn = nullptr;
    switch (nw) {       // (pqp_path_solve.hip, one translation unit per width)
        case 1: fn = pqp_path_solve_fn_nw1(cert); break;
        case 2: fn = pqp_path_solve_fn_nw2(cert); break;
        case 4: fn = pqp_path_solve_fn_nw4(cert); break;
        default: fn = pqp_path_solve_fn_nw8(cert); break;
    }
    if ((rc = lds_opt_in(fn, lds, "pqp_path_solve: LDS"))) return rc;
    // persistent workgroups: as many as the chip holds at once (a surplus one would only wait for a free slot), each with its own
    // save area; they draw the QPs from the ticket counter
    int& per_cu = h->blocks_per_cu[2 * lg + (cert ? 1 : 0)];
    if (per_cu == 0) {
        PQP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * nw, lds));
        if (per_cu < 1) per_cu = 1;
    }
    const int cus = h->num_cu - h->opt_reserve_cus > 1 ? h->num_cu - h->opt_reserve_cus : 1;
    const long long resident = (long long)per_cu * cus;
    const int grid = (int)(batch < resident ? batch : resident);
    if (!save_lds) {          // more than 256 lanes per QP: the save area and the parked Ruiz vectors live in the workgroup slot's global memory
        if ((rc = h->wsave.ensure((size_t)grid * T_lanes * PQP_SAVE_STRIDE * 8))) return rc;
        if ((rc = h->wscale.ensure((size_t)grid * T_lanes * 18 * 8))) return rc;
    }
    a.wsave = h->wsave.as<double>();
    a.wscale = h->wscale.as<double>();
    a.store_warm = (h->opt_store_warm || h->opt_carry) ? 1 : 0;
    a.carry_tails = carry_tails;
    a.carry_k = h->opt_carry;
    a.ticket = h->ticket.as<unsigned long long>();
    a.ticket_base = h->ticket_next;
    // inside a captured graph the launch cannot take its ticket base from a host counter that moves between replays: the graph resets the
    // device counter itself and every replay starts at 0 (pqp_chain.inc puts the host counter where the replay leaves the device one)
    if (h->capturing) { PQP_HIP(hipMemsetAsync(h->ticket.p, 0, 8, h->stream)); a.ticket_base = 0; }
    // Host-side bookkeeping of the launch (ticket base of the next launch, launch parity, shape of the cost histogram) is committed
    // only after the launch has been accepted: a failing step below (allocation, memset, event, launch) leaves the device ticket
    // counter and the host's idea of it in step.
    if (h->opt_order_by_cost) {
        // most expensive QPs first, by what they cost in this handle's previous solve of the same shape (a planner re-solves
        // nearly the same scenarios cycle after cycle); results do not depend on the order
        if ((rc = h->cost_key.ensure((size_t)batch * 4)) || (rc = h->order.ensure((size_t)2 * batch * 4))) return rc;
        // two order arrays: the one this launch reads (written by the previous launch's last workgroup) and the one it writes
        int32_t* order_read = h->order.as<int32_t>() + (size_t)(h->solves & 1) * batch;
        int32_t* order_write = h->order.as<int32_t>() + (size_t)((h->solves + 1) & 1) * batch;
        if (h->hist_batch == batch && h->hist_n == n) a.order = order_read;
        else { h->hist_batch = 0; h->hist_n = 0; PQP_HIP(hipMemsetAsync(h->cost_hist.p, 0, (pqp::kCostBins + 1) * 4, h->stream)); }     // (a shape change: stale counts)
        a.cost_key = h->cost_key.as<int32_t>();
        a.cost_hist = h->cost_hist.as<int32_t>();
        a.order_next = order_write;
    }
    rc = h->launch_timed([&]() -> int {
        void* kargs[] = {(void*)&a};
        hipError_t le = hipLaunchKernel(fn, dim3(grid), dim3(64 * nw), kargs, lds, h->stream);
        if (le == hipSuccess) le = hipGetLastError();
        if (le != hipSuccess) {
            h->hist_batch = 0; h->hist_n = 0;          // (the histogram may have been cleared for a launch that never ran)
            return fail(PQP_ERR_HIP, std::string("hipLaunchKernel(path_solve_kernel): ") + hipGetErrorString(le));
        }
        h->ticket_next = a.ticket_base + (unsigned long long)batch + (unsigned long long)grid;
        if (h->opt_order_by_cost) { h->hist_batch = batch; h->hist_n = n; }
        h->solves += 1;
        return PQP_OK;
    });
    if (rc) return rc;
    h->warm_batch = batch; h->warm_n = n;
    h->warm_stored = h->opt_store_warm != 0 || h->opt_carry != 0;
    h->last_path_kernel = PQP_KERNEL_LANE_PER_WAYPOINT;
    return PQP_OK;
}

int pqp_path_solve_device(pqp_handle* h, int batch, int n, const double* ref, const double* lin, const double* bounds,
                          const double* scal, int passes, int warm, double* out, int32_t* status, int32_t* iters,
                          double* info) {
    return path_solve_impl(h, batch, n, nullptr, ref, lin, bounds, scal, passes, warm, out, status, iters, info);
}

int pqp_path_solve_var_device(pqp_handle* h, int batch, int n_max, const int32_t* n_of, const double* ref, const double* lin,
                              const double* bounds, const double* scal, int passes, int warm, double* out, int32_t* status,
                              int32_t* iters, double* info) {
    if (!n_of) return fail(PQP_ERR_INVALID, "pqp_path_solve_var: n_of is null");
    return path_solve_impl(h, batch, n_max, n_of, ref, lin, bounds, scal, passes, warm, out, status, iters, info);
}

static int path_solve_host(pqp_handle* h, int batch, int n, const int32_t* n_of, const double* ref, const double* lin, const double* bounds,
                           const double* scal, int passes, int warm, double* out, int32_t* status, int32_t* iters, double* info) {
    if (!path_solve_ok(h, batch, n, ref, bounds, scal, passes, out)) return fail(PQP_ERR_INVALID, "pqp_path_solve: bad argument");
    // A box with lower > upper bound: OSQP refuses such data at setup (OsqpEigen's initSolver() fails and BaseSolver::solve returns
    // false, base_solver.cpp:76-80).  The host-pointer entry points see the data anyway: such a QP is not launched (waypoint count 0)
    // and comes back PQP_STATUS_PRIMAL_INFEASIBLE.  (The device-pointer entry points do not validate: there the row would be
    // pinned to its upper bound.)
    std::vector<int32_t> counts;            // declared before the staging: outlives the copy enqueued from it
    bool any_invalid = false;
    for (int q = 0; q < batch; ++q) {
        const int cnt = n_of ? n_of[q] : n;
        bool bad = false;
        for (int i = 0; i < cnt && i < n && !bad; ++i) {
            const double* b = bounds + ((size_t)q * n + i) * PQP_BOUNDS_STRIDE;
            bad = b[0] > b[1] || b[2] > b[3] || b[4] > b[5];
        }
        if (bad && !any_invalid) {
            counts.assign(batch, n);
            if (n_of) counts.assign(n_of, n_of + batch);
            any_invalid = true;
        }
        if (bad) counts[q] = -1;
    }
    if (any_invalid) n_of = counts.data();
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const int32_t* d_n_of = st.in(n_of, batch);
    const double *d_ref = st.in(ref, bn * 5), *d_lin = st.in(lin, bn * 3), *d_bounds = st.in(bounds, bn * 6), *d_scal = st.in(scal, (size_t)batch * 6);
    double* d_out = st.out(out, bn * 7, n_of ? 0 : -1);           // (rows beyond a QP's own count are not written)
    int32_t *d_status = st.out(status, batch), *d_iters = st.out(iters, batch);
    double* d_info = st.out(info, (size_t)batch * PQP_INFO_STRIDE);
    const int rc = st.run([&]() -> int { return path_solve_impl(h, batch, n, d_n_of, d_ref, d_lin, d_bounds, d_scal, passes, warm, d_out, d_status, d_iters, d_info); });
    if (rc) return rc;
    if (any_invalid && status)
        for (int q = 0; q < batch; ++q)
            if (counts[q] < 0) status[q] = PQP_STATUS_PRIMAL_INFEASIBLE;
    return PQP_OK;
}

int pqp_path_solve(pqp_handle* h, int batch, int n, const double* ref, const double* lin, const double* bounds,
                   const double* scal, int passes, int warm, double* out, int32_t* status, int32_t* iters, double* info) {
    return path_solve_host(h, batch, n, nullptr, ref, lin, bounds, scal, passes, warm, out, status, iters, info);
}

int pqp_path_solve_var(pqp_handle* h, int batch, int n_max, const int32_t* n_of, const double* ref, const double* lin, const double* bounds,
                       const double* scal, int passes, int warm, double* out, int32_t* status, int32_t* iters, double* info) {
    if (!n_of) return fail(PQP_ERR_INVALID, "pqp_path_solve_var: n_of is null");
    return path_solve_host(h, batch, n_max, n_of, ref, lin, bounds, scal, passes, warm, out, status, iters, info);
}

int pqp_path_get_solution(pqp_handle* h, int batch, int n, int precise, double* x, double* y) {
    if (!h || batch < 1 || n < 2 || precise < 0 || precise > n) return fail(PQP_ERR_INVALID, "pqp_path_get_solution: bad argument");
    if (h->warm_batch != batch || h->warm_n != n || !h->warm_stored)
        return fail(PQP_ERR_INVALID, "pqp_path_get_solution: no solve of that shape on this handle (or PQP_OPT_STORE_WARM is off)");
    pqp::RefIndex R{n, precise};
    Staging st(h);
    double* d_x = st.out(x, (size_t)batch * R.vars(), 0);
    double* d_y = st.out(y, (size_t)batch * R.cons(), 0);
    return st.run([&]() -> int {
        const int total = batch * n;
        hipLaunchKernelGGL(pqp::path_gather_solution, dim3((total + 255) / 256), dim3(256), 0, h->stream, R, batch, h->wx.as<double>(),
                           h->wy.as<double>(), h->wye.as<double>(), x ? d_x : nullptr, y ? d_y : nullptr);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_constrain_angle_device(pqp_handle* h, int count, const double* in, double* out) {
    if (!h || !in || !out || count < 1) return fail(PQP_ERR_INVALID, "pqp_constrain_angle: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(pqp::constrain_angle_kernel, dim3((count + 255) / 256), dim3(256), 0, h->stream, count, in, out);
    PQP_HIP(hipGetLastError());
    return PQP_OK;
}

int pqp_last_path_kernel(pqp_handle* h) {
    if (!h) return fail(PQP_ERR_INVALID, "pqp_last_path_kernel: null handle");
    return h->last_path_kernel;
}

int pqp_last_kernel_ms(pqp_handle* h, float* ms) {
    if (!h || !ms) return fail(PQP_ERR_INVALID, "pqp_last_kernel_ms: null argument");
    if (!h->timed) return fail(PQP_ERR_INVALID, "pqp_last_kernel_ms: nothing was launched yet");
    PQP_HIP(hipSetDevice(h->device));
    const long long idx = (h->ev_count - 1) % pqp_handle::kEvSlots;
    PQP_HIP(hipEventSynchronize(h->evs1[idx]));
    PQP_HIP(hipEventElapsedTime(ms, h->evs0[idx], h->evs1[idx]));
    return PQP_OK;
}

int pqp_kernel_ms_history(pqp_handle* h, float* ms, int count) {
    if (!h || !ms || count < 1) return fail(PQP_ERR_INVALID, "pqp_kernel_ms_history: bad argument");
    if (count > pqp_handle::kEvRing || (long long)count > h->ev_count)
        return fail(PQP_ERR_INVALID, "pqp_kernel_ms_history: more launches asked for than the ring holds (256) or were made");
    PQP_HIP(hipSetDevice(h->device));
    PQP_HIP(hipStreamSynchronize(h->stream));
    for (int k = 0; k < count; ++k) {          // oldest of the requested launches first
        const long long idx = (h->ev_count - count + k) % pqp_handle::kEvSlots;
        PQP_HIP(hipEventElapsedTime(ms + k, h->evs0[idx], h->evs1[idx]));
    }
    return PQP_OK;
}

// ---------------------------------------------------------------------------------------------------------
// smoother QPs
// ---------------------------------------------------------------------------------------------------------
namespace {
enum { SM_TENSION2 = 0, SM_TENSION = 1, SM_POST = 2 };

struct SmShape { int nv, nc, bw, pbw, stride; };
SmShape sm_shape(int type, int n) {
    if (type == SM_TENSION2) return {4 * n - 1, 3 * (n - 1) + 2, 4, 4, 4};
    if (type == SM_TENSION) return {3 * n, 3 * n, 9, 9, 3};
    return {3 * n, 3 * n - 2, 3, 0, 3};
}

// shared sparsity of a smoother QP in the interleaved variable order: integer host logic (like pqp_path_sizes)
int sm_upload_structure(pqp_handle* h, int type, int n) {
    if (h->b_struct_type == type && h->b_struct_n == n) return PQP_OK;
    // a host -> device copy from vectors that go out of scope + a synchronise: not something a capturing stream may do.  The capture of
    // pqp_optimize_path_device is abandoned cleanly (the body fails, the call falls back to plain launches and never captures these arguments again:
    // a chain whose smoothers alternate between two structure types on the generic core uploads on every call)
    if (h->capturing) return fail(PQP_ERR_INVALID, "smoother structure upload inside a graph capture");
    const SmShape sh = sm_shape(type, n);
    std::vector<int> acol((size_t)sh.nc * pqp::kRMax, -1), trow((size_t)sh.nv * pqp::kCMax, -1), tslot((size_t)sh.nv * pqp::kCMax, 0);
    auto row = [&](int r, int c0, int c1, int c2) { int* a = &acol[(size_t)r * pqp::kRMax]; a[0] = c0; a[1] = c1; a[2] = c2; };
    if (type == SM_TENSION2) {
        for (int i = 0; i < n - 1; ++i) {
            row(i, 4 * (i + 1), 4 * i, 4 * i + 2);
            row(n - 1 + i, 4 * (i + 1) + 1, 4 * i + 1, 4 * i + 2);
            row(2 * (n - 1) + i, 4 * (i + 1) + 2, 4 * i + 2, 4 * i + 3);
        }
        row(3 * (n - 1), 0, -1, -1);
        row(3 * (n - 1) + 1, 1, -1, -1);
    } else if (type == SM_TENSION) {
        for (int i = 0; i < n; ++i) { row(i, 3 * i, 3 * i + 2, -1); row(n + i, 3 * i + 1, 3 * i + 2, -1); row(2 * n + i, 3 * i + 2, -1, -1); }
    } else {
        for (int i = 0; i < n; ++i) row(i, 3 * i, -1, -1);
        for (int i = 0; i < n - 1; ++i) { row(n + i, 3 * (i + 1), 3 * i, 3 * i + 1); row(2 * n - 1 + i, 3 * (i + 1) + 1, 3 * i + 1, 3 * i + 2); }
    }
    std::vector<int> fill(sh.nv, 0);
    for (int r = 0; r < sh.nc; ++r)
        for (int s = 0; s < pqp::kRMax; ++s) {
            const int c = acol[(size_t)r * pqp::kRMax + s];
            if (c < 0) continue;
            if (fill[c] >= pqp::kCMax) return fail(PQP_ERR_INVALID, "smoother structure: column overflow");
            trow[(size_t)c * pqp::kCMax + fill[c]] = r; tslot[(size_t)c * pqp::kCMax + fill[c]] = s; ++fill[c];
        }
    int rc;
    if ((rc = h->b_acol.ensure(acol.size() * 4)) || (rc = h->b_trow.ensure(trow.size() * 4)) || (rc = h->b_tslot.ensure(tslot.size() * 4))) return rc;
    PQP_HIP(hipMemcpyAsync(h->b_acol.p, acol.data(), acol.size() * 4, hipMemcpyHostToDevice, h->stream));
    PQP_HIP(hipMemcpyAsync(h->b_trow.p, trow.data(), trow.size() * 4, hipMemcpyHostToDevice, h->stream));
    PQP_HIP(hipMemcpyAsync(h->b_tslot.p, tslot.data(), tslot.size() * 4, hipMemcpyHostToDevice, h->stream));
    PQP_HIP(hipStreamSynchronize(h->stream));      // the vectors go out of scope
    h->b_struct_type = type; h->b_struct_n = n;
    return PQP_OK;
}

// assemble (already enqueued by the caller into b_pband ...) -> banded ADMM solve -> finish.  All device pointers.
int sm_solve(pqp_handle* h, int type, int batch, int n, int32_t* status, int32_t* iters, double* info) {
    const SmShape sh = sm_shape(type, n);
    pqp::BandedQpArgs a;
    std::memset(&a, 0, sizeof(a));
    a.batch = batch; a.nv = sh.nv; a.nc = sh.nc; a.bw = sh.bw; a.pbw = sh.pbw;
    a.pband = h->b_pband.as<double>(); a.q = h->b_q.as<double>(); a.acol = h->b_acol.as<int>(); a.aval = h->b_aval.as<double>();
    a.trow = h->b_trow.as<int>(); a.tslot = h->b_tslot.as<int>(); a.lo = h->b_lo.as<double>(); a.up = h->b_up.as<double>();
    a.x = h->b_x.as<double>(); a.y = h->b_y.as<double>(); a.status = status; a.iters = iters; a.info = info; a.prm = h->prm;
    pqp::resolve_banded_params(&a.prm);
    // the row data of A, the index lists and q staged in LDS once per QP (256-lane kernels: always - two of them still share a CU's LDS up
    // to 80 KB each; 512-lane kernels: when it fits; 1024-lane kernels: never)
    const size_t lds0 = (size_t)pqp::BqLayout{sh.nv, sh.nc, sh.bw}.total(false) * 8, lds1 = (size_t)pqp::BqLayout{sh.nv, sh.nc, sh.bw}.total(true) * 8;
    const int nbb = pqp::BqLayout{sh.nv, sh.nc, sh.bw}.nbb();
    const int threads = 64 * ((nbb + 63) / 64);        // one lane per (padded) variable
    if (threads > 1024) return fail(PQP_ERR_CAPACITY, "smoother QP has more than 1024 variables");
    const bool stage = threads <= 512 && lds1 <= kLdsPerCu;
    const size_t lds = stage ? lds1 : lds0;
    const void* fn = nullptr;
#define PQP_BQ_PICK(BB) fn = (threads <= 256 && stage) ? (const void*)pqp::banded_solve_kernel<BB, 256, true> : threads <= 512 ? (stage ? (const void*)pqp::banded_solve_kernel<BB, 512, true> : (const void*)pqp::banded_solve_kernel<BB, 512, false>) : (const void*)pqp::banded_solve_kernel<BB, 1024, false>
    switch (sh.bw) {
        case 3: PQP_BQ_PICK(3); break;
        case 4: PQP_BQ_PICK(4); break;
        case 9: PQP_BQ_PICK(9); break;
        default: return fail(PQP_ERR_INVALID, "unsupported smoother block size");
    }
#undef PQP_BQ_PICK
    const int rc = lds_opt_in(fn, lds, "smoother QP too large for one CU's LDS");
    if (rc) return rc;
    return h->launch_timed([&]() -> int {
        void* kargs[] = {(void*)&a};
        PQP_HIP(hipLaunchKernel(fn, dim3(batch), dim3(threads), kargs, lds, h->stream));
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

// does the generic banded core hold a smoother QP of this size (its vectors, factor rows and row data in one CU's LDS, one lane per padded variable)?
bool sm_generic_fits(int type, int n) {
    const SmShape sh = sm_shape(type, n);
    const pqp::BqLayout lay{sh.nv, sh.nc, sh.bw};
    return (size_t)lay.total(false) * 8 <= kLdsPerCu && 64 * ((lay.nbb() + 63) / 64) <= 1024;
}

int sm_alloc(pqp_handle* h, int type, int batch, int n) {
    const SmShape sh = sm_shape(type, n);
    int rc;
    if ((rc = h->b_pband.ensure((size_t)batch * (sh.pbw + 1) * sh.nv * 8)) || (rc = h->b_q.ensure((size_t)batch * sh.nv * 8)) ||
        (rc = h->b_aval.ensure((size_t)batch * sh.nc * pqp::kRMax * 8)) || (rc = h->b_lo.ensure((size_t)batch * sh.nc * 8)) ||
        (rc = h->b_up.ensure((size_t)batch * sh.nc * 8)) || (rc = h->b_x.ensure((size_t)batch * sh.nv * 8)) || (rc = h->b_y.ensure((size_t)batch * sh.nc * 8)))
        return rc;
    return sm_upload_structure(h, type, n);
}
}  // namespace

static bool tension2_ok(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list, const double* k_list,
                        const double* s_list, const double* out_x, const double* out_y, const double* out_s) {
    return h && x_list && y_list && angle_list && k_list && s_list && out_x && out_y && out_s && batch >= 1 && n >= 3;
}

// TensionSmoother2::osqpSmooth (tension_smoother_2.cpp:20-72), device pointers, all lists [batch][n]; n_of [batch] (device) or nullptr
static int smooth_tension2_impl(pqp_handle* h, int batch, int n, const int32_t* n_of, const double* x_list, const double* y_list,
                                const double* angle_list, const double* k_list, const double* s_list, double* out_x, double* out_y, double* out_s,
                                int32_t* status, int32_t* iters, double* info) {
    if (!tension2_ok(h, batch, n, x_list, y_list, angle_list, k_list, s_list, out_x, out_y, out_s))
        return fail(PQP_ERR_INVALID, "pqp_smooth_tension2: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    int rc;
    if (h->prm.polish != 0 || !sm_generic_fits(SM_TENSION2, n)) {
        // exact optima asked for (or more points than the generic core holds: 4 n variables on at most 1024 lanes, tension_smoother_2.cpp:20-72 has
        // no cap): the QP has equality rows only - its optimum by one Riccati sweep per scenario (tension2_exact_kernel)
        if (!status) return fail(PQP_ERR_INVALID, "pqp_smooth_tension2: status is null");
        if ((rc = h->b_pband.ensure((size_t)batch * n * 5 * 8)) || (rc = h->b_aval.ensure((size_t)batch * n * 6 * 8))) return rc;
        hipLaunchKernelGGL(pqp::tension2_stage_kernel, dim3((batch * n + 255) / 256), dim3(256), 0, h->stream, batch, n, n_of, x_list, y_list, angle_list, k_list,
                           s_list, h->b_aval.as<double>());
        PQP_HIP(hipGetLastError());
        return h->launch_timed([&]() -> int {
            hipLaunchKernelGGL(pqp::tension2_exact_kernel, dim3((batch + 63) / 64), dim3(64), 0, h->stream, batch, n, n_of, x_list, y_list,
                               h->prm.tension2_deviation_weight, h->prm.tension2_curvature_weight, h->prm.tension2_curvature_rate_weight, h->b_aval.as<double>(),
                               h->b_pband.as<double>(), out_x, out_y, out_s, status, iters, info);
            PQP_HIP(hipGetLastError());
            return PQP_OK;
        });
    }
    if ((rc = sm_alloc(h, SM_TENSION2, batch, n))) return rc;
    const int total = batch * n;
    hipLaunchKernelGGL(pqp::tension2_assemble_kernel, dim3((total + 255) / 256), dim3(256), 0, h->stream, batch, n, n_of, x_list, y_list, angle_list,
                       k_list, s_list, h->prm.tension2_deviation_weight, h->prm.tension2_curvature_weight, h->prm.tension2_curvature_rate_weight,
                       h->b_pband.as<double>(), h->b_q.as<double>(), h->b_aval.as<double>(), h->b_lo.as<double>(), h->b_up.as<double>());
    PQP_HIP(hipGetLastError());
    if ((rc = sm_solve(h, SM_TENSION2, batch, n, status, iters, info))) return rc;
    hipLaunchKernelGGL(pqp::tension_finish_kernel, dim3(batch), dim3(64), (size_t)n * 8, h->stream, batch, n, n_of, 4 * n - 1, 4, h->b_x.as<double>(), out_x, out_y, out_s);
    PQP_HIP(hipGetLastError());
    return PQP_OK;
}

int pqp_smooth_tension2_device(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list,
                               const double* k_list, const double* s_list, double* out_x, double* out_y, double* out_s, int32_t* status,
                               int32_t* iters, double* info) {
    return smooth_tension2_impl(h, batch, n, nullptr, x_list, y_list, angle_list, k_list, s_list, out_x, out_y, out_s, status, iters, info);
}

int pqp_smooth_tension2_var_device(pqp_handle* h, int batch, int n_max, const int32_t* n_of, const double* x_list, const double* y_list,
                                   const double* angle_list, const double* k_list, const double* s_list, double* out_x, double* out_y,
                                   double* out_s, int32_t* status, int32_t* iters, double* info) {
    if (!n_of) return fail(PQP_ERR_INVALID, "pqp_smooth_tension2_var: n_of is null");
    return smooth_tension2_impl(h, batch, n_max, n_of, x_list, y_list, angle_list, k_list, s_list, out_x, out_y, out_s, status, iters, info);
}

static bool tension_ok(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list, const double* clearance,
                       const double* out_x, const double* out_y, const double* out_s) {
    return h && x_list && y_list && angle_list && clearance && out_x && out_y && out_s && batch >= 1 && n >= 4;
}

// TensionSmoother::osqpSmooth (tension_smoother.cpp:49-100); clearance[batch][n] = Map::getObstacleDistance at each point; n_of [batch]
// (device) or nullptr
static int smooth_tension_impl(pqp_handle* h, int batch, int n, const int32_t* n_of, const double* x_list, const double* y_list, const double* angle_list,
                               const double* clearance, double* out_x, double* out_y, double* out_s, int32_t* status, int32_t* iters, double* info) {
    if (!tension_ok(h, batch, n, x_list, y_list, angle_list, clearance, out_x, out_y, out_s)) return fail(PQP_ERR_INVALID, "pqp_smooth_tension: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    int rc;
    // The generic block-cyclic-reduction core keeps a QP's vectors, factor rows and row data in one compute unit's LDS: in TensionSmoother's
    // 9 x 9 blocks that ends near 166 points.  The reference has no such limit (tension_smoother.cpp:49-100; segmentRawReference gives a
    // point per metre of line).  Beyond it, also a handle in the reference's ADMM setting gets the exact kernel's optimum: a point with
    // zero residuals meets OSQP's termination test at any eps, so it IS a valid result of that setting (iters = 0; OSQP itself would
    // stop at a less accurate one).
    const bool generic_fits = sm_generic_fits(SM_TENSION, n);
    if (h->prm.polish == 1 || !generic_fits) {
        // exact optima asked for (or the only kernel that holds the QP): the box QP in the lateral shifts alone, one wavefront per scenario (tension_exact_kernel)
        if (!status) return fail(PQP_ERR_INVALID, "pqp_smooth_tension: status is null");
        const double wk = h->prm.cartesian_curvature_weight, wdk = h->prm.cartesian_curvature_rate_weight, wdev = h->prm.cartesian_deviation_weight, tol = h->prm.polish_tol;
        signed char* act_io;
        int carry;
        if ((rc = sm_carry_slot(h, 0, batch, n, act_io, carry))) return rc;
        // (any line longer than 1024 points - the reference has no cap: tension_smoother.cpp:49-100 - runs with its arrays in HBM)
        return sm_exact_launch(h, batch, n, pqp::kTensionExactArrays, [&](auto K, double* ws) {
            hipLaunchKernelGGL(pqp::tension_exact_kernel<K>, dim3(batch), dim3(64), 0, h->stream, batch, n, n_of, x_list, y_list, angle_list, clearance, wk, wdk,
                               wdev, tol, out_x, out_y, out_s, status, iters, info, act_io, carry, ws);
        });
    }
    if ((rc = sm_alloc(h, SM_TENSION, batch, n))) return rc;
    const int total = batch * n;
    hipLaunchKernelGGL(pqp::tension_assemble_kernel, dim3((total + 255) / 256), dim3(256), 0, h->stream, batch, n, n_of, x_list, y_list, angle_list, clearance,
                       h->prm.cartesian_curvature_weight, h->prm.cartesian_curvature_rate_weight, h->prm.cartesian_deviation_weight,
                       h->b_pband.as<double>(), h->b_q.as<double>(), h->b_aval.as<double>(), h->b_lo.as<double>(), h->b_up.as<double>());
    PQP_HIP(hipGetLastError());
    if ((rc = sm_solve(h, SM_TENSION, batch, n, status, iters, info))) return rc;
    hipLaunchKernelGGL(pqp::tension_finish_kernel, dim3(batch), dim3(64), (size_t)n * 8, h->stream, batch, n, n_of, 3 * n, 3, h->b_x.as<double>(), out_x, out_y, out_s);
    PQP_HIP(hipGetLastError());
    return PQP_OK;
}

int pqp_smooth_tension_device(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list,
                              const double* clearance, double* out_x, double* out_y, double* out_s, int32_t* status, int32_t* iters, double* info) {
    return smooth_tension_impl(h, batch, n, nullptr, x_list, y_list, angle_list, clearance, out_x, out_y, out_s, status, iters, info);
}

int pqp_smooth_tension_var_device(pqp_handle* h, int batch, int n_max, const int32_t* n_of, const double* x_list, const double* y_list,
                                  const double* angle_list, const double* clearance, double* out_x, double* out_y, double* out_s, int32_t* status,
                                  int32_t* iters, double* info) {
    if (!n_of) return fail(PQP_ERR_INVALID, "pqp_smooth_tension_var: n_of is null");
    return smooth_tension_impl(h, batch, n_max, n_of, x_list, y_list, angle_list, clearance, out_x, out_y, out_s, status, iters, info);
}

static bool post_smooth_ok(pqp_handle* h, int batch, int m, const double* layers_s, const double* lb, const double* ub, const double* vehicle_l,
                           const double* out_l) {
    return h && layers_s && lb && ub && vehicle_l && out_l && batch >= 1 && m >= 4;
}

// ReferencePathSmoother::postSmooth QP (reference_path_smoother.cpp:526-558): out_l[batch][m] = the lateral offsets l_i
static int post_smooth_impl(pqp_handle* h, int batch, int m, const int32_t* m_of, const double* layers_s, const double* lb, const double* ub,
                            const double* vehicle_l, double* out_l, int32_t* status, int32_t* iters, double* info) {
    if (!post_smooth_ok(h, batch, m, layers_s, lb, ub, vehicle_l, out_l)) return fail(PQP_ERR_INVALID, "pqp_post_smooth: bad argument (m >= 4, reference_path_smoother.cpp:528)");
    PQP_HIP(hipSetDevice(h->device));
    int rc;
    // (beyond what the generic core holds in a CU's LDS also a handle in the reference's ADMM setting gets the exact kernel's optimum, as in smooth_tension_impl)
    if (h->prm.polish == 1 || !sm_generic_fits(SM_POST, m)) {
        // exact optima asked for: the box QP in the offsets alone, one wavefront per scenario (post_exact_kernel)
        if (!status) return fail(PQP_ERR_INVALID, "pqp_post_smooth: status is null");
        const double tol = h->prm.polish_tol;
        signed char* act_io;
        int carry;
        if ((rc = sm_carry_slot(h, 1, batch, m, act_io, carry))) return rc;
        // (any corridor longer than 1024 layers - reference_path_smoother.cpp:526-580 has no cap - runs with its arrays in HBM)
        return sm_exact_launch(h, batch, m, pqp::kPostExactArrays, [&](auto K, double* ws) {
            hipLaunchKernelGGL(pqp::post_exact_kernel<K>, dim3(batch), dim3(64), 0, h->stream, batch, m, m_of, layers_s, lb, ub, vehicle_l, tol, out_l, status,
                               iters, info, act_io, carry, ws);
        });
    }
    if ((rc = sm_alloc(h, SM_POST, batch, m))) return rc;
    const int total = batch * m;
    hipLaunchKernelGGL(pqp::post_assemble_kernel, dim3((total + 255) / 256), dim3(256), 0, h->stream, batch, m, m_of, layers_s, lb, ub, vehicle_l,
                       h->b_pband.as<double>(), h->b_q.as<double>(), h->b_aval.as<double>(), h->b_lo.as<double>(), h->b_up.as<double>());
    PQP_HIP(hipGetLastError());
    if ((rc = sm_solve(h, SM_POST, batch, m, status, iters, info))) return rc;
    hipLaunchKernelGGL(pqp::post_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, h->stream, batch, m, h->b_x.as<double>(), out_l);
    PQP_HIP(hipGetLastError());
    return PQP_OK;
}

int pqp_post_smooth_device(pqp_handle* h, int batch, int m, const double* layers_s, const double* lb, const double* ub, const double* vehicle_l,
                           double* out_l, int32_t* status, int32_t* iters, double* info) {
    return post_smooth_impl(h, batch, m, nullptr, layers_s, lb, ub, vehicle_l, out_l, status, iters, info);
}

int pqp_post_smooth_var_device(pqp_handle* h, int batch, int m_max, const int32_t* m_of, const double* layers_s, const double* lb, const double* ub,
                               const double* vehicle_l, double* out_l, int32_t* status, int32_t* iters, double* info) {
    if (!m_of) return fail(PQP_ERR_INVALID, "pqp_post_smooth_var: m_of is null");
    return post_smooth_impl(h, batch, m_max, m_of, layers_s, lb, ub, vehicle_l, out_l, status, iters, info);
}

int pqp_smooth_tension2(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list, const double* k_list,
                        const double* s_list, double* out_x, double* out_y, double* out_s, int32_t* status, int32_t* iters) {
    if (!tension2_ok(h, batch, n, x_list, y_list, angle_list, k_list, s_list, out_x, out_y, out_s)) return fail(PQP_ERR_INVALID, "pqp_smooth_tension2: bad argument");
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double *d_x = st.in(x_list, bn), *d_y = st.in(y_list, bn), *d_angle = st.in(angle_list, bn), *d_k = st.in(k_list, bn), *d_s = st.in(s_list, bn);
    double *o_x = st.out(out_x, bn), *o_y = st.out(out_y, bn), *o_s = st.out(out_s, bn);
    int32_t *d_status = st.out(status, batch), *d_iters = st.out(iters, batch);
    return st.run([&]() -> int { return pqp_smooth_tension2_device(h, batch, n, d_x, d_y, d_angle, d_k, d_s, o_x, o_y, o_s, d_status, d_iters, nullptr); });
}

int pqp_smooth_tension(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list, const double* clearance,
                       double* out_x, double* out_y, double* out_s, int32_t* status, int32_t* iters) {
    if (!tension_ok(h, batch, n, x_list, y_list, angle_list, clearance, out_x, out_y, out_s)) return fail(PQP_ERR_INVALID, "pqp_smooth_tension: bad argument");
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double *d_x = st.in(x_list, bn), *d_y = st.in(y_list, bn), *d_angle = st.in(angle_list, bn), *d_clr = st.in(clearance, bn);
    double *o_x = st.out(out_x, bn), *o_y = st.out(out_y, bn), *o_s = st.out(out_s, bn);
    int32_t *d_status = st.out(status, batch), *d_iters = st.out(iters, batch);
    return st.run([&]() -> int { return pqp_smooth_tension_device(h, batch, n, d_x, d_y, d_angle, d_clr, o_x, o_y, o_s, d_status, d_iters, nullptr); });
}

int pqp_post_smooth(pqp_handle* h, int batch, int m, const double* layers_s, const double* lb, const double* ub, const double* vehicle_l, double* out_l,
                    int32_t* status, int32_t* iters) {
    if (!post_smooth_ok(h, batch, m, layers_s, lb, ub, vehicle_l, out_l)) return fail(PQP_ERR_INVALID, "pqp_post_smooth: bad argument");
    const size_t bm = (size_t)batch * m;
    Staging st(h);
    const double *d_s = st.in(layers_s, bm), *d_lb = st.in(lb, bm), *d_ub = st.in(ub, bm), *d_vl = st.in(vehicle_l, batch);
    double* o_l = st.out(out_l, bm);
    int32_t *d_status = st.out(status, batch), *d_iters = st.out(iters, batch);
    return st.run([&]() -> int { return pqp_post_smooth_device(h, batch, m, d_s, d_lb, d_ub, d_vl, o_l, d_status, d_iters, nullptr); });
}

// ---- corridor bounds from the distance map -----------------------------------------------------------
void pqp_corridor_default_params(pqp_corridor_params* p) {
    if (!p) return;
    p->front_length = 3.9; p->rear_length = -1.0;       // planning_flags.cpp:20,18
    p->car_width = 2.0; p->safety_margin = 0.3;         // planning_flags.cpp:10,14
    p->epsilon = 1e-6;                                  // planning_flags.cpp:108
    p->search_radius = 0.5; p->delta_s = 0.3; p->smaller_ds = 0.05; p->search_range = 6.0; p->min_space = 0.2;   // reference_path_impl.cpp:238-304
    p->projection_window = 5.0;                         // reference_path_impl.cpp:194
}

// a distance-map layer the kernels can index with 32 bits (pqp_corridor_kernels.inc: obstacle_distance)
static bool geometry_ok(const pqp_grid_geometry* g) {
    return g && g->rows >= 2 && g->cols >= 2 && g->resolution > 0.0 && (long long)g->rows * g->cols < (1ll << 30);
}

static bool corridor_ok(pqp_handle* h, int batch, int n, int m, const double* ref, const double* spline, const double* spline_ext, const float* dist,
                        const pqp_grid_geometry* geom, const pqp_corridor_params* prm, const double* bounds, const int32_t* n_valid) {
    return h && ref && spline && spline_ext && dist && prm && bounds && n_valid && batch >= 1 && n >= 1 && m >= 3 && geometry_ok(geom) &&
           prm->delta_s > 0.0 && prm->smaller_ds > 0.0;
}

// the waypoints kernel `fn` (corridor_bounds_kernel / states_bounds_kernel) holds in LDS at a time: a whole scenario's probes when they fit
// (9 m + 33 n doubles), tiles of waypoints otherwise: any path length.  Sets *lds to the dynamic LDS of that tile and opts in to it.
static int corridor_tile(const void* fn, int m, int n, int* tile, size_t* lds, const char* who) {
    *tile = n;
    size_t fixed = 0;
    if (const int rc = static_lds(fn, &fixed)) return rc;
    if (pqp::CorridorLds{m, n}.total_bytes() > kLdsPerCu - fixed) {
        const long long room = (long long)(kLdsPerCu - fixed) - (long long)pqp::CorridorLds{m, 0}.total_bytes(), per_waypoint = (long long)(pqp::CorridorLds{m, 1}.total_bytes() - pqp::CorridorLds{m, 0}.total_bytes());
        if (room < 16 * per_waypoint) return fail(PQP_ERR_CAPACITY, std::string(who) + ": the line's spline table (9 m doubles) does not leave room for the probes in one CU's LDS");
        *tile = (int)(room / per_waypoint);
    }
    *lds = pqp::CorridorLds{m, *tile}.total_bytes();
    return lds_opt_in(fn, *lds, (std::string(who) + ": scenario too large for one CU's LDS (about 9 m + 31 n doubles)").c_str());
}

// PQP_OPT_LONG_LINES on a corridor launch: the long kernel `long_fn` (the table in HBM, tiles of probes in LDS) where `fn` would refuse
// the line's table (1) or always (2); *fn_out and the tile / LDS of the launch accordingly
static int corridor_pick(int opt, const void* fn, const void* long_fn, int m, int n, const void** fn_out, int* tile, size_t* lds, const char* who) {
    // (what corridor_tile refuses: the table and the fewest probes `fn` runs on, a tile of 16 waypoints or all n, exceed one CU's LDS)
    bool go_long = false;
    if (const int rc = long_form(opt, fn, pqp::CorridorLds{m, n < 16 ? n : 16}.total_bytes(), &go_long)) return rc;
    *fn_out = go_long ? long_fn : fn;
    return corridor_tile(*fn_out, go_long ? 0 : m, n, tile, lds, who);
}

// the sample loops are strided; 512 lanes per scenario keep the most gathers in flight per CU (measured at batch 1024 x n = 80: 1024 lanes
// 142 us - two scenarios per CU -, 512: 121, 256: 120, 128: 146)
constexpr int kCorridorThreads = 512;

int pqp_corridor_bounds_device(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* spline,
                               const double* spline_ext, const float* dist, const int32_t* map_of, const pqp_grid_geometry* geom,
                               const pqp_corridor_params* prm, double* bounds, int32_t* n_valid) {
    if (!corridor_ok(h, batch, n, m, ref, spline, spline_ext, dist, geom, prm, bounds, n_valid))
        return fail(PQP_ERR_INVALID, "pqp_corridor_bounds: bad argument (m >= 3 knots: spline.cpp:164; a map layer of 2 x 2 to 2^30 cells)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::CorridorArgs a;
    a.batch = batch; a.n = n; a.m = m; a.ref = ref; a.spl = spline; a.spl_ext = spline_ext; a.dist = dist; a.map_of = map_of; a.n_of = n_of;
    a.g = *geom; a.p = *prm; a.bounds = bounds; a.n_valid = n_valid;
    size_t lds = 0;
    const void* fn = nullptr;
    if (const int rc = corridor_pick(h->opt_long_lines, (const void*)pqp::corridor_bounds_kernel, (const void*)pqp::long_corridor_kernel, m, n, &fn, &a.tile, &lds,
                                     "pqp_corridor_bounds")) return rc;
    return h->launch_timed([&]() -> int {
        if (fn == (const void*)pqp::long_corridor_kernel) hipLaunchKernelGGL(pqp::long_corridor_kernel, dim3(batch), dim3(kCorridorThreads), lds, h->stream, a);
        else hipLaunchKernelGGL(pqp::corridor_bounds_kernel, dim3(batch), dim3(kCorridorThreads), lds, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_corridor_bounds(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* spline,
                        const double* spline_ext, const float* dist, int n_maps, const int32_t* map_of, const pqp_grid_geometry* geom,
                        const pqp_corridor_params* prm, double* bounds, int32_t* n_valid) {
    if (!corridor_ok(h, batch, n, m, ref, spline, spline_ext, dist, geom, prm, bounds, n_valid) || n_maps < 1)
        return fail(PQP_ERR_INVALID, "pqp_corridor_bounds: bad argument");
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_ref = st.in(ref, bn * PQP_REF_STRIDE);
    const int32_t* d_n_of = st.in(n_of, batch);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4);
    const float* d_dist = st.in(dist, (size_t)n_maps * geom->rows * geom->cols);
    const int32_t* d_map_of = st.in(map_of, batch);
    double* d_bounds = st.out(bounds, bn * PQP_BOUNDS_STRIDE);
    int32_t* d_n_valid = st.out(n_valid, batch);
    return st.run([&]() -> int { return pqp_corridor_bounds_device(h, batch, n, m, d_ref, d_n_of, d_spl, d_ext, d_dist, d_map_of, geom, prm, d_bounds, d_n_valid); });
}

// ---- corridor bounds on the states of a solved path (ReferencePathImpl::updateBoundsOnInputStates) ----------------------------------
static bool corridor_states_ok(pqp_handle* h, int batch, int n, int m, const double* ref, const double* states, int stride, const double* spline,
                               const double* spline_ext, const float* dist, const pqp_grid_geometry* geom, const pqp_corridor_params* prm,
                               const double* bounds, const int32_t* n_valid) {
    return corridor_ok(h, batch, n, m, ref, spline, spline_ext, dist, geom, prm, bounds, n_valid) && states && stride >= 5;
}

int pqp_corridor_bounds_on_states_device(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* states,
                                         int stride, const double* spline, const double* spline_ext, const float* dist, const int32_t* map_of,
                                         const pqp_grid_geometry* geom, const pqp_corridor_params* prm, double* bounds, int32_t* n_valid) {
    if (!corridor_states_ok(h, batch, n, m, ref, states, stride, spline, spline_ext, dist, geom, prm, bounds, n_valid))
        return fail(PQP_ERR_INVALID, "pqp_corridor_bounds_on_states: bad argument (stride >= 5; m >= 3 knots; a map layer of 2 x 2 to 2^30 cells)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::CorridorArgs a;
    a.batch = batch; a.n = n; a.m = m; a.ref = ref; a.spl = spline; a.spl_ext = spline_ext; a.dist = dist; a.map_of = map_of; a.n_of = n_of;
    a.g = *geom; a.p = *prm; a.bounds = bounds; a.n_valid = n_valid;
    size_t lds = 0;
    const void* fn = nullptr;
    if (const int rc = corridor_pick(h->opt_long_lines, (const void*)pqp::states_bounds_kernel, (const void*)pqp::long_states_kernel, m, n, &fn, &a.tile, &lds,
                                     "pqp_corridor_bounds_on_states")) return rc;
    return h->launch_timed([&]() -> int {
        if (fn == (const void*)pqp::long_states_kernel) hipLaunchKernelGGL(pqp::long_states_kernel, dim3(batch), dim3(kCorridorThreads), lds, h->stream, a, states, stride);
        else hipLaunchKernelGGL(pqp::states_bounds_kernel, dim3(batch), dim3(kCorridorThreads), lds, h->stream, a, states, stride);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_corridor_bounds_on_states(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* states, int stride,
                                  const double* spline, const double* spline_ext, const float* dist, int n_maps, const int32_t* map_of,
                                  const pqp_grid_geometry* geom, const pqp_corridor_params* prm, double* bounds, int32_t* n_valid) {
    if (!corridor_states_ok(h, batch, n, m, ref, states, stride, spline, spline_ext, dist, geom, prm, bounds, n_valid) || n_maps < 1)
        return fail(PQP_ERR_INVALID, "pqp_corridor_bounds_on_states: bad argument");
    if (map_of)
        for (int b = 0; b < batch; ++b)
            if (map_of[b] < 0 || map_of[b] >= n_maps) return fail(PQP_ERR_INVALID, "pqp_corridor_bounds_on_states: map_of outside [0, n_maps)");
    if (n_of)       // CHECK_LE(input_sl_states.size(), reference_states_.size()) (reference_path_impl.cpp:119)
        for (int b = 0; b < batch; ++b)
            if (n_of[b] < 0 || n_of[b] > n) return fail(PQP_ERR_INVALID, "pqp_corridor_bounds_on_states: n_of outside [0, n] (more states than reference states)");
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_ref = st.in(ref, bn * PQP_REF_STRIDE);
    const int32_t* d_n_of = st.in(n_of, batch);
    const double* d_states = st.in(states, bn * stride);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4);
    const float* d_dist = st.in(dist, (size_t)n_maps * geom->rows * geom->cols);
    const int32_t* d_map_of = st.in(map_of, batch);
    double* d_bounds = st.out(bounds, bn * PQP_BOUNDS_STRIDE, n_of ? 0 : -1);      // (rows beyond a scenario's states are not written)
    int32_t* d_n_valid = st.out(n_valid, batch);
    return st.run([&]() -> int {
        return pqp_corridor_bounds_on_states_device(h, batch, n, m, d_ref, d_n_of, d_states, stride, d_spl, d_ext, d_dist, d_map_of, geom, prm, d_bounds, d_n_valid);
    });
}

// ---- the obstacle distance layer from an occupancy grid (src/test/demo.cpp:104-113) ------------------------------------------------
static bool distance_layer_ok(pqp_handle* h, int n_maps, const pqp_grid_geometry* geom, const uint8_t* grid, const float* dist) {
    return h && grid && dist && n_maps >= 1 && geometry_ok(geom);
}

int pqp_distance_layer_device(pqp_handle* h, int n_maps, const pqp_grid_geometry* geom, const uint8_t* grid, float* dist) {
    if (!distance_layer_ok(h, n_maps, geom, grid, dist))
        return fail(PQP_ERR_INVALID, "pqp_distance_layer: bad argument (n_maps >= 1; a map of 2 x 2 to 2^30 cells, resolution > 0)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::DistanceArgs a;
    a.grid = grid; a.out = reinterpret_cast<int32_t*>(dist); a.n_maps = n_maps; a.rows = geom->rows; a.cols = geom->cols;
    const pqp::edt::Shape sh = pqp::edt::shape_of(geom->rows, geom->cols);
    a.site_bits = sh.site_bits; a.empty_d2 = sh.empty_d2; a.res = (float)geom->resolution;
    const long long lines = (long long)n_maps * geom->cols, lanes = (long long)n_maps * geom->rows;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::distance_lines_kernel, dim3((unsigned)std::min((lines + 3) / 4, 1ll << 20)), dim3(256), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        const unsigned blocks = (unsigned)std::min((lanes + 63) / 64, 1ll << 20);
        if (sh.wide) hipLaunchKernelGGL(pqp::distance_envelope_kernel<int64_t>, dim3(blocks), dim3(64), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::distance_envelope_kernel<int32_t>, dim3(blocks), dim3(64), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_distance_layer(pqp_handle* h, int n_maps, const pqp_grid_geometry* geom, const uint8_t* grid, float* dist) {
    if (!distance_layer_ok(h, n_maps, geom, grid, dist))
        return fail(PQP_ERR_INVALID, "pqp_distance_layer: bad argument (n_maps >= 1; a map of 2 x 2 to 2^30 cells, resolution > 0)");
    const size_t cells = (size_t)n_maps * geom->rows * geom->cols;
    Staging st(h);
    const uint8_t* d_grid = st.in(grid, cells);
    float* d_dist = st.out(dist, cells);
    return st.run([&]() -> int { return pqp_distance_layer_device(h, n_maps, geom, d_grid, d_dist); });
}

// ---- vehicle footprints against the distance layer (collision_checker.cpp:17-58, car_geometry.cpp:38-72) ----------------------------
void pqp_car_default_geometry(pqp_car_geometry* c) {
    if (!c) return;
    c->width = 2.0;                 // planning_flags.cpp:10
    c->rear_length = -1.0;          // :18
    c->front_length = 3.9;          // :20
}

static bool car_ok(const pqp_car_geometry* c) {
    return c && std::isfinite(c->width) && std::isfinite(c->rear_length) && std::isfinite(c->front_length);
}

int pqp_car_circles(const pqp_car_geometry* c, double* circles) {
    if (!car_ok(c) || !circles) return fail(PQP_ERR_INVALID, "pqp_car_circles: bad argument (a finite car geometry)");
    // CollisionChecker's car_(FLAGS_car_width, fabs(FLAGS_rear_length), FLAGS_front_length) -> CarGeometry(width, back_length, front_length)
    const double width = c->width, back_length = std::fabs(c->rear_length), front_length = c->front_length;
    const double length = front_length + back_length;
    const double fl_x = front_length, fl_y = width / 2.0, fr_x = front_length, fr_y = -width / 2.0;
    const double rl_x = -back_length, rl_y = width / 2.0, rr_x = -back_length, rr_y = -width / 2.0;
    // CarGeometry::setCircles, car_geometry.cpp:38-57, term by term
    const double bounding_x = (front_length - back_length) / 2.0;
    const double bounding_r = std::sqrt(std::pow(length / 2, 2) + std::pow(width / 2, 2));
    const double small_circle_shift = width / 4.0;
    const double small_circle_radius = std::sqrt(2 * std::pow(small_circle_shift, 2));
    const double large_circle_radius = std::sqrt(std::pow(width, 2) + std::pow((length - width) / 2.0, 2)) / 2;
    const double v[7][3] = {{rr_x + small_circle_shift, rr_y + small_circle_shift, small_circle_radius},
                            {rl_x + small_circle_shift, rl_y - small_circle_shift, small_circle_radius},
                            {fr_x - small_circle_shift, fr_y + small_circle_shift, small_circle_radius},
                            {fl_x - small_circle_shift, fl_y - small_circle_shift, small_circle_radius},
                            {bounding_x + (length - width) / 4, 0, large_circle_radius},
                            {bounding_x - (length - width) / 4, 0, large_circle_radius},
                            {bounding_x, 0, bounding_r}};
    std::memcpy(circles, v, sizeof(v));
    return PQP_OK;
}

static bool footprint_ok(pqp_handle* h, int batch, int n, int stride, const double* states, const float* dist, const pqp_grid_geometry* geom,
                         const pqp_car_geometry* car, int mode, const uint8_t* free_out, const int32_t* first_collision) {
    return h && states && dist && free_out && first_collision && batch >= 1 && n >= 1 && n <= (1 << 30) && stride >= 3 && geometry_ok(geom) &&
           car_ok(car) && (mode == PQP_FOOTPRINT_CIRCLES || mode == PQP_FOOTPRINT_BOUNDING_FIRST);
}

int pqp_footprint_check_device(pqp_handle* h, int batch, int n, int stride, const double* states, const int32_t* n_of, const float* dist,
                               const int32_t* map_of, const pqp_grid_geometry* geom, const pqp_car_geometry* car, int mode, uint8_t* free_out,
                               int32_t* first_collision, double* margin) {
    if (!footprint_ok(h, batch, n, stride, states, dist, geom, car, mode, free_out, first_collision))
        return fail(PQP_ERR_INVALID, "pqp_footprint_check: bad argument (stride >= 3; a finite car geometry; mode CIRCLES or BOUNDING_FIRST; "
                                     "a map layer of 2 x 2 to 2^30 cells)");
    PQP_HIP(hipSetDevice(h->device));
    double circles[7][3];
    int rc;
    if ((rc = pqp_car_circles(car, &circles[0][0]))) return rc;
    pqp::FootprintArgs a;
    a.batch = batch; a.n = n; a.stride = stride; a.states = states; a.n_of = n_of; a.dist = dist; a.map_of = map_of; a.g = *geom;
    for (int k = 0; k < 7; ++k) { a.cx[k] = circles[k][0]; a.cy[k] = circles[k][1]; a.cr[k] = circles[k][2]; }
    a.free_out = free_out; a.first_collision = first_collision; a.margin = margin;
    return h->launch_timed([&]() -> int {
        if (mode == PQP_FOOTPRINT_CIRCLES)
            hipLaunchKernelGGL(pqp::footprint_check_kernel<PQP_FOOTPRINT_CIRCLES>, dim3(batch), dim3(pqp::kFootprintThreads), 0, h->stream, a);
        else
            hipLaunchKernelGGL(pqp::footprint_check_kernel<PQP_FOOTPRINT_BOUNDING_FIRST>, dim3(batch), dim3(pqp::kFootprintThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_footprint_check(pqp_handle* h, int batch, int n, int stride, const double* states, const int32_t* n_of, const float* dist, int n_maps,
                        const int32_t* map_of, const pqp_grid_geometry* geom, const pqp_car_geometry* car, int mode, uint8_t* free_out,
                        int32_t* first_collision, double* margin) {
    if (!footprint_ok(h, batch, n, stride, states, dist, geom, car, mode, free_out, first_collision) || n_maps < 1)
        return fail(PQP_ERR_INVALID, "pqp_footprint_check: bad argument");
    if (map_of)
        for (int b = 0; b < batch; ++b)
            if (map_of[b] < 0 || map_of[b] >= n_maps) return fail(PQP_ERR_INVALID, "pqp_footprint_check: map_of outside [0, n_maps)");
    const size_t bn = (size_t)batch * n;
    Staging st(h);
    const double* d_states = st.in(states, bn * stride);
    const int32_t* d_n_of = st.in(n_of, batch);
    const float* d_dist = st.in(dist, (size_t)n_maps * geom->rows * geom->cols);
    const int32_t* d_map_of = st.in(map_of, batch);
    uint8_t* d_free = st.out(free_out, bn);
    int32_t* d_first = st.out(first_collision, batch);
    double* d_margin = margin ? st.out(margin, bn) : nullptr;
    return st.run([&]() -> int {
        return pqp_footprint_check_device(h, batch, n, stride, d_states, d_n_of, d_dist, d_map_of, geom, car, mode, d_free, d_first, d_margin);
    });
}

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
    constexpr int per_block = pqp::kSelectThreads / 64;
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::path_score_kernel, dim3((unsigned)((batch + per_block - 1) / per_block)), dim3(pqp::kSelectThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        if (groups > 0) {
            hipLaunchKernelGGL(pqp::group_select_kernel, dim3((unsigned)((groups + per_block - 1) / per_block)), dim3(pqp::kSelectThreads), 0, h->stream, a);
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
    if (group_start[0] != 0 || group_start[groups] != batch) return fail(PQP_ERR_INVALID, "pqp_select_paths: group_start must run from 0 to batch");
    for (int g = 0; g < groups; ++g)
        if (group_start[g + 1] < group_start[g]) return fail(PQP_ERR_INVALID, "pqp_select_paths: group_start must be ascending");
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

// ---- points onto their reference line: Cartesian to Frenet (getProjection + global2Local, tools.cpp:57-126) -------------------------------
static const char* const kProjectBad =
    "pqp_project_points: bad argument (batch >= 1, m >= 2, 1 <= q_max <= 256 * 65535, stride >= 2, stride >= 3 with has_heading)";

static bool project_ok(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length, int q_max, int stride,
                       int has_heading, const double* points, const double* proj, const int32_t* flags) {
    return h && spline && spline_ext && length && points && proj && flags && batch >= 1 && m >= 2 && q_max >= 1 &&
           q_max <= pqp::kProjectThreads * 65535 && stride >= (has_heading ? 3 : 2);
}

int pqp_project_points_device(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length, int q_max,
                              int stride, int has_heading, const double* points, const int32_t* q_of, double* proj, int32_t* flags) {
    if (!project_ok(h, batch, m, spline, spline_ext, length, q_max, stride, has_heading, points, proj, flags)) return fail(PQP_ERR_INVALID, kProjectBad);
    PQP_HIP(hipSetDevice(h->device));
    pqp::ProjectArgs a;
    a.batch = batch; a.m = m; a.q_max = q_max; a.stride = stride; a.has_heading = has_heading ? 1 : 0; a.spl = spline; a.spl_ext = spline_ext;
    a.length = length; a.points = points; a.q_of = q_of; a.proj = proj; a.flags = flags;
    const dim3 grid((unsigned)batch, (unsigned)((q_max + pqp::kProjectThreads - 1) / pqp::kProjectThreads));
    return h->launch_timed([&]() -> int {
        hipLaunchKernelGGL(pqp::project_points_kernel, grid, dim3(pqp::kProjectThreads), 0, h->stream, a);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

int pqp_project_points(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length, int q_max,
                       int stride, int has_heading, const double* points, const int32_t* q_of, double* proj, int32_t* flags) {
    if (!project_ok(h, batch, m, spline, spline_ext, length, q_max, stride, has_heading, points, proj, flags)) return fail(PQP_ERR_INVALID, kProjectBad);
    const size_t rows = (size_t)batch * q_max;
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4), *d_length = st.in(length, batch);
    const double* d_points = st.in(points, rows * stride);
    const int32_t* d_q_of = st.in(q_of, batch);
    double* d_proj = st.out(proj, rows * PQP_PROJ_STRIDE);
    int32_t* d_flags = st.out(flags, rows);
    return st.run([&]() -> int {
        return pqp_project_points_device(h, batch, m, d_spl, d_ext, d_length, q_max, stride, has_heading, d_points, d_q_of, d_proj, d_flags);
    });
}

// ---- reference states + initial error ----------------------------------------------------------------
static bool reference_states_ok(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext, const double* max_s,
                                const double* start, double ds_small, double ds_large, const double* ref, const int32_t* count, const double* init_err) {
    return h && spline && spline_ext && max_s && ref && count && batch >= 1 && n_max >= 1 && m >= 3 && ds_small > 0.0 && ds_large >= ds_small &&
           (!init_err || start);
}

int pqp_reference_states_device(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext,
                                const double* max_s, const double* start, double ds_small, double ds_large, int dynamic, double* ref,
                                int32_t* count, double* init_err) {
    if (!reference_states_ok(h, batch, n_max, m, spline, spline_ext, max_s, start, ds_small, ds_large, ref, count, init_err))
        return fail(PQP_ERR_INVALID, "pqp_reference_states: bad argument (0 < ds_small <= ds_large: reference_path_impl.cpp:315)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::RefStatesArgs a;
    a.batch = batch; a.n_max = n_max; a.m = m; a.spl = spline; a.spl_ext = spline_ext; a.max_s = max_s; a.start = start;
    a.ds_small = ds_small; a.ds_large = ds_large; a.dynamic = dynamic ? 1 : 0; a.ref = ref; a.count = count; a.init_err = init_err;
    a.lx = a.ly = a.ls = a.langle = a.lk = nullptr;
    const size_t lds = ((size_t)9 * m + n_max) * 8;
    return line_launch(h, (const void*)pqp::reference_states_kernel, lds, "pqp_reference_states: 9 m + n_max doubles exceed one CU's LDS", 0,
                       [&](auto go_long, double*) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_ref_states_kernel, dim3(batch), dim3(64), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::reference_states_kernel, dim3(batch), dim3(64), lds, h->stream, a);
    });
}

// ---- raw reference line -> the smoother QPs' input lists (ReferencePathSmoother::segmentRawReference) ------------------------------
static bool segment_ok(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext, const double* max_s, double delta_s,
                       const double* x, const double* y, const double* s, const double* angle, const double* k, const int32_t* count) {
    return h && spline && spline_ext && max_s && x && y && s && angle && k && count && batch >= 1 && n_max >= 1 && m >= 3 && delta_s > 0.0;
}

int pqp_segment_raw_reference_device(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext,
                                     const double* max_s, double delta_s, double* x, double* y, double* s, double* angle, double* k,
                                     int32_t* count) {
    if (!segment_ok(h, batch, n_max, m, spline, spline_ext, max_s, delta_s, x, y, s, angle, k, count))
        return fail(PQP_ERR_INVALID, "pqp_segment_raw_reference: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    pqp::RefStatesArgs a;
    a.batch = batch; a.n_max = n_max; a.m = m; a.spl = spline; a.spl_ext = spline_ext; a.max_s = max_s; a.start = nullptr;
    a.ds_small = delta_s; a.ds_large = delta_s; a.dynamic = 2; a.ref = nullptr; a.count = count; a.init_err = nullptr;
    a.lx = x; a.ly = y; a.ls = s; a.langle = angle; a.lk = k;
    const size_t lds = ((size_t)9 * m + n_max) * 8;
    return line_launch(h, (const void*)pqp::reference_states_kernel, lds, "pqp_segment_raw_reference: 9 m + n_max doubles exceed one CU's LDS", 0,
                       [&](auto go_long, double*) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_ref_states_kernel, dim3(batch), dim3(64), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::reference_states_kernel, dim3(batch), dim3(64), lds, h->stream, a);
    });
}

int pqp_segment_raw_reference(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext, const double* max_s,
                              double delta_s, double* x, double* y, double* s, double* angle, double* k, int32_t* count) {
    if (!segment_ok(h, batch, n_max, m, spline, spline_ext, max_s, delta_s, x, y, s, angle, k, count))
        return fail(PQP_ERR_INVALID, "pqp_segment_raw_reference: bad argument");
    const size_t bn = (size_t)batch * n_max;
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4), *d_max_s = st.in(max_s, batch);
    double *d_x = st.out(x, bn, 0), *d_y = st.out(y, bn, 0), *d_s = st.out(s, bn, 0), *d_angle = st.out(angle, bn, 0), *d_k = st.out(k, bn, 0);
    int32_t* d_count = st.out(count, batch);
    return st.run([&]() -> int { return pqp_segment_raw_reference_device(h, batch, n_max, m, d_spl, d_ext, d_max_s, delta_s, d_x, d_y, d_s, d_angle, d_k, d_count); });
}

int pqp_reference_states(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext, const double* max_s,
                         const double* start, double ds_small, double ds_large, int dynamic, double* ref, int32_t* count,
                         double* init_err) {
    if (!reference_states_ok(h, batch, n_max, m, spline, spline_ext, max_s, start, ds_small, ds_large, ref, count, init_err))
        return fail(PQP_ERR_INVALID, "pqp_reference_states: bad argument");
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4), *d_max_s = st.in(max_s, batch);
    const double* d_start = st.in(start, (size_t)batch * 3);
    double* d_ref = st.out(ref, (size_t)batch * n_max * PQP_REF_STRIDE, 0);
    int32_t* d_count = st.out(count, batch);
    double* d_err = init_err ? st.out(init_err, (size_t)batch * 2) : nullptr;
    return st.run([&]() -> int {
        return pqp_reference_states_device(h, batch, n_max, m, d_spl, d_ext, d_max_s, d_start, ds_small, ds_large, dynamic, d_ref, d_count, d_err);
    });
}

// ---- lateral offsets on a line -> points with chord-length abscissae (tail of ReferencePathSmoother::postSmooth) ---------------------
static bool offsets_ok(pqp_handle* h, int batch, int m_spline, int m, const double* spline, const double* spline_ext, const double* at_s, const double* l,
                       const double* x, const double* y, const double* s) {
    return h && spline && spline_ext && at_s && l && x && y && s && batch >= 1 && m_spline >= 3 && m >= 1;
}

int pqp_offsets_to_points_device(pqp_handle* h, int batch, int m_spline, int m, const double* spline, const double* spline_ext, const double* at_s,
                                 const double* l, const int32_t* m_of, double* x, double* y, double* s) {
    if (!offsets_ok(h, batch, m_spline, m, spline, spline_ext, at_s, l, x, y, s)) return fail(PQP_ERR_INVALID, "pqp_offsets_to_points: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    pqp::OffsetsArgs a;
    a.batch = batch; a.m_spl = m_spline; a.m = m; a.spl = spline; a.spl_ext = spline_ext; a.at_s = at_s; a.l = l; a.m_of = m_of;
    a.x = x; a.y = y; a.s = s;
    const size_t lds = ((size_t)9 * m_spline + 2 * (size_t)m) * 8;
    return line_launch(h, (const void*)pqp::offsets_to_points_kernel, lds, "pqp_offsets_to_points: 9 m_spline + 2 m doubles exceed one CU's LDS", 0,
                       [&](auto go_long, double*) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_offsets_kernel, dim3(batch), dim3(64), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::offsets_to_points_kernel, dim3(batch), dim3(64), lds, h->stream, a);
    });
}

int pqp_offsets_to_points(pqp_handle* h, int batch, int m_spline, int m, const double* spline, const double* spline_ext, const double* at_s,
                          const double* l, const int32_t* m_of, double* x, double* y, double* s) {
    if (!offsets_ok(h, batch, m_spline, m, spline, spline_ext, at_s, l, x, y, s)) return fail(PQP_ERR_INVALID, "pqp_offsets_to_points: bad argument");
    const size_t bm = (size_t)batch * m;
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m_spline), *d_ext = st.in(spline_ext, (size_t)batch * 4);
    const double *d_at_s = st.in(at_s, bm), *d_l = st.in(l, bm);
    const int32_t* d_m_of = st.in(m_of, batch);
    double *d_x = st.out(x, bm, 0), *d_y = st.out(y, bm, 0), *d_s = st.out(s, bm, 0);
    return st.run([&]() -> int { return pqp_offsets_to_points_device(h, batch, m_spline, m, d_spl, d_ext, d_at_s, d_l, d_m_of, d_x, d_y, d_s); });
}

// ---- length of the reference line up to the target state (PathOptimizer::setReferencePathLength) ---------------------------------
static bool reference_length_ok(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length, const double* target,
                                const double* length_out) {
    return h && spline && spline_ext && length && target && length_out && batch >= 1 && m >= 3;
}

int pqp_reference_length_device(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length,
                                const double* target, double* length_out) {
    if (!reference_length_ok(h, batch, m, spline, spline_ext, length, target, length_out)) return fail(PQP_ERR_INVALID, "pqp_reference_length: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    pqp::RefLengthArgs a;
    a.batch = batch; a.m = m; a.spl = spline; a.spl_ext = spline_ext; a.length = length; a.target = target; a.length_out = length_out;
    const size_t lds = (size_t)9 * m * 8;
    return line_launch(h, (const void*)pqp::reference_length_kernel, lds, "pqp_reference_length: 9 m doubles exceed one CU's LDS", 0,
                       [&](auto go_long, double*) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_ref_length_kernel, dim3(batch), dim3(64), 0, h->stream, a);
        else hipLaunchKernelGGL(pqp::reference_length_kernel, dim3(batch), dim3(64), lds, h->stream, a);
    });
}

int pqp_reference_length(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length,
                         const double* target, double* length_out) {
    if (!reference_length_ok(h, batch, m, spline, spline_ext, length, target, length_out)) return fail(PQP_ERR_INVALID, "pqp_reference_length: bad argument");
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4);
    const double *d_length = st.in(length, batch), *d_target = st.in(target, (size_t)batch * 3);
    double* d_out = st.out(length_out, batch);
    return st.run([&]() -> int { return pqp_reference_length_device(h, batch, m, d_spl, d_ext, d_length, d_target, d_out); });
}

// ---- input points -> dense raw reference line (ReferencePathSmoother::bSpline) --------------------------------------------------
static bool bspline_ok(pqp_handle* h, int batch, int p_max, int n_max, const double* points, const int32_t* n_points, const double* x, const double* y,
                       const double* s, const int32_t* count) {
    return h && points && n_points && x && y && s && count && batch >= 1 && p_max >= 4 && n_max >= 2;
}

int pqp_bspline_resample_device(pqp_handle* h, int batch, int p_max, int n_max, const double* points, const int32_t* n_points, double* x,
                                double* y, double* s, int32_t* count) {
    if (!bspline_ok(h, batch, p_max, n_max, points, n_points, x, y, s, count))
        return fail(PQP_ERR_INVALID, "pqp_bspline_resample: bad argument (at least 4 input points: reference_path_smoother.cpp:33)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::BsplineArgs a;
    a.batch = batch; a.p_max = p_max; a.n_max = n_max; a.pts = points; a.n_pts = n_points; a.x = x; a.y = y; a.s = s; a.count = count;
    const size_t lds = ((size_t)3 * p_max + 6 + (size_t)3 * n_max) * 8;
    return line_launch(h, (const void*)pqp::bspline_resample_kernel, lds, "pqp_bspline_resample: 3 p_max + 3 n_max doubles exceed one CU's LDS", (size_t)batch * (p_max + 6) * 8,
                       [&](auto go_long, double* ws) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_bspline_kernel, dim3(batch), dim3(64), 0, h->stream, a, ws);
        else hipLaunchKernelGGL(pqp::bspline_resample_kernel, dim3(batch), dim3(64), lds, h->stream, a);
    });
}

int pqp_bspline_resample(pqp_handle* h, int batch, int p_max, int n_max, const double* points, const int32_t* n_points, double* x, double* y,
                         double* s, int32_t* count) {
    if (!bspline_ok(h, batch, p_max, n_max, points, n_points, x, y, s, count)) return fail(PQP_ERR_INVALID, "pqp_bspline_resample: bad argument");
    const size_t bn = (size_t)batch * n_max;
    Staging st(h);
    const double* d_pts = st.in(points, (size_t)batch * p_max * 2);
    const int32_t* d_n_pts = st.in(n_points, batch);
    double *d_x = st.out(x, bn, 0), *d_y = st.out(y, bn, 0), *d_s = st.out(s, bn, 0);
    int32_t* d_count = st.out(count, batch);
    return st.run([&]() -> int { return pqp_bspline_resample_device(h, batch, p_max, n_max, d_pts, d_n_pts, d_x, d_y, d_s, d_count); });
}

// ---- spline fit ---------------------------------------------------------------------------------------
static bool spline_fit_ok(pqp_handle* h, int batch, int m, const double* s, const double* x, const double* y, const double* spline, const double* spline_ext) {
    return h && s && x && y && spline && spline_ext && batch >= 1 && m >= 3;
}

static int spline_fit_impl(pqp_handle* h, int batch, int m, const int32_t* m_of, const double* s, const double* x, const double* y, double* spline,
                           double* spline_ext) {
    if (!spline_fit_ok(h, batch, m, s, x, y, spline, spline_ext)) return fail(PQP_ERR_INVALID, "pqp_spline_fit: bad argument (m >= 3: spline.cpp:164)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::SplineFitArgs a;
    a.m_of = m_of;
    a.batch = batch; a.m = m; a.s = s; a.vx = x; a.vy = y; a.spl = spline; a.spl_ext = spline_ext;
    const size_t lds = (size_t)7 * m * 8;
    return line_launch(h, (const void*)pqp::spline_fit_kernel, lds, "pqp_spline_fit: 7 m doubles exceed one CU's LDS", (size_t)2 * batch * lds,
                       [&](auto go_long, double* ws) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_fit_kernel, dim3(2 * batch), dim3(64), 0, h->stream, a, ws);
        else hipLaunchKernelGGL(pqp::spline_fit_kernel, dim3(2 * batch), dim3(64), lds, h->stream, a);
    });
}

int pqp_spline_fit_device(pqp_handle* h, int batch, int m, const double* s, const double* x, const double* y, double* spline,
                          double* spline_ext) {
    return spline_fit_impl(h, batch, m, nullptr, s, x, y, spline, spline_ext);
}

int pqp_spline_fit_var_device(pqp_handle* h, int batch, int m_max, const int32_t* m_of, const double* s, const double* x, const double* y,
                              double* spline, double* spline_ext) {
    if (!m_of) return fail(PQP_ERR_INVALID, "pqp_spline_fit_var: m_of is null");
    return spline_fit_impl(h, batch, m_max, m_of, s, x, y, spline, spline_ext);
}

int pqp_spline_fit(pqp_handle* h, int batch, int m, const double* s, const double* x, const double* y, double* spline, double* spline_ext) {
    if (!spline_fit_ok(h, batch, m, s, x, y, spline, spline_ext)) return fail(PQP_ERR_INVALID, "pqp_spline_fit: bad argument");
    const size_t bm = (size_t)batch * m;
    Staging st(h);
    const double *d_s = st.in(s, bm), *d_x = st.in(x, bm), *d_y = st.in(y, bm);
    double *d_spl = st.out(spline, 9 * bm), *d_ext = st.out(spline_ext, (size_t)batch * 4);
    return st.run([&]() -> int { return pqp_spline_fit_device(h, batch, m, d_s, d_x, d_y, d_spl, d_ext); });
}

// ---- layered DP corridor search ------------------------------------------------------------------------
void pqp_dp_default_params(pqp_dp_params* p) {
    if (!p) return;
    p->lateral_range = 10.0; p->longitudinal_spacing = 1.5; p->lateral_spacing = 0.6; p->car_width = 2.0;      // planning_flags.cpp:38-42,10
}

static bool dp_ok(pqp_handle* h, int batch, int m, int max_layers, const double* spline, const double* spline_ext, const double* length, const double* start,
                  const float* dist, const pqp_grid_geometry* geom, const pqp_dp_params* prm, const double* layers_s, const double* lb, const double* ub,
                  const int32_t* count, const double* vehicle_l) {
    return h && spline && spline_ext && length && start && dist && prm && layers_s && lb && ub && count && vehicle_l && batch >= 1 && m >= 3 &&
           max_layers >= 2 && geometry_ok(geom) && prm->lateral_spacing > 0.0 && prm->longitudinal_spacing > 0.0 &&
           !(2.0 * prm->lateral_range / prm->lateral_spacing + 1.0 > 64.0);
}

int pqp_dp_corridor_device(pqp_handle* h, int batch, int m, int max_layers, const double* spline, const double* spline_ext,
                           const double* length, const double* start, const float* dist, const int32_t* map_of,
                           const pqp_grid_geometry* geom, const pqp_dp_params* prm, double* layers_s, double* lb, double* ub,
                           int32_t* count, double* vehicle_l) {
    if (!dp_ok(h, batch, m, max_layers, spline, spline_ext, length, start, dist, geom, prm, layers_s, lb, ub, count, vehicle_l))
        return fail(PQP_ERR_INVALID, "pqp_dp_corridor: bad argument (at most 64 lateral samples per layer)");
    PQP_HIP(hipSetDevice(h->device));
    pqp::DpArgs a;
    a.batch = batch; a.m = m; a.max_layers = max_layers; a.spl = spline; a.spl_ext = spline_ext; a.length = length; a.start = start;
    a.dist = dist; a.map_of = map_of; a.g = *geom; a.p = *prm; a.layers_s = layers_s; a.lb = lb; a.ub = ub; a.count = count; a.vehicle_l = vehicle_l;
    const int nlat = pqp::dp_lateral_samples(prm->lateral_range, prm->lateral_spacing);
    const size_t lds = pqp::DpBlock<true, true>{m, max_layers, nlat}.total_bytes();
    const size_t lds_long = pqp::DpBlock<false, true>{m, max_layers, nlat}.total_bytes();
    return line_launch(h, (const void*)pqp::dp_corridor_kernel, lds, "pqp_dp_corridor: 9 m + 17 max_layers doubles (+ the edge table) exceed one CU's LDS",
                       (size_t)batch * pqp::DpBlock<true, false>{m, max_layers, nlat}.doubles() * 8, [&](auto go_long, double* ws) {
        if constexpr (go_long) hipLaunchKernelGGL(pqp::long_dp_kernel, dim3(batch), dim3(pqp::kDpThreads), lds_long, h->stream, a, ws);
        else hipLaunchKernelGGL(pqp::dp_corridor_kernel, dim3(batch), dim3(pqp::kDpThreads), lds, h->stream, a);
    }, (const void*)pqp::long_dp_kernel, lds_long, "pqp_dp_corridor: the long form's cost tables exceed one CU's LDS");
}

int pqp_dp_corridor(pqp_handle* h, int batch, int m, int max_layers, const double* spline, const double* spline_ext, const double* length,
                    const double* start, const float* dist, int n_maps, const int32_t* map_of, const pqp_grid_geometry* geom,
                    const pqp_dp_params* prm, double* layers_s, double* lb, double* ub, int32_t* count, double* vehicle_l) {
    if (!dp_ok(h, batch, m, max_layers, spline, spline_ext, length, start, dist, geom, prm, layers_s, lb, ub, count, vehicle_l) || n_maps < 1)
        return fail(PQP_ERR_INVALID, "pqp_dp_corridor: bad argument");
    const size_t bl = (size_t)batch * max_layers;
    Staging st(h);
    const double *d_spl = st.in(spline, (size_t)batch * 9 * m), *d_ext = st.in(spline_ext, (size_t)batch * 4);
    const double *d_length = st.in(length, batch), *d_start = st.in(start, (size_t)batch * 3);
    const float* d_dist = st.in(dist, (size_t)n_maps * geom->rows * geom->cols);
    const int32_t* d_map_of = st.in(map_of, batch);
    double *d_ls = st.out(layers_s, bl, 0), *d_lb = st.out(lb, bl, 0), *d_ub = st.out(ub, bl, 0);
    int32_t* d_count = st.out(count, batch);
    double* d_vl = st.out(vehicle_l, batch);
    return st.run([&]() -> int {
        return pqp_dp_corridor_device(h, batch, m, max_layers, d_spl, d_ext, d_length, d_start, d_dist, d_map_of, geom, prm, d_ls, d_lb, d_ub, d_count, d_vl);
    });
}

}  // extern "C"

#include "pqp_chain.inc"
