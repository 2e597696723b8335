// pqp_kernels.hip — the core of libpqp_hip.so (gfx950, MI355X / CDNA4): the handle and the path-QP entry points of include/pqp.h.
//
//   shared state          the thread-local message of pqp_last_error, the allocation generation, the static-LDS cache: defined here,
//                         declared in pqp_internal.hpp for the other translation units
//   handle                pqp_create / pqp_destroy, parameters and options, marks, sync, the timing ring
//   path_solve_kernel     the lane-per-waypoint path-QP kernel lives in pqp_path_solve.hip (one translation unit per workgroup width),
//                         the lane-per-QP kernel in pqp_path_stream.hip; this file holds their launchers, path_solve_impl / path_stream_impl.
//   path_assemble_kernel  BaseSolver::setCost/setConstraints in the REFERENCE numbering: CSC values of A,
//                         diagonal of P, l, u; staged through LDS and written with contiguous, coalesced
//                         stores (base_solver.cpp:119-261).
//   path_pattern_kernel   the value-independent CSC pattern (integer index maps, base_solver.cpp:154-209).
//   path_gather_solution  lane layout -> reference numbering of the primal / dual solution.
//
// The other kernel families, each with its kernels, launchers and entry points: pqp_smoothers.hip (the reference-line smoothing QPs),
// pqp_lines.hip (line geometry: corridor bounds, reference states, spline fit, DP, projection), pqp_maps.hip (distance layer, footprints,
// standing agents over the layers), pqp_agents.hip (trajectories against predicted agents, the agents' prediction), pqp_speed.hip (speed
// profile, trajectory samples, path-time search, speed refine, fine plan samples), pqp_select.hip (path selection, plan ranking),
// pqp_chain.hip (pqp_optimize_path_device).
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
#include <vector>

#include "pqp_defaults.hpp"
#include "pqp_path_lane.hpp"
#include "pqp_path_lq_abi.hpp"
#include "pqp_wave.hpp"
#include "pqp_internal.hpp"

using namespace pqp_internal;

namespace pqp {

// -------------------------------------------------------------------------------------------------------
// reference numbering helpers (base_solver.cpp:22-37,154-158)
// -------------------------------------------------------------------------------------------------------
struct RefIndex {
    int n, precise;
    int with_l;      // weight_l != 0: P's diagonal has the l_i columns too (the reference's sparseView drops them only while weight_l is an exact zero, base_solver.cpp:123,145)
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
    __host__ __device__ int nnz_p() const { return p_states() + n - 1 + precise + n; }
    // P's diagonal in ascending column order: per waypoint (l_i,) k_i; then u_i; then the slacks
    __host__ __device__ int p_states() const { return with_l ? 2 * n : n; }
    __host__ __device__ int p_kappa(int i) const { return with_l ? 2 * i + 1 : i; }
    __host__ __device__ int p_control(int i) const { return p_states() + i; }
    __host__ __device__ int p_slack(int i, int which) const { return p_states() + n - 1 + (i < precise ? 2 * i + which : 2 * precise + (i - precise)); }
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
    // P diagonal columns (base_solver.cpp:127-143), ascending: (l_i,) k_i, then u_i, then slacks
    if (R.with_l) pcols[2 * i] = 3 * i;
    pcols[R.p_kappa(i)] = 3 * i + 2;
    if (has_next) pcols[R.p_control(i)] = R.state() + i;
    if (precise) { pcols[R.p_slack(i, 0)] = R.slack_col(i, 0); pcols[R.p_slack(i, 1)] = R.slack_col(i, 1); }
    else pcols[R.p_slack(i, 0)] = R.slack_col(i, 0);
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
            if (R.with_l) vp[2 * i] = prm.weight_l;
            vp[R.p_kappa(i)] = prm.weight_kappa;
            if (has_next) vp[R.p_control(i)] = prm.weight_dkappa;
            if (precise) { vp[R.p_slack(i, 0)] = prm.weight_slack; vp[R.p_slack(i, 1)] = prm.weight_slack; }
            else vp[R.p_slack(i, 0)] = prm.weight_slack;
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

// =========================================================================================================
// the state behind pqp_internal.hpp: one definition each
// =========================================================================================================
namespace {
thread_local std::string g_last_error;
}  // namespace

namespace pqp_internal {
int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

std::atomic<unsigned long long> g_alloc_generation{0};

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

int lds_opt_in(const void* fn, size_t bytes, const char* who) {
    size_t fixed = 0;
    if (const int rc = static_lds(fn, &fixed)) return rc;
    if (bytes > kLdsPerCu - fixed) return fail(PQP_ERR_CAPACITY, who);
    if (fixed + bytes > 48 * 1024) PQP_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return PQP_OK;
}

int long_form(int opt, const void* fn, size_t bytes, bool* out) {
    *out = opt == 2;
    if (opt != 1) return PQP_OK;
    size_t fixed = 0;
    if (const int rc = static_lds(fn, &fixed)) return rc;
    *out = bytes > kLdsPerCu - fixed;
    return PQP_OK;
}
}  // namespace pqp_internal

// =========================================================================================================
// C ABI
// =========================================================================================================
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
        for (int k = 0; k < pqp_handle::Timing::kEvSlots; ++k) { PQP_HIP(hipEventCreate(&h->timing.evs0[k])); PQP_HIP(hipEventCreate(&h->timing.evs1[k])); }
        for (int k = 0; k < pqp_handle::kMarks + pqp_handle::kChainMarks; ++k) PQP_HIP(hipEventCreateWithFlags(&h->marks[k], hipEventDisableTiming));
        int rc;
        if ((rc = h->lane.ticket.ensure(8)) || (rc = h->lane.cost_hist.ensure(2 * pqp::kCostBins * 4))) return rc;
        if (max_batch > 0 && max_n > 0) {
            const size_t bn = (size_t)max_batch * max_n;
            if ((rc = h->lane.wx.ensure(bn * 6 * 8)) || (rc = h->lane.wy.ensure(bn * 6 * 8)) || (rc = h->lane.wye.ensure((size_t)max_batch * 2 * 8)) ||
                (rc = h->lane.wrho.ensure((size_t)max_batch * 8)))
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
    for (auto& g : h->chain.graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    h->chain.graphs.clear();
    for (int k = 0; k < pqp_handle::Timing::kEvSlots; ++k) { if (h->timing.evs0[k]) (void)hipEventDestroy(h->timing.evs0[k]); if (h->timing.evs1[k]) (void)hipEventDestroy(h->timing.evs1[k]); }
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
    for (const OptionRow& row : kOptionTable) {
        if (row.id != option) continue;
        h->opt.*row.member = row.normalise(value);
        h->invalidate(row.stale);
        return PQP_OK;
    }
    return fail(PQP_ERR_INVALID, "pqp_set_option: unknown option");
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
    pqp::RefIndex R{n, precise, params->weight_l != 0.0};
    out->n = n; out->state = 3 * n; out->control = n - 1; out->precise = precise; out->slack = precise + n;
    out->vars = R.vars(); out->cons = R.cons(); out->nnz_a = R.nnz_a(); out->nnz_p = R.nnz_p();
    return PQP_OK;
}

int pqp_path_pattern(pqp_handle* h, int n, int precise, int32_t* rows, int32_t* colptr, int32_t* pcols) {
    if (!h || !rows || !colptr || !pcols || n < 2 || precise < 0 || precise > n)
        return fail(PQP_ERR_INVALID, "pqp_path_pattern: bad argument");
    pqp::RefIndex R{n, precise, h->prm.weight_l != 0.0};
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
    pqp::RefIndex R{n, precise, h->prm.weight_l != 0.0};
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
    pqp::RefIndex R{n, precise, h->prm.weight_l != 0.0};
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
    const void* ws_before = h->strm.ws.p;
    if ((rc = h->strm.ws.ensure((size_t)waves * n * pqp::lq::kBlockDoubles * 64 * 8))) return rc;
    pqp::lq::Args a;
    std::memset(&a, 0, sizeof(a));
    a.batch = batch; a.n = n; a.passes = passes; a.n_of = n_of; a.ref = ref; a.lin = lin; a.bounds = bounds; a.scal = scal; a.out = out;
    a.status = status; a.iters = iters; a.info = info; a.ws = h->strm.ws.as<double>(); a.prm = h->prm;
    // Which of the kernel's two workspace layouts (pqp_path_lq_abi.hpp): a launch that leaves SIMDs idle - fewer than 768 wavefronts - waits for its loads, not for
    // HBM's throughput: the sweeps' records staged in LDS two waypoints ahead, +29 ... 33 % at 24 576 / 32 768 QPs of 80 waypoints; a launch that fills the chip
    // loses 3-4 % with them (profiles/r06au_*) and keeps the [field][lane] layout and the register prefetch.  A function of the shape alone: what PQP_OPT_CARRY_CYCLES
    // finds in the workspace was left there in the same layout.
    a.staged = h->opt.stream_staged >= 0 ? h->opt.stream_staged : (waves < 3 * h->num_cu ? 1 : 0);
    // PQP_OPT_CARRY_CYCLES: the workspace still holds, slot by slot, the optimum of the previous launch of this very shape
    a.carry = (h->opt.carry && !lin && h->strm.last_batch == batch && h->strm.last_n == n && h->strm.ws.p == ws_before) ? 1 : 0;       // (lin == NULL: pqp.h)
    // PQP_OPT_ORDER_BY_COST: wavefronts of QPs that ran the same phases in the handle's previous solve of the shape.  Only where it pays - batches that
    // put a wavefront on (nearly) every SIMD: below that a launch lasts as long as one wavefront's sweeps whatever its lanes do (profiles/r05g_*) - and
    // not with PQP_OPT_CARRY_CYCLES (a slot's workspace then holds the previous optimum of the QP that sat there) or inside a graph capture (host-side parity).
    const bool ordered = h->opt.order_by_cost && !h->opt.carry && !h->chain.capturing && waves >= 3 * h->num_cu;
    if (ordered) {
        if ((rc = h->strm.key_buf.ensure((size_t)batch * 4)) || (rc = h->strm.hist.ensure(((size_t)pqp::lq::kOrderBins + 1) * 4)) ||
            (rc = h->strm.order.ensure((size_t)2 * batch * 4)))
            return rc;
        if (h->strm.order_batch != batch || h->strm.order_n != n) {          // a shape change: stale counts, no map yet
            PQP_HIP(hipMemsetAsync(h->strm.hist.p, 0, ((size_t)pqp::lq::kOrderBins + 1) * 4, h->stream));
            a.order = nullptr;
        } else {
            a.order = h->strm.order.as<int32_t>() + (size_t)(h->strm.solves & 1) * batch;
        }
        a.key_out = h->strm.key_buf.as<int32_t>();
        a.hist = h->strm.hist.as<int32_t>();
        a.order_next = h->strm.order.as<int32_t>() + (size_t)((h->strm.solves + 1) & 1) * batch;
    }
    // (path_stream_kernel lives in its own translation unit, pqp_path_stream.hip)
    if ((rc = h->launch_timed([&]() -> int { PQP_HIP(pqp_stream_launch(&a, waves, (void*)h->stream)); return PQP_OK; }))) return rc;
    if (ordered) { h->strm.solves += 1; h->strm.order_batch = batch; h->strm.order_n = n; }
    h->strm.last_batch = batch; h->strm.last_n = n;
    h->lane.solved(PQP_KERNEL_LANE_PER_QP, batch, n, /*stored=*/false);
    return PQP_OK;
}

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

// ---- path_solve_impl in its steps: route, plan, arguments, launch, commit ---------------------------------------------------------

// 1. Route: which kernel serves the call, and whether a cold call is promoted to a warm one (PQP_OPT_CARRY_CYCLES)
struct PathRoute { bool stream; int warm, carry_tails; };
static PathRoute path_route(const pqp_handle* h, int batch, int n, const double* lin, int warm) {
    // lane-per-QP kernel: large batches of a caller that keeps no warm state (PQP_OPT_STREAM_BATCH), and every path of more than 512
    // waypoints (the lane-per-waypoint kernel's workgroup ends there; a reference path of 80 m at 0.15 m spacing has 530:
    // reference_path_impl.cpp:321-336) - those with any batch size and without warm state
    // (warm == 1 beyond 512 waypoints: the QP around `lin` is solved cold - its optimum is unique, a warm start only saves iterations -
    //  so BaseSolver::solve + updateProblemFormulationAndSolve work at any size; and there also a handle in the reference's ADMM setting
    //  gets the exact optimum: zero residuals meet OSQP's termination test at any eps)
    const int stream_from = h->opt.stream_batch < 0 ? stream_batch_auto(n) : h->opt.stream_batch;
    if ((n > 512 && (!warm || lin)) || (h->prm.polish != 0 && !warm && !h->opt.store_warm && stream_from > 0 && batch >= stream_from))
        return {true, warm, 0};
    // PQP_OPT_CARRY_CYCLES on this kernel: a cold call (warm == 0, lin == NULL) of the shape of the handle's previous solve starts from
    // the final iterate, equilibration and active set that solve left in the warm state - the same scenarios one planning cycle later.
    // (With waypoint counts per QP the state is kept per waypoint: a path that grew or shrank by a few waypoints since the previous cycle
    //  starts its common waypoints from where they were and the new ones from whatever the slot last held there - zero at first.)
    // (only on a handle whose polish returns the exact optimum: with polish == 0 - the reference's ADMM setting - a promoted call would end at an
    //  eps-accurate point that depends on the slot's previous QP, and pqp.h promises the cold solve's optimum to the 1e-7 of the KKT test)
    // (value k >= 2, "tails": only the QPs that were among the most expensive 1 / k of the previous launch - by the cost keys PQP_OPT_ORDER_BY_COST
    //  keeps - start from there, the others start cold: what bounds a launch is its slowest QPs)
    if (h->opt.carry && h->prm.polish != 0 && !warm && !lin && h->lane.warm_is(batch, n) &&
        (h->opt.carry < 2 || (h->opt.order_by_cost && h->lane.hist_batch == batch && h->lane.hist_n == n)))
        return {false, 1, h->opt.carry >= 2 ? h->opt.carry : 0};
    return {false, warm, 0};
}

// 2. Plan: the kernel variant and its launch geometry for paths of n waypoints, with the workgroup slots' save area allocated
struct PathPlan { const void* fn; int threads, grid; size_t lds; };
static int path_plan(pqp_handle* h, int batch, int n, bool cert, PathPlan* plan) {
    int nw = 1, lg = 0;
    while (64 * nw < n) { nw *= 2; lg += 1; }           // one waypoint per lane: T = 64 * nw >= n threads per QP
    const int T_lanes = 64 * nw;
    const bool save_lds = nw <= pqp::kSaveLdsMaxNw;
    const size_t lds = (size_t)pqp::ShLayout{T_lanes}.total(save_lds) * 8;
    const void* fn = nullptr;
    switch (nw) {       // (pqp_path_solve.hip, one translation unit per width)
        case 1: fn = pqp_path_solve_fn_nw1(cert); break;
        case 2: fn = pqp_path_solve_fn_nw2(cert); break;
        case 4: fn = pqp_path_solve_fn_nw4(cert); break;
        default: fn = pqp_path_solve_fn_nw8(cert); break;
    }
    int rc;
    if ((rc = lds_opt_in(fn, lds, "pqp_path_solve: LDS"))) return rc;
    // persistent workgroups: as many as the chip holds at once (a surplus one would only wait for a free slot), each with its own
    // save area; they draw the QPs from the ticket counter
    int& per_cu = h->lane.blocks_per_cu[2 * lg + (cert ? 1 : 0)];
    if (per_cu == 0) {
        PQP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, T_lanes, lds));
        if (per_cu < 1) per_cu = 1;
    }
    const int cus = h->num_cu - h->opt.reserve_cus > 1 ? h->num_cu - h->opt.reserve_cus : 1;
    const long long resident = (long long)per_cu * cus;
    const int grid = (int)(batch < resident ? batch : resident);
    if (!save_lds) {          // more than 256 lanes per QP: the save area and the parked Ruiz vectors live in the workgroup slot's global memory
        if ((rc = h->lane.wsave.ensure((size_t)grid * T_lanes * PQP_SAVE_STRIDE * 8))) return rc;
        if ((rc = h->lane.wscale.ensure((size_t)grid * T_lanes * 18 * 8))) return rc;
    }
    *plan = {fn, T_lanes, grid, lds};
    return PQP_OK;
}

// 3. Arguments, the part that is the handle's: its buffers, parameters and options, the ticket base, the cost order.  What it enqueues
// (the ticket reset of a capture, the clearing of a stale histogram) precedes the launch on the stream.
static int path_args(pqp_handle* h, const PathRoute& route, pqp::PathSolveArgs& a) {
    pqp_handle::LanePath& L = h->lane;
    const int batch = a.batch, n = a.n;
    int rc;
    a.warm = route.warm ? 1 : 0;
    a.wx = L.wx.as<double>(); a.wy = L.wy.as<double>(); a.wye = L.wye.as<double>(); a.wrho = L.wrho.as<double>();
    a.prm = h->prm;
    // Long paths: the polished point's residuals in the transition rows add up along the path - the rows are a discrete double integrator, an error of
    // 1e-9 per row in (psi, kappa) is 1e-4 in l after 300 waypoints - so an accepted point gets one more refinement solve per pass beyond 128 waypoints, three beyond 256 (each shrinks the error ~10x: 4.6e-3 -> 4.4e-4 -> 4.1e-5 -> 3.3e-6 on
    // the worst path of 300 waypoints; the kernels of up to 128 waypoints do not compile the feature in: Ctx::kFinalRefine) (a 100x
    // tighter acceptance test instead leaves a few QPs in 30 000 unverifiable: 350-1000 solves, configs[4] halved).  Measured against the converged C oracle over 32 768 QPs per shape (profiles/r05o_*): before, 7 paths of 200 waypoints
    // and 117 of 300 were 3e-5 ... 4.6e-3 off (the lane-per-QP kernel, whose roll-out satisfies the rows exactly: 5e-6).
    // ... and the production setting's intervals by path length (pqp_defaults.hpp)
    pqp::resolve_path_params(&a.prm, n);
    a.wsave = L.wsave.as<double>();
    a.wscale = L.wscale.as<double>();
    a.store_warm = (h->opt.store_warm || h->opt.carry) ? 1 : 0;
    a.carry_tails = route.carry_tails;
    a.carry_k = h->opt.carry;
    a.ticket = L.ticket.as<unsigned long long>();
    a.ticket_base = L.ticket_next;
    // inside a captured graph the launch cannot take its ticket base from a host counter that moves between replays: the graph resets the
    // device counter itself and every replay starts at 0 (pqp_chain.hip puts the host counter where the replay leaves the device one)
    if (h->chain.capturing) { PQP_HIP(hipMemsetAsync(L.ticket.p, 0, 8, h->stream)); a.ticket_base = 0; }
    if (h->opt.order_by_cost) {
        // most expensive QPs first, by what they cost in this handle's previous solve of the same shape (a planner re-solves
        // nearly the same scenarios cycle after cycle); results do not depend on the order
        if ((rc = L.cost_key.ensure((size_t)batch * 4)) || (rc = L.order.ensure((size_t)2 * batch * 4))) return rc;
        // two order arrays: the one this launch reads (written by the previous launch's last workgroup) and the one it writes
        int32_t* order_read = L.order.as<int32_t>() + (size_t)(L.solves & 1) * batch;
        int32_t* order_write = L.order.as<int32_t>() + (size_t)((L.solves + 1) & 1) * batch;
        if (L.hist_batch == batch && L.hist_n == n) a.order = order_read;
        else { L.hist_batch = 0; L.hist_n = 0; PQP_HIP(hipMemsetAsync(L.cost_hist.p, 0, (pqp::kCostBins + 1) * 4, h->stream)); }     // (a shape change: stale counts)
        a.cost_key = L.cost_key.as<int32_t>();
        a.cost_hist = L.cost_hist.as<int32_t>();
        a.order_next = order_write;
    }
    return PQP_OK;
}

static int path_solve_impl(pqp_handle* h, int batch, int n, const int32_t* n_of, const double* ref, const double* lin, const double* bounds,
                           const double* scal, int passes, int warm, double* out, int32_t* status, int32_t* iters, double* info) {
    if (!path_solve_ok(h, batch, n, ref, bounds, scal, passes, out)) return fail(PQP_ERR_INVALID, "pqp_path_solve: bad argument");
    PQP_HIP(hipSetDevice(h->device));
    pqp_handle::LanePath& L = h->lane;
    // ---- 1. route ----
    const PathRoute route = path_route(h, batch, n, lin, warm);
    if (route.stream) return path_stream_impl(h, batch, n, n_of, ref, lin, bounds, scal, passes, out, status, iters, info);
    if (n > 512) return fail(PQP_ERR_CAPACITY, "pqp_path_solve: warm == 1 beyond 512 waypoints needs the linearisation point (`lin`): the lane-per-QP kernel keeps no warm state");
    if (route.warm && !L.warm_is(batch, n))
        return fail(PQP_ERR_INVALID, "pqp_path_solve: warm == 1 needs a previous solve with the same batch and n (with PQP_OPT_STORE_WARM on)");
    const size_t bn = (size_t)batch * n;
    int rc;
    if (!route.warm) {
        if ((rc = L.wx.ensure(bn * 6 * 8)) || (rc = L.wy.ensure(bn * 6 * 8)) || (rc = L.wye.ensure((size_t)batch * 2 * 8)) ||
            (rc = L.wrho.ensure((size_t)batch * 8)))
            return rc;
    }
    // ---- 2. plan ----
    // two variants of every kernel: with and without OSQP's primal infeasibility certificate (prm.eps_prim_inf > 0)
    const bool cert = h->prm.eps_prim_inf > 0.0 && h->prm.prim_inf_after <= 0;
    PathPlan plan;
    if ((rc = path_plan(h, batch, n, cert, &plan))) return rc;
    // ---- 3. arguments: the call's, then the handle's ----
    pqp::PathSolveArgs a;
    std::memset(&a, 0, sizeof(a));
    a.batch = batch; a.n = n; a.n_of = n_of; a.passes = passes;
    a.ref = ref; a.lin = lin; a.bounds = bounds; a.scal = scal; a.out = out;
    a.status = status; a.iters = iters; a.info = info;
    if ((rc = path_args(h, route, a))) return rc;
    // ---- 4. launch, 5. commit ----
    // Host-side bookkeeping of the launch (ticket base of the next launch, launch parity, shape of the cost histogram) is committed
    // only after the launch has been accepted: a failing step above or here (allocation, memset, event, launch) leaves the device ticket
    // counter and the host's idea of it in step.
    bool accepted = false;
    rc = h->launch_timed([&]() -> int {
        void* kargs[] = {(void*)&a};
        hipError_t le = hipLaunchKernel(plan.fn, dim3(plan.grid), dim3(plan.threads), kargs, plan.lds, h->stream);
        if (le == hipSuccess) le = hipGetLastError();
        if (le != hipSuccess) {
            L.hist_batch = 0; L.hist_n = 0;          // (the histogram may have been cleared for a launch that never ran)
            return fail(PQP_ERR_HIP, std::string("hipLaunchKernel(path_solve_kernel): ") + hipGetErrorString(le));
        }
        accepted = true;
        return PQP_OK;
    });
    if (!accepted) return rc;
    L.ticket_next = a.ticket_base + (unsigned long long)batch + (unsigned long long)plan.grid;
    if (h->opt.order_by_cost) { L.hist_batch = batch; L.hist_n = n; }
    L.solves += 1;
    if (rc) return rc;          // (the launch is on the stream, its closing event is not: the kernel's tickets are spent, the call still fails)
    L.solved(PQP_KERNEL_LANE_PER_WAYPOINT, batch, n, /*stored=*/h->opt.store_warm != 0 || h->opt.carry != 0);
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
    if (!h->lane.warm_is(batch, n))
        return fail(PQP_ERR_INVALID, "pqp_path_get_solution: no solve of that shape on this handle (or PQP_OPT_STORE_WARM is off)");
    pqp::RefIndex R{n, precise};
    Staging st(h);
    double* d_x = st.out(x, (size_t)batch * R.vars(), 0);
    double* d_y = st.out(y, (size_t)batch * R.cons(), 0);
    return st.run([&]() -> int {
        const int total = batch * n;
        hipLaunchKernelGGL(pqp::path_gather_solution, dim3((total + 255) / 256), dim3(256), 0, h->stream, R, batch, h->lane.wx.as<double>(),
                           h->lane.wy.as<double>(), h->lane.wye.as<double>(), x ? d_x : nullptr, y ? d_y : nullptr);
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
    return h->lane.last_path_kernel;
}

int pqp_last_kernel_ms(pqp_handle* h, float* ms) {
    if (!h || !ms) return fail(PQP_ERR_INVALID, "pqp_last_kernel_ms: null argument");
    if (!h->timing.timed) return fail(PQP_ERR_INVALID, "pqp_last_kernel_ms: nothing was launched yet");
    PQP_HIP(hipSetDevice(h->device));
    const long long idx = (h->timing.ev_count - 1) % pqp_handle::Timing::kEvSlots;
    PQP_HIP(hipEventSynchronize(h->timing.evs1[idx]));
    PQP_HIP(hipEventElapsedTime(ms, h->timing.evs0[idx], h->timing.evs1[idx]));
    return PQP_OK;
}

int pqp_kernel_ms_history(pqp_handle* h, float* ms, int count) {
    if (!h || !ms || count < 1) return fail(PQP_ERR_INVALID, "pqp_kernel_ms_history: bad argument");
    if (count > pqp_handle::Timing::kEvRing || (long long)count > h->timing.ev_count)
        return fail(PQP_ERR_INVALID, "pqp_kernel_ms_history: more launches asked for than the ring holds (256) or were made");
    PQP_HIP(hipSetDevice(h->device));
    PQP_HIP(hipStreamSynchronize(h->stream));
    for (int k = 0; k < count; ++k) {          // oldest of the requested launches first
        const long long idx = (h->timing.ev_count - count + k) % pqp_handle::Timing::kEvSlots;
        PQP_HIP(hipEventElapsedTime(ms + k, h->timing.evs0[idx], h->timing.evs1[idx]));
    }
    return PQP_OK;
}

}  // extern "C"
