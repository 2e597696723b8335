// pqp_internal.hpp — host side only: what the translation units of libpqp_hip.so share behind the C ABI of include/pqp.h.  The handle, its
// device buffers, launch timing and host staging, the error message of pqp_last_error, and the launch and checking helpers that several kernel families use.
// Everything here lives in a namespace of hidden visibility: the library exports the entry points of pqp.h (and its kernels' host stubs), nothing of this.
// The state behind it - the thread-local error message, the allocation generation, the cache of static_lds - is defined once, in pqp_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pqp.h"

namespace pqp { struct CarCircles; }     // pqp_car_circles.hpp (device side)

#ifndef PQP_HIDDEN
#define PQP_HIDDEN __attribute__((visibility("hidden")))      // (also pqp_chain_ws.hpp, which stands alone)
#endif
namespace pqp_internal PQP_HIDDEN {

// sets the calling thread's message (pqp_last_error) and returns `code`
int fail(int code, const std::string& msg);
#define PQP_HIP(call)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return ::pqp_internal::fail(PQP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// every (re)allocation of a device buffer of the library: captured hipGraphs of the chain hold device pointers and are only replayed
// while this has not moved (pqp_chain.hip)
extern std::atomic<unsigned long long> g_alloc_generation;

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

// The arrays of a batch of QPs for the generic banded core (pqp_banded_qp.hpp): the problem data, the solution and the sparsity its batch
// shares, cached per structure type and size.  Each user of the core on the handle owns one (the smoothers, the speed refine), so one's
// structure never displaces another's.
struct BandedGroup {
    DevBuf pband, q, aval, lo, up, x, y, acol, trow, tslot;
    int struct_type = -1, struct_n = -1;
};

// one CU's LDS on gfx950: the most dynamic LDS a workgroup can have
constexpr size_t kLdsPerCu = 160 * 1024;

// the static LDS of kernel `fn`: its __shared__ variables, padded to the alignment of the dynamic LDS that follows them (the compiler's
// "LDS Size" remark; 16 bytes for a single int in front of an aligned(16) array).  Looked up once per kernel.
int static_lds(const void* fn, size_t* out);

// `bytes` of dynamic LDS for kernel `fn`: PQP_ERR_CAPACITY (message `who`) when they and the kernel's static LDS exceed one CU's LDS, the
// opt-in beyond the 48 KiB any kernel may use.  The attribute takes the dynamic bytes alone (the runtime adds the static ones to it).
int lds_opt_in(const void* fn, size_t bytes, const char* who);

// PQP_OPT_LONG_LINES = `opt`: whether a launch of the LDS kernel `fn` with `bytes` of dynamic LDS goes to its long form
// (long_*_kernel, pqp_corridor_kernels.inc) - never (0), where the LDS kernel does not fit one CU (1), always (2)
int long_form(int opt, const void* fn, size_t bytes, bool* out);

// Bytes that identify what a launch sequence depends on (the chain's captured graphs, pqp_chain.hip).  bytes() takes a type only where
// every bit of it is value: no padding.
struct Key {
    std::vector<unsigned char> v;
    void put(const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; v.insert(v.end(), b, b + n); }
    void put_int(long long x) { put(&x, sizeof(x)); }
    template <class T> void bytes(const T& x) { static_assert(std::is_trivially_copyable_v<T>); put(&x, sizeof(T)); }
    bool operator==(const Key& o) const { return v == o.v; }
};
// the structs of pqp.h that go into a Key as bytes: the size of each is the sum of its members' sizes, i.e. it has no padding.  The member
// counts below are kept by hand - C++17 cannot enumerate a struct's members - so they are a tripwire, not a derivation: any member added to
// one of these structs changes its size and trips its line, and whoever mends the line recounts ALL members against pqp.h (an int added
// with 4 bytes of padding passes if only the double count is bumped) and puts the struct field by field if padding has appeared
static_assert(sizeof(pqp_params) == 29 * sizeof(double) + 18 * sizeof(int32_t), "pqp_params has padding");
static_assert(sizeof(pqp_corridor_params) == 11 * sizeof(double), "pqp_corridor_params has padding");
static_assert(sizeof(pqp_dp_params) == 4 * sizeof(double), "pqp_dp_params has padding");
static_assert(sizeof(pqp_grid_geometry) == 2 * sizeof(int32_t) + 5 * sizeof(double), "pqp_grid_geometry has padding");

// pqp_set_option: one int per option, nothing else - the struct goes into the chain's graph key as bytes, so every option, present or
// future, is part of it
struct Options {
    int store_warm = 1, order_by_cost = 0, reserve_cus = 0;
    int stream_batch = -1;       // (< 0: stream_batch_auto(n))
    int carry = 0;               // PQP_OPT_CARRY_CYCLES
    int stream_staged = -1;      // (< 0: by launch size, path_stream_impl)
    int chain_graph = 0;         // PQP_OPT_CHAIN_GRAPH: pqp_optimize_path_device captured as hipGraphs (pqp_chain.hip); 2: without the fences
    int long_lines = 0;          // PQP_OPT_LONG_LINES: 0 LDS forms only, 1 long form where the LDS form does not fit, 2 long forms
};
static_assert(std::has_unique_object_representations_v<Options>, "Options: ints only, no padding");

// what a changed option leaves stale on the handle (pqp_handle::invalidate)
enum Stale : unsigned {
    kStaleCostOrder = 1,         // the cost histograms / order maps of both path kernels (LanePath::hist_batch, StreamPath::order_batch)
    kStaleStreamCarry = 2,       // what the lane-per-QP kernel's workspace holds (StreamPath::last_batch)
    kStaleSmootherCarry = 4,     // the exact smoothers' carried active sets (Smoothers::act_batch)
};
// every option: its id, its member, how a value is normalised, what a change invalidates.  pqp_set_option is a walk over this table.
struct OptionRow { int id; int Options::*member; int (*normalise)(int); unsigned stale; };
inline constexpr OptionRow kOptionTable[] = {
    {PQP_OPT_STORE_WARM, &Options::store_warm, [](int v) { return v ? 1 : 0; }, 0},
    {PQP_OPT_ORDER_BY_COST, &Options::order_by_cost, [](int v) { return v ? 1 : 0; }, kStaleCostOrder},
    {PQP_OPT_RESERVE_CUS, &Options::reserve_cus, [](int v) { return v < 0 ? 0 : v; }, 0},
    {PQP_OPT_STREAM_BATCH, &Options::stream_batch, [](int v) { return v < 0 ? -1 : v; }, 0},
    {PQP_OPT_STREAM_STAGED, &Options::stream_staged, [](int v) { return v < 0 ? -1 : (v ? 1 : 0); }, kStaleStreamCarry},      // (another layout: nothing to carry)
    {PQP_OPT_CARRY_CYCLES, &Options::carry, [](int v) { return v < 0 ? 0 : (v > 64 ? 64 : v); }, kStaleStreamCarry | kStaleSmootherCarry},
    {PQP_OPT_CHAIN_GRAPH, &Options::chain_graph, [](int v) { return v == 2 ? 2 : (v ? 1 : 0); }, 0},
    {PQP_OPT_LONG_LINES, &Options::long_lines, [](int v) { return v >= 2 ? 2 : (v == 1 ? 1 : 0); }, 0},
};

}  // namespace pqp_internal

// The handle: what every launcher shares (device, parameters, stream, options, timing, marks, staging pool) and one group of state per
// launcher that owns it.  A group that decides what a launch of pqp_optimize_path_device's body enqueues says so in key(), directly
// under its fields: the chain's graph key is read off those (chain_key, pqp_chain.hip).  The groups are hidden like everything else
// behind the C ABI; only the handle's own name is the ABI's.
struct pqp_handle {
    using DevBuf = pqp_internal::DevBuf;
    using Key = pqp_internal::Key;
    int device = 0;
    int num_cu = 0;
    pqp_params prm;
    hipStream_t stream = nullptr;
    pqp_internal::Options opt;

    // HIP events around the dominant kernel of every call, on the stream it is launched on: a ring of the last kEvRing launches,
    // read back (after the work is done) by pqp_last_kernel_ms / pqp_kernel_ms_history without putting a sync between launches.
    // One slot more than the history: the one launch_timed records into, which a launch that fails may leave half recorded.
    // (no key: events are not recorded inside a capture, and a replay clears `timed`)
    struct PQP_HIDDEN Timing {
        static constexpr int kEvRing = 256, kEvSlots = kEvRing + 1;
        hipEvent_t evs0[kEvSlots] = {}, evs1[kEvSlots] = {};
        long long ev_count = 0;          // launches recorded so far
        bool timed = false;              // the last of them is what pqp_last_kernel_ms reports
        // the launches of one call between the next pair of the ring's events, which count only once the launches were accepted: a call that
        // fails leaves the timing of the previous one.  No events inside a graph capture.
        template <class F> int launch_timed(hipStream_t stream, bool capturing, F&& launch) {
            if (capturing) return launch();
            const int slot = (int)(ev_count % kEvSlots);
            PQP_HIP(hipEventRecord(evs0[slot], stream));
            if (const int rc = launch()) return rc;
            PQP_HIP(hipEventRecord(evs1[slot], stream));
            ev_count += 1;
            timed = true;
            return PQP_OK;
        }
    } timing;
    template <class F> int launch_timed(F&& launch) { return timing.launch_timed(stream, chain.capturing, launch); }

    static constexpr int kMarks = 8;
    static constexpr int kChainMarks = 2;      // + two events of pqp_optimize_path_device's own
    hipEvent_t marks[kMarks + kChainMarks] = {};   // pqp_mark / pqp_wait_mark: ordering between the streams of two handles

    // path_solve_impl (pqp_kernels.hip): the lane-per-waypoint path kernel
    struct PQP_HIDDEN LanePath {
        DevBuf wx, wy, wye, wrho, wsave, wscale;    // warm state (lane layout) + polish save area, parked Ruiz vectors (per workgroup slot)
        // work distribution of the solve kernel: ticket counter (never reset: a launch uses batch + grid tickets), cost bins of the
        // last solve and the ticket -> QP order derived from them
        DevBuf ticket, cost_key, cost_hist, order;
        unsigned long long ticket_next = 0;
        long long solves = 0;                       // solve launches so far (parity selects the cost histogram being filled)
        int hist_batch = 0, hist_n = 0;             // shape of the solve whose costs cost_key / cost_hist hold (0: none)
        int blocks_per_cu[8] = {0, 0, 0, 0, 0, 0, 0, 0};    // occupancy of the solve kernel variants [log2(nw)][cert]
        // The outcome of the handle's last path solve, whichever kernel ran it.  This is the one home of these four: path_stream_impl
        // writes them too, through solved() and nothing else (a launch of the lane-per-QP kernel keeps no warm state: stored = false).
        int warm_batch = 0, warm_n = 0;
        bool warm_stored = false;                   // the last solve wrote its final iterate to wx / wy / wye
        int last_path_kernel = 0;                   // pqp_path_kernel of the last pqp_path_solve* launch (pqp_last_path_kernel)
        void solved(int kernel, int batch, int n, bool stored) { warm_batch = batch; warm_n = n; warm_stored = stored; last_path_kernel = kernel; }
        bool warm_is(int batch, int n) const { return warm_stored && warm_batch == batch && warm_n == n; }

        // a captured launch holds: which of the two order arrays it reads (launch parity), whether it reads one at all, and the warm / carry
        // decisions of path_solve_impl (ticket_next is not in it: a captured launch resets the device counter itself)
        void key(Key& k) const {
            k.put_int(solves & 1); k.put_int(hist_batch); k.put_int(hist_n); k.put_int(warm_batch); k.put_int(warm_n); k.put_int(warm_stored ? 1 : 0);
        }

        // The host bookkeeping of a chain body around its capture and its replays (pqp_optimize_path_device).  Only a body whose path solve
        // ran on the lane-per-waypoint kernel touches the ticket counter (the graph resets it and leaves it at ticket_after) and counts solve
        // launches; a body that went to path_stream_kernel leaves both alone - plain pqp_path_solve* calls on the handle between two replays
        // keep their counter.
        struct Mark { long long solves; unsigned long long ticket_next; };
        struct Replay { long long lane_launches = 0; int path_kernel = 0; unsigned long long ticket_after = 0; };     // (lane_launches: two with second_pass = BOUNDS_ON_STATES)
        Mark mark() const { return {solves, ticket_next}; }
        // nothing of the captured body has run: undo its bookkeeping
        void rewind(const Mark& m) { solves = m.solves; ticket_next = m.ticket_next; }
        // what the capture recorded since `m`, for every replay; the launches it counted only happen then
        Replay captured(const Mark& m) { const Replay r{solves - m.solves, last_path_kernel, ticket_next}; solves = m.solves; return r; }
        // the host-side state a plain run of the body leaves (everything else the body sets is the same from call to call: it is in the key)
        void replayed(const Replay& r) {
            if (r.lane_launches) { ticket_next = r.ticket_after; solves += r.lane_launches; }
            last_path_kernel = r.path_kernel;        // (pqp_last_path_kernel: the kernel the replayed body's path solve runs on)
        }
    } lane;

    // path_stream_impl (pqp_kernels.hip): the lane-per-QP path kernel
    struct PQP_HIDDEN StreamPath {
        DevBuf ws;                                  // workspace of path_stream_kernel
        DevBuf key_buf, hist, order;                // PQP_OPT_ORDER_BY_COST on that kernel: phase keys, key histogram, two slot -> QP maps
        long long solves = 0;                       // ordered launches so far (parity selects the map being read)
        int order_batch = 0, order_n = 0;           // shape the map being read was built for (0: none)
        int last_batch = 0, last_n = 0;             // shape of the last path_stream_kernel launch (what its workspace still holds)
        // a captured launch holds the carry decision; the ordered launches are off inside a capture, so their state decides nothing there
        void key(Key& k) const { k.put_int(last_batch); k.put_int(last_n); }
    } strm;

    // pqp_smoothers.hip
    struct PQP_HIDDEN Smoothers : pqp_internal::BandedGroup {
        // smoother QPs: banded problem data + shared sparsity (cached per type and size) are the base's
        DevBuf act[2];                              // final active sets of the exact TensionSmoother / postSmooth kernels (PQP_OPT_CARRY_CYCLES)
        int act_batch[2] = {0, 0}, act_n[2] = {0, 0};
        // a captured launch holds the carry flags of the exact kernels; a structure upload cannot be captured at all (sm_upload_structure)
        void key(Key& k) const {
            k.put_int(act_batch[0]); k.put_int(act_n[0]); k.put_int(act_batch[1]); k.put_int(act_n[1]); k.put_int(struct_type); k.put_int(struct_n);
        }
    } sm;

    // pqp_speed_refine_device (pqp_speed.hip): the speed QPs' own group for the banded core, and the corridor [batch][m][3] its three
    // kernels share.  (no key: the chain runs none of it, and its structure is not the smoothers')
    struct PQP_HIDDEN Refine : pqp_internal::BandedGroup { DevBuf bounds; } rf;

    // line_launch: workspace of the long forms of the line kernels (one launch at a time on the stream).
    // (no key: which form runs follows from opt.long_lines and the call's sizes; a reallocation moves the allocation generation)
    struct PQP_HIDDEN Lines { DevBuf ws; } lines;

    // one captured chain: the key it was captured under, and what its replays do to the path handle's bookkeeping
    struct ChainGraph { Key key; hipGraphExec_t exec = nullptr; bool failed = false; LanePath::Replay replay; };
    // pqp_optimize_path_device (pqp_chain.hip).  capturing: the handle's stream is in capture mode - no timing events, the path solve
    // resets its ticket counter inside the graph.  (no key: it is the key's user)
    struct PQP_HIDDEN Chain {
        DevBuf d, i;                                // workspace (pqp_chain_ws.hpp)
        std::vector<ChainGraph> graphs;
        bool capturing = false;
    } chain;

    static constexpr int kStage = 16;           // pqp_speed_search stages the most: eight inputs, three workspaces, five outputs
    DevBuf stage[kStage];                       // device copies of the arrays of a host-pointer entry point (Staging), in argument order
                                                // (no key: the chain is a device-pointer entry point and stages nothing)

    void invalidate(unsigned stale) {
        if (stale & pqp_internal::kStaleCostOrder) { lane.hist_batch = 0; strm.order_batch = 0; }
        if (stale & pqp_internal::kStaleStreamCarry) strm.last_batch = 0;
        if (stale & pqp_internal::kStaleSmootherCarry) sm.act_batch[0] = sm.act_batch[1] = 0;
    }
};

namespace pqp_internal PQP_HIDDEN {

inline int hip_ok(hipError_t e, const char* what) { return e == hipSuccess ? PQP_OK : fail(PQP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

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

// The generic banded core on a buffer group of the handle's (pqp_smoothers.hip, where its kernels are instantiated).  kBanded*: the QP
// families whose sparsity sm_alloc knows; n: points (layers) of the pattern.
enum { kBandedTension2 = 0, kBandedTension = 1, kBandedPost = 2, kBandedRefine = 3 };
// does the core hold a QP of this family and size (its vectors, factor rows and row data in one CU's LDS, one lane per padded variable)?
bool sm_generic_fits(int type, int n);
// the group's arrays for `batch` QPs, and the family's sparsity uploaded unless the group holds it
int sm_alloc(pqp_handle* h, BandedGroup& g, int type, int batch, int n);
// one launch of banded_solve_kernel on what an assemble kernel wrote into the group, under `prm`; `timed`: between a pair of the
// handle's timing events of its own (a caller that times a longer sequence passes false)
int sm_solve(pqp_handle* h, BandedGroup& g, const pqp_params& prm, int type, int batch, int n, const int32_t* n_of, int32_t* status, int32_t* iters,
             double* info, bool timed);

// PQP_OPT_CARRY_CYCLES for an exact smoother kernel (slot 0: TensionSmoother, 1: postSmooth): the active set every scenario ended with is kept
// on the handle; a solve of the shape of the previous one (and the buffer still where it was) starts from it (carry = 1)
inline int sm_carry_slot(pqp_handle* h, int slot, int batch, int n, signed char*& act_io, int& carry) {
    act_io = nullptr;
    carry = 0;
    if (!h->opt.carry) return PQP_OK;
    const void* before = h->sm.act[slot].p;
    int rc;
    if ((rc = h->sm.act[slot].ensure((size_t)batch * n))) return rc;
    act_io = h->sm.act[slot].as<signed char>();
    carry = (h->sm.act_batch[slot] == batch && h->sm.act_n[slot] == n && before == h->sm.act[slot].p) ? 1 : 0;
    h->sm.act_batch[slot] = batch; h->sm.act_n[slot] = n;
    return PQP_OK;
}

// One launch of an exact smoother kernel (tension_exact_kernel / post_exact_kernel) on n elements per scenario: launch(K, ws) with K = the fewest
// chunks of 64 per lane that hold them (SmRegs<K>), or K = 0 beyond 1024 with `arrays` workspace arrays per scenario in HBM (SmHbm, ws).
// (twelve / sixteen per lane: the lane state no longer fits the registers - S2 1.8 / 3.3 KB of scratch per lane - but lines that long are rare,
//  a point per metre of reference line, and the recursion down the lanes, not the spills, is what their time goes to)
template <class F>
int sm_exact_launch(pqp_handle* h, int batch, int n, int arrays, F&& launch) {
    int rc;
    if (n > 1024 && (rc = h->sm.pband.ensure((size_t)batch * arrays * (64 * (((size_t)n + 63) / 64)) * 8))) return rc;
    double* ws = n > 1024 ? h->sm.pband.as<double>() : nullptr;
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
int line_launch(pqp_handle* h, const void* fn, size_t lds, const char* who, size_t ws_bytes, F&& launch, const void* long_fn = nullptr,
                size_t long_lds = 0, const char* long_who = nullptr) {
    bool go_long = false;
    int rc = long_form(h->opt.long_lines, fn, lds, &go_long);
    if (!rc && !go_long) rc = lds_opt_in(fn, lds, who);
    if (!rc && go_long && long_fn) rc = lds_opt_in(long_fn, long_lds, long_who);
    if (!rc && go_long && ws_bytes) rc = h->lines.ws.ensure(ws_bytes);
    if (rc) return rc;
    double* ws = h->lines.ws.as<double>();
    return h->launch_timed([&]() -> int {
        if (go_long) launch(std::true_type(), ws);
        else launch(std::false_type(), ws);
        PQP_HIP(hipGetLastError());
        return PQP_OK;
    });
}

// a distance-map layer the kernels can index with 32 bits (obstacle_distance, pqp_line_device.hpp)
inline bool geometry_ok(const pqp_grid_geometry* g) {
    return g && g->rows >= 2 && g->cols >= 2 && g->resolution > 0.0 && (long long)g->rows * g->cols < (1ll << 30);
}

// ---- what the entry points of the planning stages share (pqp_maps.hip, pqp_agents.hip, pqp_speed.hip, pqp_select.hip) -----------------
// the grid of a kernel that gives every item a wavefront, threads / 64 of them to a workgroup
inline dim3 wave_grid(long long items, int threads) {
    const int per_block = threads / 64;
    return dim3((unsigned)((items + per_block - 1) / per_block));
}

// an optional index array of a host form: every entry inside [0, count), or the refusal `what`
inline int index_range(const int32_t* of, int batch, int count, const char* what) {
    if (of)
        for (int b = 0; b < batch; ++b)
            if (of[b] < 0 || of[b] >= count) return fail(PQP_ERR_INVALID, what);
    return PQP_OK;
}

inline bool car_ok(const pqp_car_geometry* c) {
    return c && std::isfinite(c->width) && std::isfinite(c->rear_length) && std::isfinite(c->front_length);
}
// the car's circles as the kernels take them (pqp_car_circles.hpp); beside pqp_car_circles in pqp_maps.hip
int car_circles_of(const pqp_car_geometry* car, pqp::CarCircles* c);

// The predicted rows [n_scenes][a_max][steps >= 1] of a stage that tests against agents (the agent check, the overlay, the speed search)
// or writes them (the prediction).  (the frames' launch is one block per 256 rows in x: 2^38 rows are 2^30 blocks, and 16 TiB of frames)
inline bool agent_rows_ok(int n_scenes, int a_max, int steps, const double* agents) {
    return n_scenes >= 1 && a_max >= 0 && (long long)n_scenes * a_max <= (1ll << 38) / steps && (agents || a_max == 0);
}
// agent_frames_kernel over every (scene, agent, step) row into `frames`, inside a launch_timed; the kernel and this are pqp_agents.hip's
int launch_agent_frames(pqp_handle* h, int n_scenes, int a_max, int m, const double* agents, double* frames);
// the device copies of those rows in a host form: the rows, the scenes' counts, the stage's own index array `of` [n_of] (scene_of, base_of)
// and the frames scratch, in the pool order of all three stages; no rows: neither they nor the frames take a slot
struct AgentArrays { const double* agents; const int32_t* a_of; const int32_t* of; double* frames; };
inline AgentArrays stage_agents(Staging& st, int n_scenes, int a_max, int steps, const double* agents, const int32_t* a_of, const int32_t* of,
                                size_t n_of) {
    const size_t rows = (size_t)n_scenes * a_max * steps;
    AgentArrays d;
    d.agents = rows ? st.in(agents, rows * PQP_AGENT_STRIDE) : nullptr;
    d.a_of = st.in(a_of, n_scenes);
    d.of = st.in(of, n_of);
    d.frames = rows ? st.out((double*)nullptr, rows * PQP_AGENT_FRAME_STRIDE) : nullptr;
    return d;
}

// a selector's group_start [groups + 1] in its host form: from 0 to batch, ascending, or the refusal under the entry point's name `who`
inline int group_start_ok(const char* who, const int32_t* group_start, int groups, int batch) {
    if (group_start[0] != 0 || group_start[groups] != batch) return fail(PQP_ERR_INVALID, std::string(who) + ": group_start must run from 0 to batch");
    for (int g = 0; g < groups; ++g)
        if (group_start[g + 1] < group_start[g]) return fail(PQP_ERR_INVALID, std::string(who) + ": group_start must be ascending");
    return PQP_OK;
}

}  // namespace pqp_internal
