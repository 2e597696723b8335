// pqp_wrapper_detail.hpp — PathOptimizationNS::detail: what the header-only wrappers over the C ABI (pqp_*.hpp) share, stated once.
// Ragged batches to the zero-filled arrays the C ABI takes, the row layouts a state is written to and read from, the agents of many
// scenes as PQP_AGENT_STRIDE rows and back, and the handle a wrapper owns.  Templates over the state type, so the wrappers' own types and,
// with PQP_USE_REFERENCE_TYPES, the reference's serve alike.  No HIP runtime here: the device arrays are in pqp_wrapper_device.hpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "pqp.h"

namespace PathOptimizationNS {

// an agent at one time step: a rectangle of half_length x half_width around (x, y), turned by heading and rounded by radius (a disc:
// half_length = half_width = 0).  half_length < 0 or half_width < 0: not there at that step
struct PredictedAgent {
    double x{}, y{}, heading{}, half_length{}, half_width{}, radius{};
};
using StandingAgent = PredictedAgent;          // the row pqp_overlay_agents reads is the same row, at one step

namespace detail {

// the longest inner vector, at least `least`
template <class T>
size_t longest(const std::vector<std::vector<T>>& batch, size_t least = 1) {
    for (const auto& v : batch) least = std::max(least, v.size());
    return least;
}

struct Packed {
    size_t n = 0;                       // rows per inner vector: longest()
    std::vector<double> rows;           // [batch][n][stride], zeros where write() put nothing
    std::vector<int32_t> count;         // [batch]: the inner vectors' sizes
};

// write(element, its index in the inner vector, its row) for every element of a ragged batch
template <class T, class Writer>
Packed pack(const std::vector<std::vector<T>>& batch, size_t stride, Writer write, size_t least = 1) {
    Packed p;
    p.n = longest(batch, least);
    p.rows.assign(batch.size() * p.n * stride, 0.0);
    p.count.resize(batch.size());
    for (size_t b = 0; b < batch.size(); ++b) {
        p.count[b] = (int32_t)batch[b].size();
        for (size_t i = 0; i < batch[b].size(); ++i) write(batch[b][i], i, &p.rows[(b * p.n + i) * stride]);
    }
    return p;
}

// The row layouts: a writer for pack(), and the reader of the same columns.

struct PoseRow {            // [3]: x, y, heading
    template <class S> void operator()(const S& s, size_t, double* r) const { r[0] = s.x; r[1] = s.y; r[2] = s.heading; }
    template <class S> static void read(const double* r, S* s) { s->x = r[0]; s->y = r[1]; s->heading = r[2]; }
};

struct PathRow {            // [6]: x, y, heading, ., ., k (pqp_speed_profile reads no heading: SpeedProfiler leaves that column 0)
    bool heading = true;
    template <class S> void operator()(const S& s, size_t, double* r) const { r[0] = s.x; r[1] = s.y; r[2] = heading ? s.heading : 0.0; r[5] = s.k; }
    template <class S> static void read(const double* r, S* s) { s->x = r[0]; s->y = r[1]; s->heading = r[2]; s->k = r[5]; }
};

struct ProfileRow {         // [PQP_SPEED_STRIDE], beside a path row: s, v, a, . (the time: the caller's)
    template <class S> void operator()(const S& s, size_t, double* r) const { r[0] = s.s; r[1] = s.v; r[2] = s.a; }
    template <class S> static void read(const double* r, S* s) { s->s = r[0]; s->v = r[1]; s->a = r[2]; }
};

struct TrajRow {            // [PQP_TRAJ_STRIDE]: x, y, heading, k, s, v, a, . (the time column left 0)
    template <class S> void operator()(const S& s, size_t, double* r) const {
        r[0] = s.x; r[1] = s.y; r[2] = s.heading; r[3] = s.k; r[4] = s.s; r[5] = s.v; r[6] = s.a;
    }
    template <class S> static S read(const double* r) {          // the time is r[7]
        S st{};
        st.x = r[0]; st.y = r[1]; st.heading = r[2]; st.k = r[3]; st.s = r[4]; st.v = r[5]; st.a = r[6];
        return st;
    }
};

struct TimedTrajRow {       // the same with t = index * dt in column 7
    double dt;
    template <class S> void operator()(const S& s, size_t f, double* r) const { TrajRow()(s, f, r); r[7] = (double)f * dt; }
};

// the first count[b] rows of every [n][PQP_TRAJ_STRIDE] block as states
template <class S>
void read_trajectories(const std::vector<double>& rows, size_t n, const std::vector<int32_t>& count, std::vector<std::vector<S>>* out) {
    out->assign(count.size(), std::vector<S>());
    for (size_t b = 0; b < count.size(); ++b)
        for (size_t f = 0; f < (size_t)std::max(count[b], 0); ++f) (*out)[b].push_back(TrajRow::read<S>(&rows[(b * n + f) * PQP_TRAJ_STRIDE]));
}

// Agent scenes.

struct AgentRows {
    size_t a_max = 0;                   // the most agents of a scene
    std::vector<double> rows;           // [scenes][a_max][m][PQP_AGENT_STRIDE]
    std::vector<int32_t> a_of;          // [scenes]: the agents of every scene
};

// at(agent, k): the agent at step k, or nullptr.  Where there is none - behind an agent's last step, behind a scene's last agent - the
// row is the absent one as pqp_predict_agents writes it: (0, 0, 0, -1, -1, 0)
template <class Agent, class At>
AgentRows pack_agents(const std::vector<std::vector<Agent>>& scenes, size_t m, At at) {
    AgentRows out;
    out.a_max = longest(scenes, 0);
    out.rows.resize(scenes.size() * out.a_max * m * PQP_AGENT_STRIDE);
    out.a_of.resize(scenes.size());
    double* r = out.rows.data();
    for (size_t s = 0; s < scenes.size(); ++s) {
        out.a_of[s] = (int32_t)scenes[s].size();
        for (size_t a = 0; a < out.a_max; ++a)
            for (size_t k = 0; k < m; ++k, r += PQP_AGENT_STRIDE) {
                const PredictedAgent* p = a < scenes[s].size() ? at(scenes[s][a], k) : nullptr;
                if (p) { r[0] = p->x; r[1] = p->y; r[2] = p->heading; r[3] = p->half_length; r[4] = p->half_width; r[5] = p->radius; }
                else { r[0] = r[1] = r[2] = r[5] = 0.0; r[3] = r[4] = -1.0; }
            }
    }
    return out;
}

// [scene][agent][step] at m steps
inline AgentRows pack_agents(const std::vector<std::vector<std::vector<PredictedAgent>>>& scenes, size_t m) {
    return pack_agents(scenes, m, [](const std::vector<PredictedAgent>& a, size_t k) { return k < a.size() ? &a[k] : nullptr; });
}

// [scene][agent] at one step
inline AgentRows pack_agents(const std::vector<std::vector<PredictedAgent>>& scenes) {
    return pack_agents(scenes, 1, [](const PredictedAgent& a, size_t) { return &a; });
}

// the inverse: a_of[s] agents of m steps each out of rows [scenes][a_max][m][PQP_AGENT_STRIDE]
inline void unpack_agents(const std::vector<double>& rows, const std::vector<int32_t>& a_of, size_t a_max, size_t m,
                          std::vector<std::vector<std::vector<PredictedAgent>>>* scenes) {
    scenes->assign(a_of.size(), {});
    for (size_t s = 0; s < a_of.size(); ++s) {
        (*scenes)[s].assign(a_of[s], std::vector<PredictedAgent>(m));
        for (size_t a = 0; a < (size_t)a_of[s]; ++a)
            for (size_t k = 0; k < m; ++k) {
                const double* r = &rows[((s * a_max + a) * m + k) * PQP_AGENT_STRIDE];
                (*scenes)[s][a][k] = PredictedAgent{r[0], r[1], r[2], r[3], r[4], r[5]};
            }
    }
}

// The handle of a wrapper that keeps its own (max_batch 1, max_n 2: the stages size their own buffers).  wanted = false: none is made
class OwnedHandle {
 public:
    explicit OwnedHandle(int device, bool wanted = true) { ok_ = wanted && pqp_create(&h_, nullptr, device, 1, 2) == PQP_OK; }
    OwnedHandle(const OwnedHandle&) = delete;
    OwnedHandle& operator=(const OwnedHandle&) = delete;
    ~OwnedHandle() { if (h_) pqp_destroy(h_); }
    bool ok() const { return ok_; }
    pqp_handle* get() const { return h_; }
    void* stream() const {              // a hipStream_t
        void* s = nullptr;
        if (ok_) pqp_get_stream(h_, &s);
        return s;
    }

 private:
    pqp_handle* h_ = nullptr;
    bool ok_ = false;
};

}  // namespace detail
}  // namespace PathOptimizationNS
