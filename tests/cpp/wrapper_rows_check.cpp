// wrapper_rows_check.cpp — what the C++ wrappers share (include/pqp_wrapper_detail.hpp), checked on the host alone: ragged batches, the row
// layouts there and back, agent scenes there and back.  No library, no GPU: build with -fsanitize=address,undefined and run.
// Prints "ok N" for N cases, or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pqp_types.hpp"
#include "pqp_wrapper_detail.hpp"

using namespace PathOptimizationNS;
namespace d = PathOptimizationNS::detail;

static int cases = 0;
#define CHECK(c) do { if (!(c)) { std::printf("case %d, line %d: %s\n", cases + 1, __LINE__, #c); std::exit(1); } } while (0)

// a state whose every field is its own number, from the batch index b and the element index i
static SlState state(size_t b, size_t i) {
    SlState s;
    const double o = 100.0 * (double)b + 10.0 * (double)i;
    s.x = o + 1; s.y = o + 2; s.heading = o + 3; s.k = o + 4; s.d_k = o + 5; s.s = o + 6; s.v = o + 7; s.a = o + 8; s.l = o + 9; s.d_heading = o + 9.5;
    return s;
}

static std::vector<std::vector<SlState>> ragged(const std::vector<size_t>& sizes) {
    std::vector<std::vector<SlState>> batch(sizes.size());
    for (size_t b = 0; b < sizes.size(); ++b)
        for (size_t i = 0; i < sizes[b]; ++i) batch[b].push_back(state(b, i));
    return batch;
}

static const std::vector<size_t> SIZES = {0, 1, 3, 2};

// a layout on the 0-1-3-2 batch: the shape, the counts, the columns in `carried` as same() finds them after the reader, zeros elsewhere
template <class Writer, class Same>
static void layout(size_t stride, Writer write, const std::vector<int>& carried, Same same) {
    const auto batch = ragged(SIZES);
    const d::Packed p = d::pack(batch, stride, write);
    CHECK(p.n == 3 && p.rows.size() == SIZES.size() * 3 * stride && p.count.size() == SIZES.size());
    for (size_t b = 0; b < SIZES.size(); ++b) {
        CHECK(p.count[b] == (int32_t)SIZES[b]);
        for (size_t i = 0; i < p.n; ++i) {
            const double* r = &p.rows[(b * p.n + i) * stride];
            for (size_t c = 0; c < stride; ++c) {
                bool is_carried = false;
                for (int k : carried) is_carried |= (size_t)k == c;
                if (i >= SIZES[b] || !is_carried) CHECK(r[c] == 0.0);
                else CHECK(r[c] != 0.0);
            }
            if (i < SIZES[b]) CHECK(same(batch[b][i], r, i));
        }
    }
    ++cases;
}

static PredictedAgent agent(size_t s, size_t a, size_t k) {
    const double o = 100.0 * (double)s + 10.0 * (double)a + (double)k;
    return PredictedAgent{o + 0.1, o + 0.2, o + 0.3, o + 0.4, o + 0.5, o + 0.6};
}

static bool same_agent(const PredictedAgent& p, const PredictedAgent& q) {
    return p.x == q.x && p.y == q.y && p.heading == q.heading && p.half_length == q.half_length && p.half_width == q.half_width && p.radius == q.radius;
}

static bool absent(const double* r) { return r[0] == 0.0 && r[1] == 0.0 && r[2] == 0.0 && r[3] == -1.0 && r[4] == -1.0 && r[5] == 0.0; }

typedef std::vector<std::vector<std::vector<PredictedAgent>>> Scenes;

// steps[s][a]: the steps of agent a of scene s
static Scenes scenes_of(const std::vector<std::vector<size_t>>& steps) {
    Scenes scenes(steps.size());
    for (size_t s = 0; s < steps.size(); ++s) {
        scenes[s].resize(steps[s].size());
        for (size_t a = 0; a < steps[s].size(); ++a)
            for (size_t k = 0; k < steps[s][a]; ++k) scenes[s][a].push_back(agent(s, a, k));
    }
    return scenes;
}

// packed at m steps: a_of and a_max, every row either the agent's own or the absent one - exactly from where the agent, or the scene, ends -
// and the inverse gives every agent back with m steps, the absent rows behind its own
static void agent_scenes(const std::vector<std::vector<size_t>>& steps, size_t m, size_t a_max) {
    const Scenes scenes = scenes_of(steps);
    const d::AgentRows ag = d::pack_agents(scenes, m);
    CHECK(ag.a_max == a_max && ag.a_of.size() == steps.size() && ag.rows.size() == steps.size() * a_max * m * PQP_AGENT_STRIDE);
    for (size_t s = 0; s < steps.size(); ++s) {
        CHECK(ag.a_of[s] == (int32_t)steps[s].size());
        for (size_t a = 0; a < a_max; ++a)
            for (size_t k = 0; k < m; ++k) {
                const double* r = &ag.rows[((s * a_max + a) * m + k) * PQP_AGENT_STRIDE];
                if (a < steps[s].size() && k < steps[s][a]) CHECK(same_agent(scenes[s][a][k], PredictedAgent{r[0], r[1], r[2], r[3], r[4], r[5]}));
                else CHECK(absent(r));
            }
    }
    Scenes back;
    d::unpack_agents(ag.rows, ag.a_of, ag.a_max, m, &back);
    CHECK(back.size() == scenes.size());
    for (size_t s = 0; s < steps.size(); ++s) {
        CHECK(back[s].size() == scenes[s].size());
        for (size_t a = 0; a < steps[s].size(); ++a) {
            CHECK(back[s][a].size() == m);
            for (size_t k = 0; k < m; ++k)
                if (k < steps[s][a]) CHECK(same_agent(back[s][a][k], scenes[s][a][k]));
                else CHECK(back[s][a][k].half_length < 0.0 && back[s][a][k].half_width < 0.0);
        }
    }
    ++cases;
}

int main() {
    // ragged batches: the longest inner vector, and the floor of 1 (and of 0, where it is asked for: the agents of a scene)
    CHECK(d::longest(ragged(SIZES)) == 3);
    ++cases;
    CHECK(d::longest(ragged({0})) == 1 && d::longest(ragged({0}), 0) == 0 && d::longest(ragged({})) == 1);
    const d::Packed one = d::pack(ragged({0}), 3, d::PoseRow());
    CHECK(one.n == 1 && one.rows == std::vector<double>(3, 0.0) && one.count == std::vector<int32_t>(1, 0));
    ++cases;

    // the row layouts, each written and read back
    layout(3, d::PoseRow(), {0, 1, 2}, [](const SlState& s, const double* r, size_t) {
        SlState q;
        d::PoseRow::read(r, &q);
        return q.x == s.x && q.y == s.y && q.heading == s.heading && q.k == 0.0;
    });
    layout(6, d::PathRow(), {0, 1, 2, 5}, [](const SlState& s, const double* r, size_t) {
        SlState q;
        d::PathRow::read(r, &q);
        return q.x == s.x && q.y == s.y && q.heading == s.heading && q.k == s.k && q.s == 0.0;
    });
    layout(6, d::PathRow{false}, {0, 1, 5}, [](const SlState& s, const double* r, size_t) {
        SlState q;
        d::PathRow::read(r, &q);
        return q.x == s.x && q.y == s.y && q.heading == 0.0 && q.k == s.k;
    });
    layout(PQP_SPEED_STRIDE, d::ProfileRow(), {0, 1, 2}, [](const SlState& s, const double* r, size_t) {
        SlState q;
        d::ProfileRow::read(r, &q);
        return q.s == s.s && q.v == s.v && q.a == s.a && q.x == 0.0;
    });
    const auto same_traj = [](const SlState& s, const double* r) {
        const State q = d::TrajRow::read<State>(r);
        return q.x == s.x && q.y == s.y && q.heading == s.heading && q.k == s.k && q.s == s.s && q.v == s.v && q.a == s.a && q.d_k == 0.0;
    };
    layout(PQP_TRAJ_STRIDE, d::TrajRow(), {0, 1, 2, 3, 4, 5, 6}, [&](const SlState& s, const double* r, size_t) { return same_traj(s, r) && r[7] == 0.0; });
    // the time column: index * dt, which is 0 - and so "not carried" to layout() - at index 0 only
    {
        const auto batch = ragged(SIZES);
        const d::Packed p = d::pack(batch, PQP_TRAJ_STRIDE, d::TimedTrajRow{0.25});
        CHECK(p.n == 3 && p.rows.size() == SIZES.size() * 3 * PQP_TRAJ_STRIDE);
        for (size_t b = 0; b < SIZES.size(); ++b)
            for (size_t i = 0; i < p.n; ++i) {
                const double* r = &p.rows[(b * p.n + i) * PQP_TRAJ_STRIDE];
                if (i < SIZES[b]) CHECK(same_traj(batch[b][i], r) && r[7] == (double)i * 0.25);
                else for (int c = 0; c < PQP_TRAJ_STRIDE; ++c) CHECK(r[c] == 0.0);
            }
        std::vector<std::vector<SlState>> back;
        d::read_trajectories(p.rows, p.n, p.count, &back);
        CHECK(back.size() == batch.size());
        for (size_t b = 0; b < SIZES.size(); ++b) {
            CHECK(back[b].size() == SIZES[b]);
            for (size_t i = 0; i < SIZES[b]; ++i) CHECK(same_traj(batch[b][i], &p.rows[(b * p.n + i) * PQP_TRAJ_STRIDE]) && back[b][i].x == batch[b][i].x && back[b][i].a == batch[b][i].a);
        }
        ++cases;
    }

    // agent scenes
    agent_scenes({{3, 1, 0}}, 3, 3);
    agent_scenes({{}, {2, 2}}, 2, 2);
    agent_scenes({{}, {}}, 3, 0);
    // the one-step form: [scene][agent], a scene with fewer agents ends in absent rows
    {
        const std::vector<std::vector<StandingAgent>> standing = {{agent(0, 0, 0)}, {}, {agent(2, 0, 0), agent(2, 1, 0)}};
        const d::AgentRows ag = d::pack_agents(standing);
        CHECK(ag.a_max == 2 && ag.a_of == std::vector<int32_t>({1, 0, 2}) && ag.rows.size() == 3 * 2 * PQP_AGENT_STRIDE);
        for (size_t s = 0; s < 3; ++s)
            for (size_t a = 0; a < 2; ++a) {
                const double* r = &ag.rows[(s * 2 + a) * PQP_AGENT_STRIDE];
                if (a < standing[s].size()) CHECK(same_agent(standing[s][a], PredictedAgent{r[0], r[1], r[2], r[3], r[4], r[5]}));
                else CHECK(absent(r));
            }
        ++cases;
    }
    std::printf("ok %d\n", cases);
    return 0;
}
