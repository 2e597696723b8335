// look_emu.cpp — TEST INFRASTRUCTURE: the host emulation (lane_emu.cpp, included whole) with PathQp::run()'s look hook armed.  After every polish solve
// the values the fused look (iterate(true) + look_after_solve()) hands the policy are compared, bit for bit, with what residuals() returns on the
// same state.  Built only by tests/test_fused_look_emulation.py.
#include <cstdint>
#include <cstring>
#include <type_traits>

namespace {
long long g_looks[2] = {0, 0}, g_mismatch[2] = {0, 0};      // [0] lazy looks (four values), [1] full looks (six)
double g_first[12];                                        // the first mismatch: what the look gave (padded with 0), what residuals() gives
template <class PQ, class V> void look_check(PQ& pq, const V& v);
}  // namespace
#define PQP_LOOK_HOOK(k, v) look_check(*this, v)

#include "lane_emu.cpp"

namespace {
template <class PQ, class V>
void look_check(PQ& pq, const V& v) {
    double ref[6], got[6] = {0, 0, 0, 0, 0, 0}, want[6] = {0, 0, 0, 0, 0, 0};
    pq.residuals(ref);       // (touches only the exchange buffers a look may use: the run goes on as it would have)
    int kind, k;
    if constexpr (std::is_same<V, typename PQ::LazyLook>::value) {
        kind = 0; k = 4;
        got[0] = v.pr; got[1] = v.du; got[2] = v.bad; got[3] = v.viol;
        want[0] = ref[0]; want[1] = ref[1]; want[2] = ref[4]; want[3] = ref[5];
    } else {
        kind = 1; k = 6;
        for (int j = 0; j < 6; ++j) { got[j] = v[j]; want[j] = ref[j]; }
    }
    g_looks[kind] += 1;
    if (std::memcmp(got, want, sizeof(double) * k) != 0) {
        if (g_mismatch[0] + g_mismatch[1] == 0) { std::memcpy(g_first, got, sizeof(got)); std::memcpy(g_first + 6, want, sizeof(want)); }
        g_mismatch[kind] += 1;
    }
}
}  // namespace

extern "C" void pqp_emu_look_counts(long long* looks, long long* mismatch, double* first, int reset) {
    for (int k = 0; k < 2; ++k) { looks[k] = g_looks[k]; mismatch[k] = g_mismatch[k]; }
    std::memcpy(first, g_first, sizeof(g_first));
    if (reset) { g_looks[0] = g_looks[1] = g_mismatch[0] = g_mismatch[1] = 0; std::memset(g_first, 0, sizeof(g_first)); }
}
