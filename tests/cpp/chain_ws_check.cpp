// The chain's workspace layout (csrc/pqp_chain_ws.hpp) on the host: for every (batch, R, S, L, N, second) of the set below the measured
// sizes equal the closed forms the layout had when it was a formula beside a list of takes - the recorded expectation -
//     per scenario 12 R + 18 S + 16 L + 11 N + 25 doubles and 14 ints, + 3 N doubles and 7 ints with second_pass = BOUNDS_ON_STATES,
// and the arrays carved from buffers of exactly the measured bytes are pairwise disjoint, tile both buffers without gap or overhang, and
// every double array is 8-byte aligned.  Every array is written over its full extent (a sanitizer build sees an overhang as it happens).
// Plain C++, nothing of HIP: prints "ok <cases>" and exits 0, or says what failed and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../path_optimizer_2_amd/csrc/pqp_chain_ws.hpp"

using namespace pqp_internal;

struct Span { const char* name; size_t begin, end; bool is_double; };

static int fail(const char* what, const ChainDims& c, size_t batch, const char* name = "") {
    std::printf("FAILED: %s %s (batch %zu R %d S %d L %d N %d second %d)\n", what, name, batch, c.R, c.S, c.L, c.N, (int)c.second);
    return 1;
}

static int check(size_t batch, ChainDims c) {
    ChainWs w;
    const ChainWsSize need = carve(w, c, batch, nullptr, nullptr);
    const size_t R = c.R, S = c.S, L = c.L, N = c.N;
    const size_t want_d = batch * (12 * R + 18 * S + 16 * L + 11 * N + 25 + (c.second ? 3 * N : 0)), want_i = batch * (14 + (c.second ? 7 : 0));
    if (need.doubles != want_d) return fail("doubles differ from the closed form", c, batch);
    if (need.ints != want_i) return fail("ints differ from the closed form", c, batch);
    double* d = (double*)std::malloc(need.doubles * sizeof(double));
    int32_t* i = (int32_t*)std::malloc(need.ints * sizeof(int32_t));
    if (!d || !i) return fail("malloc", c, batch);
    const ChainWsSize used = carve(w, c, batch, d, i);
    if (used.doubles != need.doubles || used.ints != need.ints) return fail("the second carve took another size than the first measured", c, batch);
    std::vector<Span> spans;
    int arrays = 0, rc = 0;
    chain_ws_arrays(w, c, [&](const char* name, auto*& p, size_t per) {
        using T = std::remove_pointer_t<std::remove_reference_t<decltype(p)>>;
        constexpr bool is_double = std::is_same_v<T, double>;
        ++arrays;
        if (!p) { rc |= fail("null pointer", c, batch, name); return; }
        if (is_double && (uintptr_t)p % 8 != 0) rc |= fail("double array not 8-byte aligned", c, batch, name);
        for (size_t k = 0; k < batch * per; ++k) p[k] = (T)arrays;                     // the full extent
        const size_t begin = (size_t)((const char*)p - (is_double ? (const char*)d : (const char*)i));
        spans.push_back({name, begin, begin + batch * per * sizeof(T), is_double});
    });
    if (arrays != (c.second ? 56 : 48)) rc |= fail("array count", c, batch);
    // pairwise disjoint, and together exactly the buffer: sorted by begin, each starts where the previous one ended
    for (const bool dbl : {true, false}) {
        std::vector<Span> v;
        for (const Span& s : spans) if (s.is_double == dbl) v.push_back(s);
        std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.begin < b.begin; });
        size_t at = 0;
        for (const Span& s : v) {
            if (s.begin < at) rc |= fail("overlaps the array before it", c, batch, s.name);
            if (s.begin > at) rc |= fail("gap before", c, batch, s.name);
            at = s.end;
        }
        if (at != (dbl ? need.doubles * sizeof(double) : need.ints * sizeof(int32_t))) rc |= fail(dbl ? "doubles do not end with their buffer" : "ints do not end with their buffer", c, batch);
    }
    // nothing written through one array shows in another
    int seen = 0;
    chain_ws_arrays(w, c, [&](const char* name, auto*& p, size_t per) {
        using T = std::remove_pointer_t<std::remove_reference_t<decltype(p)>>;
        ++seen;
        for (size_t k = 0; k < batch * per; ++k) if (p[k] != (T)seen) { rc |= fail("overwritten through another array", c, batch, name); break; }
    });
    // the arrays of the second pass exist with it alone
    if (!c.second && (w.lin || w.n_valid2 || w.n_of2 || w.qp_status2 || w.iters1 || w.iters2 || w.n_valid_out || w.status_out)) rc |= fail("second-pass array without the second pass", c, batch);
    std::free(d); std::free(i);
    return rc;
}

int main() {
    const int caps[][4] = {{160, 128, 96, 256}, {64, 48, 32, 128}, {8, 4, 4, 2}};        // the defaults, the tests', the minimum
    const size_t batches[] = {1, 40};
    int cases = 0;
    for (const auto& k : caps)
        for (const size_t batch : batches)
            for (const bool second : {false, true}) {
                if (check(batch, ChainDims{k[0], k[1], k[2], k[3], second})) return 1;
                ++cases;
            }
    std::printf("ok %d\n", cases);
    return 0;
}
