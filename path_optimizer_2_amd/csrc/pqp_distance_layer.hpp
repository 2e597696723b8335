// pqp_distance_layer.hpp — the per-line routines of pqp_distance_layer (exact Euclidean distance transform of an occupancy grid,
// cv::distanceTransform(obstacle, dist, CV_DIST_L2, CV_DIST_MASK_PRECISE); dist *= resolution, reference src/test/demo.cpp:104-113).
// Shared source of the two kernels of pqp_distance_kernels.inc and of the host build tests/emu/edt_emu.cpp.
//
// Layout: a map is [cols][rows], rows contiguous (Eigen's column-major order of grid_map's layers).  Separable and linear in the cells:
//   phase A  along rows: g(r, c) = distance to the nearest obstacle of column line c (kNoObstacle when the line has none);
//   phase B  across columns, per row r: d2(r, c) = min over c' of g(r, c')^2 + (c - c')^2, the lower envelope of parabolas
//            (Meijster, Roerdink & Hesselink 2000; Felzenszwalb & Huttenlocher 2012), then dist = fl32(fl32(sqrt(d2)) * fl32(resolution)).
// g lives in the dist buffer itself (int32 bits) between the phases, and phase B keeps its envelope stack in its own line of that buffer
// (entry k at column k, a column already read; see envelope_line): the transform needs no workspace.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifndef PQP_HD
#if defined(__HIPCC__)
#define PQP_HD __host__ __device__ __forceinline__
#else
#define PQP_HD inline
#endif
#endif
#if defined(__HIPCC__)
#define PQP_EDT_UNROLL _Pragma("unroll")
#else
#define PQP_EDT_UNROLL
#endif

namespace pqp {
namespace edt {

constexpr int32_t kNoObstacle = -1;      // g of a column line without obstacle

PQP_HD int ctz64(uint64_t m) { return __builtin_ctzll(m); }
PQP_HD int clz64(uint64_t m) { return __builtin_clzll(m); }

// ---- phase A --------------------------------------------------------------------------------------------------------------------
// One column line of `rows` cells in blocks of 64.  mask_at(base): bit i set iff cell base + i (< rows) is an obstacle (on the device one
// ballot of a wavefront); emit(base, mask, prev, next) writes the block: prev = last obstacle before base, next = first obstacle at or
// after base + 64 ("none": farther than any cell).  Every block is loaded once, plus once more when it lies in a free stretch that a
// block in front of it searched for its next obstacle (that search resumes where the last one ended: linear in the line).
template <class MaskAt, class Emit>
PQP_HD void obstacle_line(int rows, MaskAt&& mask_at, Emit&& emit) {
    const int none_prev = -1 - rows, none_next = 2 * rows;
    int prev = none_prev, next = -1;
    uint64_t cur = mask_at(0);
    for (int base = 0; base < rows; base += 64) {
        const uint64_t ahead = base + 64 < rows ? mask_at(base + 64) : 0;
        if (next < base + 64) {               // the next obstacle found so far lies in this block or before it: look further
            next = none_next;
            if (ahead) next = base + 64 + ctz64(ahead);
            else
                for (int p = base + 128; p < rows; p += 64) {
                    const uint64_t m = mask_at(p);
                    if (m) { next = p + ctz64(m); break; }
                }
        }
        emit(base, cur, prev, next);
        if (cur) prev = base + 63 - clz64(cur);
        cur = ahead;
    }
}

// g of cell base + lane of a block (prev / next as obstacle_line passes them)
PQP_HD int32_t cell_g(int rows, int base, int lane, uint64_t mask, int prev, int next) {
    const int r = base + lane;
    const uint64_t at_or_after = mask & (~0ull << lane), at_or_before = mask & (~0ull >> (63 - lane));
    const int p = at_or_before ? base + 63 - clz64(at_or_before) : prev;
    const int n = at_or_after ? base + ctz64(at_or_after) : next;
    const int g = r - p < n - r ? r - p : n - r;
    return g >= rows ? kNoObstacle : g;
}

// ---- the float conversion ---------------------------------------------------------------------------------------------------------
// sqrt(d2) rounded to the nearest float (ties to even).  Below 2^50 the double square root, rounded to float, is that value: a float
// rounding boundary m (25 significant bits) with m^2 != d2 lies at least 2^-51 m from sqrt(d2), beyond the double's own error.  Above
// (a map side beyond 2^25 cells) the float estimate is corrected by comparing d2 with the squares of the two midpoints, in integers.
PQP_HD uint64_t sq_scaled(uint64_t a, int e) { return e >= 0 ? (a * a) << (2 * e) : (a * a) >> (-2 * e); }    // (a * 2^e)^2, exact here
PQP_HD float sqrt_rn(uint64_t d2) {
    float f = (float)sqrt((double)d2);
    if (d2 < (1ull << 50)) return f;
    // f >= 2^25: f = F * 2^e with F in [2^23, 2^24), e >= 2; the midpoints (2F +- 1) * 2^(e-1) are integers
    uint32_t bits;
    memcpy(&bits, &f, 4);
    const int e = (int)(bits >> 23) - 127 - 23;
    const uint64_t F = (bits & 0x7fffffu) | 0x800000u;
    const uint64_t hi = sq_scaled(2 * F + 1, e - 1);
    const uint64_t lo = F == 0x800000u ? sq_scaled(4 * F - 1, e - 2) : sq_scaled(2 * F - 1, e - 1);
    if (d2 > hi || (d2 == hi && (F & 1))) bits += 1;
    else if (d2 < lo || (d2 == lo && (F & 1))) bits -= 1;
    memcpy(&f, &bits, 4);
    return f;
}

PQP_HD int32_t float_bits(float v) { int32_t b; memcpy(&b, &v, 4); return b; }

// ---- phase B ----------------------------------------------------------------------------------------------------------------------
// Stack entries of the envelope, one int32 each: site column in the low `site_bits` bits (site_bits = bits of cols - 1), g above.  Both
// always fit: rows * cols < 2^30 gives g < rows < 2^(31 - site_bits).
struct Site { int32_t c, g; };
PQP_HD int32_t pack(Site s, int site_bits) { return (s.g << site_bits) | s.c; }
PQP_HD Site unpack(int32_t v, int site_bits) { return Site{v & ((1 << site_bits) - 1), v >> site_bits}; }

// D: int32_t while every squared distance of the map fits ((rows - 1)^2 + (cols - 1)^2 < 2^31), int64_t otherwise
template <class D> PQP_HD D f_at(int32_t x, Site s) { const D dx = (D)x - s.c; return dx * dx + (D)s.g * s.g; }
// first column at which site b (right of a) is strictly nearer than a:  1 + floor((b^2 - a^2 + g_b^2 - g_a^2) / (2 (b - a)))
template <class D> PQP_HD D start_of(Site a, Site b) {
    const D num = (D)b.c * b.c - (D)a.c * a.c + (D)b.g * b.g - (D)a.g * a.g, den = 2 * ((D)b.c - a.c);
    return 1 + (num >= 0 ? num / den : -((-num + den - 1) / den));
}

// What phase B needs of a map's shape: stack packing, the value of a map without obstacle, and whether its squared distances need 64 bits
struct Shape { int site_bits; uint64_t empty_d2; bool wide; };
inline Shape shape_of(int rows, int cols) {
    return Shape{32 - __builtin_clz((unsigned)(cols - 1)), (uint64_t)rows * rows + (uint64_t)cols * cols,
                 (uint64_t)(rows - 1) * (rows - 1) + (uint64_t)(cols - 1) * (cols - 1) >= (1ull << 31)};
}

// One row r of one map: line[c * stride] holds g(r, c) on entry and dist(r, c) (float bits) on return.  empty_d2 = rows^2 + cols^2,
// what every cell of a map without obstacle gets.  Pass 1 builds the envelope with stack entry k stored at line[k * stride]: k <= c at
// column c, a column already read.  Pass 2 writes column c after reading the entries it needs, which lie at columns <= c (an entry's
// start column is at least its index).  Only the top entry and the one below it are kept in registers.
template <class D>
PQP_HD void envelope_line(int32_t* line, int64_t stride, int cols, int site_bits, uint64_t empty_d2, float res) {
    int q = -1;                    // index of the top entry
    Site top{0, 0}, below{0, 0};
    D top_start = 0;
    auto pop = [&]() {
        --q;
        top = below;
        if (q >= 1) { below = unpack(line[(int64_t)(q - 1) * stride], site_bits); top_start = start_of<D>(below, top); }
        else top_start = 0;
    };
    constexpr int kAhead = 8;      // loads of g issued together: columns beyond c are never written during this pass
    for (int c0 = 0; c0 < cols; c0 += kAhead) {
        int32_t gs[kAhead];
PQP_EDT_UNROLL
        for (int k = 0; k < kAhead; ++k) gs[k] = c0 + k < cols ? line[(int64_t)(c0 + k) * stride] : kNoObstacle;
PQP_EDT_UNROLL
        for (int k = 0; k < kAhead; ++k) {
            if (gs[k] < 0) continue;
            const Site u{c0 + k, gs[k]};
            while (q >= 0 && f_at<D>((int32_t)top_start, top) > f_at<D>((int32_t)top_start, u)) pop();
            if (q < 0) {
                q = 0; top = u; top_start = 0;
                line[0] = pack(u, site_bits);
            } else {
                const D w = start_of<D>(top, u);
                if (w < cols) {
                    ++q; below = top; top = u; top_start = w;
                    line[(int64_t)q * stride] = pack(u, site_bits);
                }
            }
        }
    }
    if (q < 0) {                   // no obstacle in the map
        const int32_t v = float_bits(sqrt_rn(empty_d2) * res);
        for (int c = 0; c < cols; ++c) line[(int64_t)c * stride] = v;
        return;
    }
    for (int c = cols - 1; c >= 0; --c) {
        line[(int64_t)c * stride] = float_bits(sqrt_rn((uint64_t)f_at<D>(c, top)) * res);
        if (c == top_start && q > 0) pop();
    }
}

}  // namespace edt
}  // namespace pqp
