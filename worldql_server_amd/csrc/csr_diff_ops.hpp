// csr_diff_ops.hpp — the per-row and per-element arithmetic of the interest diff (wq_csr_diff.hip):
// clamped row bounds, the ordinal space of a side and its limit, the row of an ordinal, the
// membership search and the output offset of a row. __host__ __device__, so
// tests/cpp/csr_diff_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/interest.py.
//
// A side (the new tick for "entered", the old one for "left") is walked in its ordinal space: the
// elements of its clamped rows laid end to end, pre[m] = elements of the rows before m (an exclusive
// prefix of the clamped lengths, monotone whatever the offsets hold). For a valid CSR the ordinal of
// an element is its index. 64 consecutive ordinals are one granule (one wave step): a granule's
// flag word marks the elements that are not in the other side's row, its count is the word's
// popcount, and the exclusive prefix of the counts places every kept element — the output is the
// compaction of the flagged elements in ordinal order, which is row order.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace wq {

constexpr uint32_t kDiffGranule = 64;  // ordinals per granule (one wave step)
constexpr uint32_t kDiffErrRows = 1u;  // wq_diff_counters.error bit 0

// Two u32 side by side, the new side first: clamped row lengths and their prefix (per row), granule
// counts and their prefix (per granule). Arrays of it are indexed as words: [2 * i + side].
struct alignas(8) DiffPair {
    uint32_t n, o;
};

__host__ __device__ __forceinline__ uint32_t diff_sat_add(uint32_t a, uint32_t b) {
    const uint64_t s = (uint64_t)a + b;
    return s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
}

// Prefix sums saturate: offsets that are not monotone can make the clamped rows overlap and their
// lengths sum past 2^32. A saturated prefix is above every ordinal (diff_limit).
struct DiffSatAdd {
    __host__ __device__ __forceinline__ DiffPair operator()(const DiffPair& a, const DiffPair& b) const {
        return DiffPair{diff_sat_add(a.n, b.n), diff_sat_add(a.o, b.o)};
    }
};

// Ordinals of a side are below this: twice its capacity, a multiple of the granule, below 2^32 - 63.
// The rows of a valid CSR hold at most `capacity` elements together, and so do the clamped rows
// around one descending pair of offsets twice that; rows that start past the limit are taken as
// empty (only with several descending pairs, error bit 0 is set then).
__host__ __device__ __forceinline__ uint32_t diff_limit(uint64_t capacity) {
    const uint64_t two = (2 * capacity + (kDiffGranule - 1)) & ~(uint64_t)(kDiffGranule - 1);
    return two > 0xFFFFFFC0ull ? 0xFFFFFFC0u : (uint32_t)two;
}

// Row m of a CSR as the part of [off[m], off[m + 1]) inside [0, cap): a <= b <= cap always. Returns
// false when the row had to be cut (off[m + 1] < off[m] or a bound past cap).
__host__ __device__ __forceinline__ bool diff_row_bounds(const uint32_t* __restrict__ off, uint32_t m, uint32_t cap,
                                                          uint32_t& a, uint32_t& b) {
    const uint32_t o0 = off[m], o1 = off[m + 1];
    a = o0 < cap ? o0 : cap;
    b = o1 < cap ? o1 : cap;
    if (b < a) b = a;
    return o1 >= o0 && o1 <= cap;
}

// The row of ordinal q: the last m in [lo, hi] with pre[2 * m + side] <= q (rows without elements
// share a prefix value with the next row that has some). Needs pre[2 * lo + side] <= q.
__host__ __device__ __forceinline__ uint32_t diff_row_of(const uint32_t* __restrict__ pre, int side, uint32_t lo,
                                                          uint32_t hi, uint32_t q) {
    while (hi > lo) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (pre[2ull * mid + side] <= q)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// Lower bound of v in the ascending peers[a, b).
__host__ __device__ __forceinline__ uint32_t diff_lower_bound(const uint32_t* __restrict__ peers, uint32_t a,
                                                               uint32_t b, uint32_t v) {
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (peers[mid] < v)
            a = mid + 1;
        else
            b = mid;
    }
    return a;
}

// One side of the diff: a CSR and the element count of its peers array.
struct DiffSide {
    const uint32_t* off;
    const uint32_t* peers;
    uint32_t cap;
};

// The source element of ordinal q (its row is in [rlo, rhi]): row in *m, index into src.peers
// returned; *ok is false for an ordinal whose row was cut short of it (never for q below the side's
// total, kept as a bound on the read).
__host__ __device__ __forceinline__ uint32_t diff_source(const DiffSide& src, const uint32_t* __restrict__ pre,
                                                          int side, uint32_t rlo, uint32_t rhi, uint32_t q,
                                                          uint32_t* m, bool* ok) {
    const uint32_t r = diff_row_of(pre, side, rlo, rhi, q);
    uint32_t a, b;
    (void)diff_row_bounds(src.off, r, src.cap, a, b);
    const uint32_t j = a + (q - pre[2ull * r + side]);
    *m = r;
    *ok = j >= a && j < b;
    return j;
}

// Is the element of ordinal q of `src` missing from the same row of `oth`?
__host__ __device__ __forceinline__ bool diff_keeps(const DiffSide& src, const DiffSide& oth,
                                                     const uint32_t* __restrict__ pre, int side, uint32_t rlo,
                                                     uint32_t rhi, uint32_t q) {
    uint32_t m;
    bool ok;
    const uint32_t j = diff_source(src, pre, side, rlo, rhi, q, &m, &ok);
    if (!ok) return false;
    const uint32_t v = src.peers[j];
    uint32_t c, d;
    (void)diff_row_bounds(oth.off, m, oth.cap, c, d);
    const uint32_t k = diff_lower_bound(oth.peers, c, d, v);
    return !(k < d && oth.peers[k] == v);
}

// Kept elements before ordinal q (q <= the side's total): the output offset of the row that starts
// there. base: exclusive prefix of the granule counts, flags: the granules' words.
__host__ __device__ __forceinline__ uint32_t diff_kept_before(const uint32_t* __restrict__ base,
                                                               const uint64_t* __restrict__ flags, int side,
                                                               uint32_t q) {
    const uint32_t g = q / kDiffGranule, r = q % kDiffGranule;
    uint32_t n = base[2ull * g + side];
    if (r) n += (uint32_t)__builtin_popcountll(flags[g] & ((1ull << r) - 1ull));
    return n;
}

}  // namespace wq
