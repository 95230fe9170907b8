// rotate_ops.hpp — the arithmetic of the fair share (wq_rotate.hip, wq_peer_rotate_device): which
// elements of a peer's full send list a budget cut, their cyclic order behind the peer's cursor, the
// running bytes in that order and the predicate that chooses the rotating share. __host__ __device__,
// so tests/cpp/peer_rotate_host_shim.hip runs the same text on the CPU against
// worldql_server_amd/interest.py (peer_rotate_np).
//
// Both CSRs, the full one and the kept one, use the budgets' rows (budget_ops.hpp): clamped to their
// array, walked up to the array's element count in total. The full CSR's walk is the ordinal space of
// every per-element array here; x below is an ordinal, s and e its row's first and end ordinal.
//
// Cut. For ascending rows the element at index i of full row p, with value m, is the occ-th m of its
// row (occ = i - lower bound of m); the kept row holds ck = upper bound - lower bound elements m. The
// first min(cf, ck) occurrences are kept, so the element is cut iff occ >= ck.
//
// Order. P = s + (upper bound of cursor[p] in the full row). C is the exclusive prefix of the cut
// flags over the ordinals, B the exclusive u64 prefix of cut flag * size. The cyclic rank of a cut
// element is C[x] - C[P] from P on, and C[x] - C[s] + (C[e] - C[P]) before P; its running bytes are
// the same expression in B, plus its own size. Per row the terms that do not depend on x are folded
// into RotRow, so an element needs its own C and B only.
#pragma once

#include "budget_ops.hpp"

namespace wq {

// The cut and keep flags are kept as one u64 word per granule of kRotGranule ordinals (a wave's
// ballot); a block of kRotTile ordinals sums its chosen bytes before it adds them to the call's total.
constexpr uint32_t kRotGranule = 64;
constexpr uint32_t kRotTile = 256;
// The per-block and per-wave counter adds are spread over kRotParts slots (a power of two).
constexpr uint32_t kRotParts = 256;
struct RotPart {
    unsigned long long bytes_chosen;
    uint32_t rows_rotated, rows_behind;
};
constexpr uint32_t kRotErrRows = 1u, kRotErrMsg = 2u, kRotErrKept = 4u;

// The first index of a[0 .. n) whose value is >= v (lower) or > v (upper); n when there is none.
// On an array that does not ascend the result is some index in [0, n], the same every time.
__host__ __device__ __forceinline__ uint32_t rot_lower(const uint32_t* __restrict__ a, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
__host__ __device__ __forceinline__ uint32_t rot_upper(const uint32_t* __restrict__ a, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// The occurrence index of element i of a row: how many elements equal to it stand before it. An
// element that differs from its left neighbour is the first of its value (rows ascend); otherwise
// the lower bound of the value among the elements before it. Never above i.
__host__ __device__ __forceinline__ uint32_t rot_occurrence(const uint32_t* __restrict__ row, uint32_t i) {
    const uint32_t m = row[i];
    if (i == 0 || row[i - 1] != m) return 0;
    return i - rot_lower(row, i, m);
}

// Is the occ-th element of value m of the full row cut, given the kept row krow[0 .. klen)? The upper
// bound is searched behind the lower one, so the count is never negative.
__host__ __device__ __forceinline__ bool rot_is_cut(const uint32_t* __restrict__ krow, uint32_t klen, uint32_t m,
                                                    uint32_t occ) {
    const uint32_t lb = rot_lower(krow, klen, m);
    if (lb == klen || krow[lb] != m) return true;
    const uint32_t ck = rot_upper(krow + lb, klen - lb, m);
    return occ >= ck;
}

__host__ __device__ __forceinline__ uint32_t rot_share(const uint32_t* __restrict__ extra, uint32_t r, uint32_t p) {
    return extra ? extra[p] : r;
}
__host__ __device__ __forceinline__ uint64_t rot_share_bytes(const uint64_t* __restrict__ extra_bytes, uint64_t v,
                                                             uint32_t p) {
    return extra_bytes ? extra_bytes[p] : v;
}

// What an element needs of its row: P, and the x-independent terms of the rank and the running bytes
// on either side of P (mod 2^32 and 2^64; the results are exact, see rot_rank).
struct RotRow {
    uint32_t P;       // s + upper bound of the cursor
    uint32_t CP;      // C[P]
    uint32_t wrap;    // C[e] - C[P] - C[s]
    uint32_t n_cut;   // C[e] - C[s]
    uint64_t BP;      // B[P]
    uint64_t Bwrap;   // B[e] - B[P] - B[s]
};

__host__ __device__ __forceinline__ RotRow rot_row(uint32_t P, uint32_t Cs, uint32_t CP, uint32_t Ce, uint64_t Bs,
                                                   uint64_t BP, uint64_t Be) {
    return RotRow{P, CP, Ce - CP - Cs, Ce - Cs, BP, Be - BP - Bs};
}

// Cyclic rank of the cut element at ordinal x, Cx = C[x]: the cut elements in [P, x) from P on, else
// those in [P, e) and [s, x).
__host__ __device__ __forceinline__ uint32_t rot_rank(const RotRow& r, uint32_t x, uint32_t Cx) {
    return x >= r.P ? Cx - r.CP : Cx + r.wrap;
}

// Running bytes of the cut element at ordinal x in the cyclic order, its own size included.
__host__ __device__ __forceinline__ uint64_t rot_bytes(const RotRow& r, uint32_t x, uint64_t Bx, uint32_t size) {
    return (x >= r.P ? Bx - r.BP : Bx + r.Bwrap) + size;
}

// The chosen elements are the longest prefix of the cyclic order with rank < R and, with sizes,
// running bytes <= V; rank 0 is chosen whenever R >= 1. Rank and running bytes both grow along the
// order, so the prefix is the set of elements that meet the test on their own: once the bytes pass
// V they stay above it, the first element's overshoot included.
__host__ __device__ __forceinline__ bool rot_chosen(uint32_t rank, uint64_t bytes, uint32_t R, bool with_sizes,
                                                    uint64_t V) {
    if (R == 0) return false;
    if (rank == 0) return true;
    return rank < R && (!with_sizes || bytes <= V);
}

// Elements chosen in a row from its lengths: the output row holds the kept (len - n_cut) and the chosen.
__host__ __device__ __forceinline__ uint32_t rot_n_chosen(uint32_t out_len, uint32_t len, uint32_t n_cut) {
    return out_len - (len - n_cut);
}

// `error` bit 2: some kept element had no partner in its full row. Every full element that is not cut
// is matched to one kept element, so the bit is "matched != kept elements walked".
__host__ __device__ __forceinline__ uint32_t rot_kept_error(uint64_t n_matched, uint64_t n_kept_walked) {
    return n_matched != n_kept_walked ? kRotErrKept : 0u;
}

}  // namespace wq
