// peer_major_ops.hpp — the per-element arithmetic of the per-peer send lists (wq_peers.hip): the
// clamped row bounds, the row that covers an element, the connected test and the sort key of an
// element, sentinel included. __host__ __device__, so tests/cpp/peer_major_host_shim.hip runs the
// same code on the CPU against worldql_server_amd/interest.py (peer_major_np).
//
// The expand is element-parallel: element j of [0, n_pairs) finds the row that covers it by a
// binary search over offsets[0 .. n_msgs], then checks the found row's clamped bounds. For ascending
// offsets that is exactly "the row m with offsets[m] <= j < offsets[m + 1]"; for any other offsets
// the search still ends on one row in [0, n_msgs], the check still decides from that row's two
// bounds alone, and an element no row covers gets the sentinel key. Every one of the n_pairs keys
// is written by exactly one lane, so nothing of an earlier call shows through and two calls give
// the same bytes.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace wq {

// Row m of a CSR as the part of [off[m], off[m + 1]) inside [0, cap): a <= b <= cap always; empty
// when off[m + 1] < off[m].
__host__ __device__ __forceinline__ void pm_row_bounds(const uint32_t* __restrict__ off, uint32_t m, uint32_t cap,
                                                       uint32_t& a, uint32_t& b) {
    const uint32_t o0 = off[m], o1 = off[m + 1];
    a = o0 < cap ? o0 : cap;
    b = o1 < cap ? o1 : cap;
    if (b < a) b = a;
}

// The row that covers element j (j < cap), or M when none does. Reads off[0 .. M] only. The search
// keeps off[lo] <= j: for ascending offsets it ends on the last such row, whose successor starts
// past j unless the row is M itself (j is behind the last row) — rows without elements are stepped
// over. Whatever the offsets hold, the result is in [0, M] and the bounds check has the last word.
__host__ __device__ __forceinline__ uint32_t pm_row_of(const uint32_t* __restrict__ off, uint32_t M, uint32_t cap,
                                                       uint32_t j) {
    if (M == 0 || off[0] > j) return M;
    uint32_t lo = 0, hi = M;
    while (hi > lo) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= j)
            lo = mid;
        else
            hi = mid - 1;
    }
    if (lo == M) return M;
    uint32_t a, b;
    pm_row_bounds(off, lo, cap, a, b);
    return (j >= a && j < b) ? lo : M;
}

// Is peer p one the transport sends to: below n_peers and its bit set (connected == nullptr: every
// peer is connected). The bitmap is read only for p < n_peers: words [0, ceil(n_peers / 32)).
__host__ __device__ __forceinline__ bool pm_connected(const uint32_t* __restrict__ connected, uint32_t n_peers,
                                                      uint32_t p) {
    return p < n_peers && (!connected || ((connected[p >> 5] >> (p & 31)) & 1u));
}

// Sort key and message of element j of [0, cap): the peer when a row covers j and the peer is
// connected, else the sentinel n_peers (sorted behind every peer). *msg is the covering row, 0 when
// there is none: always below max(M, 1). peers is read at j only, and only when a row covers it.
__host__ __device__ __forceinline__ uint32_t pm_key(const uint32_t* __restrict__ off,
                                                    const uint32_t* __restrict__ peers, uint32_t M, uint32_t cap,
                                                    const uint32_t* __restrict__ connected, uint32_t n_peers,
                                                    uint32_t j, uint32_t* msg) {
    const uint32_t m = pm_row_of(off, M, cap, j);
    if (m == M) {
        *msg = 0;
        return n_peers;
    }
    *msg = m;
    const uint32_t p = peers[j];
    return pm_connected(connected, n_peers, p) ? p : n_peers;
}

// Bits of the radix sort: enough for the keys 0 .. n_peers (the sentinel), at least one.
__host__ __device__ __forceinline__ int pm_key_bits(uint32_t n_peers) {
    int bits = 1;
    while (bits < 32 && (1ull << bits) <= n_peers) bits++;
    return bits;
}

// Lower bound of key p in the ascending skey[0, P): where peer p's messages start.
__host__ __device__ __forceinline__ uint32_t pm_lower_bound(const uint32_t* __restrict__ skey, uint32_t P,
                                                            uint32_t p) {
    uint32_t lo = 0, hi = P;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (skey[mid] < p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

}  // namespace wq
