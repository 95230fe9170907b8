// sends_ops.hpp — the per-element arithmetic of the tick sends (wq_sends.hip): the region that holds an
// element of the laid-out element space, the row that covers it (peer_major_ops.hpp on the region's own
// offsets), its frame, its drops and its composite sort key, and the per-peer lower bound in the sorted
// keys. __host__ __device__, so tests/cpp/tick_sends_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/interest.py (tick_sends_np).
//
// Element j of [0, n_elems) is owned by one lane: it finds its region by a search over the regions'
// element prefix, its row by pm_row_of on the region's offsets (no search for unit rows), then reads one
// src entry and one peer. No lane owns a row, a region or a peer, so one region of 16M elements and a
// million regions of one element are the same work per lane. Every key and value is written by exactly
// one lane: nothing of an earlier call shows through and two calls give the same bytes.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/wq_router.h"
#include "peer_major_ops.hpp"

namespace wq {

// What became of an element: the order of wq_tick_sends_counters' n_kept, n_drop_peer, n_drop_frame.
enum : int { kSndNone = 0, kSndKept = 1, kSndDropPeer = 2, kSndDropFrame = 3 };

// The arrays of a call as the passes take them. elem_pre[n_regions + 1]: the exclusive prefix of the
// regions' capacities; row_pre[n_regions + 1]: of their n_rows, unit-row regions counted as 0 (the rows
// whose offsets the row check reads).
struct SndView {
    const wq_send_region* reg;
    const uint32_t* elem_pre;
    const uint64_t* row_pre;
    const uint32_t* off;
    const uint32_t* peers;
    const uint32_t* src[2];
    const uint32_t* connected;
    uint32_t n_regions, n_peers, n_frames;
    int frame_bits;
};

// Bits of a frame index: the width of n_frames - 1 (0 for n_frames <= 1).
__host__ __device__ __forceinline__ int snd_frame_bits(uint32_t n_frames) {
    int bits = 0;
    while (bits < 32 && (1ull << bits) < n_frames) bits++;
    return bits;
}

// The region that holds element j (j < pre[n]): the last g with pre[g] <= j. Regions without elements
// share their successor's prefix and are stepped over.
template <typename T>
__host__ __device__ __forceinline__ uint32_t snd_region_of(const T* __restrict__ pre, uint32_t n, T j) {
    uint32_t lo = 0, hi = n;  // pre[lo] <= j < pre[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (pre[mid] <= j)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// The row that covers element e of region g (e < g.capacity), or g.n_rows when none does.
__host__ __device__ __forceinline__ uint32_t snd_row_of(const SndView& v, const wq_send_region& g, uint32_t e) {
    if (g.off_at == WQ_SEND_UNIT_ROWS) return e < g.n_rows ? e : g.n_rows;
    return pm_row_of(v.off + g.off_at, g.n_rows, g.capacity, e);
}

// Element j of the element space: what became of it, its frame (0 unless kept) and its sort key,
// (peer, or the sentinel n_peers unless kept) << frame_bits | frame.
template <typename K>
__host__ __device__ __forceinline__ int snd_elem(const SndView& v, uint32_t j, K* key, uint32_t* frame) {
    const uint32_t gi = snd_region_of<uint32_t>(v.elem_pre, v.n_regions, j);
    const wq_send_region g = v.reg[gi];
    const uint32_t e = j - v.elem_pre[gi];
    *key = (K)v.n_peers << v.frame_bits;
    *frame = 0;
    const uint32_t r = snd_row_of(v, g, e);
    if (r == g.n_rows) return kSndNone;
    const uint64_t f = (uint64_t)g.frame_base + (g.src_at == WQ_SEND_NO_SRC ? r : v.src[g.src_sel][(uint64_t)g.src_at + r]);
    if (f >= v.n_frames) return kSndDropFrame;
    const uint32_t p = v.peers[(uint64_t)g.peers_at + e];
    if (!pm_connected(v.connected, v.n_peers, p)) return kSndDropPeer;
    *key = ((K)p << v.frame_bits) | (K)f;
    *frame = (uint32_t)f;
    return kSndKept;
}

// Row i of the row space (i < row_pre[n_regions]): does its end lie before its start or past the
// region's capacity (error bit 0: a cut route call, or offsets that are no CSR's).
__host__ __device__ __forceinline__ bool snd_row_bad(const SndView& v, uint64_t i) {
    const uint32_t gi = snd_region_of<uint64_t>(v.row_pre, v.n_regions, i);
    const wq_send_region g = v.reg[gi];
    const uint32_t* off = v.off + g.off_at;
    const uint64_t r = i - v.row_pre[gi];
    return off[r + 1] < off[r] || off[r + 1] > g.capacity;
}

// The host's check of a call's sizes and regions (64-bit sums): nullptr, or why the call is invalid.
inline const char* snd_check(const wq_tick_sends_in* in, size_t n_elems) {
    if ((in->n_regions && !in->regions) || (in->n_offsets && !in->d_offsets) || (in->n_pairs && !in->d_peers) ||
        (in->n_src[0] && !in->d_src[0]) || (in->n_src[1] && !in->d_src[1]))
        return "tick_sends: a null array with a non-zero size";
    if (in->n_peers == 0xFFFFFFFFu) return "tick_sends: n_peers must be < 2^32 - 1";
    uint64_t total = 0;
    for (uint32_t k = 0; k < in->n_regions; ++k) {
        const wq_send_region& g = in->regions[k];
        if (g.pad_ || g.src_sel > 1) return "tick_sends: a region with pad_ != 0 or src_sel > 1";
        if (g.n_rows && g.off_at != WQ_SEND_UNIT_ROWS && (uint64_t)g.off_at + g.n_rows + 1 > in->n_offsets)
            return "tick_sends: a region reaches outside d_offsets";
        if ((uint64_t)g.peers_at + g.capacity > in->n_pairs) return "tick_sends: a region reaches outside d_peers";
        if (g.n_rows && g.src_at != WQ_SEND_NO_SRC && (uint64_t)g.src_at + g.n_rows > in->n_src[g.src_sel])
            return "tick_sends: a region reaches outside its src array";
        total += g.capacity;
        if (total > 0xFFFFFFFFull) return "tick_sends: the capacities sum to more than 2^32 - 1";
    }
    if (total != n_elems) return "tick_sends: n_elems is not the sum of the regions' capacities";
    return nullptr;
}

// The prefixes of SndView over checked regions: elem_pre and row_pre, n_regions + 1 entries each.
inline void snd_prefixes(const wq_send_region* reg, uint32_t n, uint32_t* elem_pre, uint64_t* row_pre) {
    uint32_t e = 0;
    uint64_t r = 0;
    for (uint32_t k = 0; k < n; ++k) {
        elem_pre[k] = e;
        row_pre[k] = r;
        e += reg[k].capacity;
        if (reg[k].off_at != WQ_SEND_UNIT_ROWS) r += reg[k].n_rows;
    }
    elem_pre[n] = e;
    row_pre[n] = r;
}

// Lower bound of peer p's first key, p << frame_bits, in the ascending skey[0, P): where its frames start.
template <typename K>
__host__ __device__ __forceinline__ uint32_t snd_lower_bound(const K* __restrict__ skey, uint32_t P, uint32_t p,
                                                             int frame_bits) {
    const K want = (K)p << frame_bits;
    uint32_t lo = 0, hi = P;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (skey[mid] < want)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

}  // namespace wq
