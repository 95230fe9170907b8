// compact_ops.hpp — the arithmetic of the slab's compaction (wq_slab_compact.hip, wq_slab_compact_device):
// the term of an entry under the range rule, the scan's pair and operator, the all-or-nothing decision, the
// 16-byte chunk a quad lane writes and the tiles of the copy. __host__ __device__, so
// tests/cpp/slab_compact_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/records.py (slab_compact_np).
//
// An entry is four 16-byte chunks: 0 the uuid, 1 pos[0] and pos[1], 2 pos[2], world and bits, 3 off,
// data_len and flex_len. A quad of four lanes walks it, lane c with chunk c; lane 3 does the arithmetic with
// the bits lane 2 holds.
//
// Handle i has the term (live, size): size = data_len + flex_len of a live entry whose range stays inside
// the source arena, else 0. (K, E) is the exclusive scan of the terms over the handles: K[i] the rank of
// handle i among the live ones, E[i] the byte where its payload goes. The copy's elements are the live
// entries alone, the dense list dE[K[i]] = E[i], dS[K[i]] = the entry's source offset, dE[n_live] = the
// total; behind that it is pack_ops.hpp's copy from byte 0 of the destination arena.
#pragma once

#include "../../include/wq_router.h"
#include "pack_ops.hpp"

namespace wq {

constexpr uint32_t kCmpErrRange = 1u;  // error bit 0: a live entry whose range leaves the source arena
constexpr uint32_t kCmpOverArena = 1u, kCmpOverEntries = 2u;
constexpr uint64_t kCmpMaxEntries = 0xFFFFFFFFull;  // n_entries stays below it on both sides
constexpr uint64_t kCmpLive = 1ull << 63;           // a term's live flag; the size is the bits below it
constexpr uint32_t kCmpQuad = 4;                    // lanes, and chunks, of an entry

// Sixteen aligned bytes of an entry as four little-endian words.
struct alignas(16) CmpChunk {
    uint32_t x, y, z, w;
};

// What the control block carries between the passes.
struct CmpCtrl {
    uint64_t max_need;  // the highest live handle + 1 (atomic max of the size pass)
    uint64_t n_live;    // set by the decision: the elements of the copy
    uint32_t error;
    uint32_t overflow;  // set by the decision; the passes behind it do nothing when it is not 0
};

// The term of an entry with these fields in a source arena of n_src_bytes. The range check is in u64 and
// does not wrap: an `off` near 2^64 is past the arena.
__host__ __device__ __forceinline__ uint64_t cmp_term(uint32_t bits, uint64_t off, uint32_t data_len, uint32_t flex_len,
                                                      uint64_t n_src_bytes, uint32_t* err) {
    if (!(bits & WQ_SLAB_LIVE)) return 0ull;
    const uint64_t len = (uint64_t)data_len + (uint64_t)flex_len;
    if (off > n_src_bytes || len > n_src_bytes - off) {
        *err |= kCmpErrRange;
        return kCmpLive;
    }
    return kCmpLive | len;
}
__host__ __device__ __forceinline__ bool cmp_live(uint64_t term) { return (term & kCmpLive) != 0; }
__host__ __device__ __forceinline__ uint64_t cmp_size(uint64_t term) { return term & ~kCmpLive; }

// The scan's value: live entries and payload bytes before a handle. The byte sum saturates, so a total no
// arena holds is an overflow and never a small number.
struct CmpKE {
    uint64_t k, e;
};
struct CmpPlus {
    __host__ __device__ __forceinline__ CmpKE operator()(const CmpKE& a, const CmpKE& b) const {
        const uint64_t e = a.e + b.e;
        return CmpKE{a.k + b.k, e < a.e ? ~0ull : e};
    }
};
// The term of handle i in the scan: nothing behind the n handles.
__host__ __device__ __forceinline__ CmpKE cmp_ke(const uint64_t* __restrict__ term, uint64_t n, uint64_t i) {
    if (i >= n) return CmpKE{0ull, 0ull};
    const uint64_t t = term[i];
    return CmpKE{cmp_live(t) ? 1ull : 0ull, cmp_size(t)};
}

// The decision: the overflow bits of a result of `total` bytes whose highest live handle + 1 is max_need.
__host__ __device__ __forceinline__ uint32_t cmp_decide(uint64_t total, uint64_t max_need, const wq_slab_view& dst) {
    uint32_t over = 0;
    if (total > dst.n_payload_bytes) over |= kCmpOverArena;
    if (max_need > dst.n_entries) over |= kCmpOverEntries;
    return over;
}

// Chunk c of the destination entry of a handle: zeros for a handle that is not kept, else the source's
// chunk v, chunk 3 with `off` = e and, for an entry whose range left the arena (its size is not its
// lengths' sum), both lengths 0.
__host__ __device__ __forceinline__ CmpChunk cmp_entry_chunk(uint32_t c, CmpChunk v, bool kept, uint64_t term, uint64_t e) {
    if (!kept) return CmpChunk{0u, 0u, 0u, 0u};
    if (c != 3) return v;
    const bool whole = cmp_size(term) == (uint64_t)v.z + (uint64_t)v.w;
    return CmpChunk{(uint32_t)e, (uint32_t)(e >> 32), whole ? v.z : 0u, whole ? v.w : 0u};
}
// The source offset chunk 3 holds.
__host__ __device__ __forceinline__ uint64_t cmp_chunk_off(CmpChunk v) { return (uint64_t)v.x | (uint64_t)v.y << 32; }

// The destination's tiles: tile t covers the arena bytes [t kPackTile, + kPackTile) below the total.
__host__ __device__ __forceinline__ uint64_t cmp_tiles(uint64_t total) { return (total + kPackTile - 1) / kPackTile; }

}  // namespace wq
