// slab_ops.hpp — the arithmetic of the record payload slab (wq_slab.hip, wq_slab_store_device): the two
// payload parts of an op under the validity rules, the all-or-nothing decision, the entry of a create
// and the bytes of one 16-byte chunk of the arena. __host__ __device__, so
// tests/cpp/slab_store_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/records.py (slab_store_np).
//
// Op q has two elements, 2q (its data) and 2q + 1 (its flex); an op that is no create, an absent payload
// and a hostile reference are elements of size 0. E is the exclusive u64 prefix sum of the element sizes
// over the T = 2 n_ops elements, so element k lies at arena bytes [base + E[k], base + E[k + 1]) with
// base the cursor before the call, and S[k] says where its bytes start in the frame bytes.
//
// The copy runs over the arena's bytes [base, base + E[T]) in the send buffers' shape (pack_ops.hpp, whose
// element search, window, composer and stores it shares): tiles are kPackTile bytes at kPackTile-aligned
// arena addresses, so every whole chunk is one aligned 16-byte store whatever the cursor was. Only the
// range's first chunk can start inside a chunk; it is stored byte by byte, the last one by pack_store.
#pragma once

#include "../../include/wq_router.h"
#include "pack_ops.hpp"

namespace wq {

constexpr uint32_t kSlabErrFrame = 1u;  // error bit 0: a frame index >= n_frames or a frame whose offsets are refused
constexpr uint32_t kSlabErrData = 2u;   // bit 1: the data range leaves its frame
constexpr uint32_t kSlabErrFlex = 4u;   // bit 2: the same for flex
constexpr uint32_t kSlabOverArena = 1u, kSlabOverEntries = 2u;
constexpr uint64_t kSlabMaxOps = 1ull << 31;  // T = 2 n_ops stays a u32

struct SlabIn {
    const wq_rec_op* ops;
    const wq_rec_op_ref* refs;
    const uint8_t* frames;
    const uint64_t* fo;  // [n_frames + 1]
    uint64_t n_ops, n_frames;
};

// What the scratch's control block carries from the decision to the passes behind it.
struct SlabCtrl {
    uint64_t base;          // the cursor before the call
    uint64_t max_need;      // the largest create handle + 1 (atomic max of the size pass)
    uint64_t n_creates;
    uint32_t error;
    uint32_t overflow;      // set by the decision; the passes behind it do nothing when it is not 0
};

// The size of d_frames as the call takes it: 0 without frames.
__host__ __device__ __forceinline__ uint64_t slab_frame_bytes(const SlabIn& in) {
    return in.n_frames ? in.fo[in.n_frames] : 0ull;
}

// One payload range [off, off + len) of a frame of flen bytes: false when it leaves the frame.
__host__ __device__ __forceinline__ bool slab_range_ok(uint32_t off, uint32_t len, uint64_t flen) {
    return (uint64_t)off + (uint64_t)len <= flen;
}

// The two parts of op q: their lengths and where they start in the frame bytes (0 when empty).
struct SlabParts {
    uint64_t src[2];
    uint32_t len[2];
    uint32_t err;
    bool create;
};

__host__ __device__ __forceinline__ SlabParts slab_parts(const SlabIn& in, uint64_t q) {
    SlabParts p;
    p.src[0] = p.src[1] = 0;
    p.len[0] = p.len[1] = 0;
    p.err = 0;
    p.create = in.ops[q].kind == WQ_RECORD_CREATE;
    if (!p.create) return p;
    const wq_rec_op_ref r = in.refs[q];
    const uint32_t want[2] = {(r.bits & 1u) ? r.data_len : 0u, (r.bits & 2u) ? r.flex_len : 0u};
    const uint32_t off[2] = {r.data_off, r.flex_off};
    if (!want[0] && !want[1]) return p;  // nothing to copy: the frame is not looked at
    const uint64_t total = slab_frame_bytes(in);
    uint64_t a = 0, b = 0;
    bool frame_ok = r.frame < in.n_frames;
    if (frame_ok) {
        a = in.fo[r.frame], b = in.fo[(uint64_t)r.frame + 1];
        frame_ok = a <= b && b <= total;
    }
    if (!frame_ok) {
        p.err |= kSlabErrFrame;
        return p;
    }
    for (uint32_t k = 0; k < 2; ++k) {
        if (!want[k]) continue;
        if (!slab_range_ok(off[k], want[k], b - a)) {
            p.err |= k ? kSlabErrFlex : kSlabErrData;
            continue;
        }
        p.src[k] = a + off[k];
        p.len[k] = want[k];
    }
    return p;
}

// The term of element k in the scan of the sizes: 0 behind the T elements.
__host__ __device__ __forceinline__ uint64_t slab_term(const uint32_t* __restrict__ size, uint64_t T, uint64_t k) {
    return k < T ? (uint64_t)size[k] : 0ull;
}

// The decision: the overflow bits of a call that starts at `base`, stores `total` bytes and whose largest
// create handle + 1 is max_need.
__host__ __device__ __forceinline__ uint32_t slab_decide(uint64_t base, uint64_t total, uint64_t max_need,
                                                         const wq_slab_view& v) {
    uint32_t over = 0;
    if (base > v.n_payload_bytes || total > v.n_payload_bytes - base) over |= kSlabOverArena;
    if (max_need > v.n_entries) over |= kSlabOverEntries;
    return over;
}

__host__ __device__ __forceinline__ void slab_be64(uint8_t* out, uint64_t v) {
    for (uint32_t i = 0; i < 8; ++i) out[i] = (uint8_t)(v >> (8 * (7 - i)));
}

// The entry of create op q whose data starts at arena byte `off`.
__host__ __device__ __forceinline__ wq_slab_entry slab_entry(const SlabIn& in, uint64_t q, uint64_t off,
                                                             uint32_t data_len, uint32_t flex_len) {
    const wq_rec_op& op = in.ops[q];
    wq_slab_entry e;
    slab_be64(e.uuid, op.uuid_hi);
    slab_be64(e.uuid + 8, op.uuid_lo);
    e.pos[0] = op.pos[0], e.pos[1] = op.pos[1], e.pos[2] = op.pos[2];
    e.world = op.world;
    e.bits = (in.refs[q].bits & (WQ_SLAB_DATA | WQ_SLAB_FLEX)) | WQ_SLAB_POSITION | WQ_SLAB_LIVE;
    e.off = off;
    e.data_len = data_len;
    e.flex_len = flex_len;
    return e;
}

// The arena's tiles: tile t of the call covers [slab_tile0(base) + t kPackTile, + kPackTile).
__host__ __device__ __forceinline__ uint64_t slab_tile0(uint64_t base) { return base & ~(uint64_t)(kPackTile - 1); }
__host__ __device__ __forceinline__ uint64_t slab_tiles(uint64_t base, uint64_t total) {
    return total ? (base + total - slab_tile0(base) + kPackTile - 1) / kPackTile : 0ull;
}
__host__ __device__ __forceinline__ uint64_t slab_tiles_per_block(uint64_t tiles, uint64_t blocks) {
    return (tiles + blocks - 1) / blocks;
}

// Blocks of the copy for an arena of n_payload_bytes > 0: the call's range can be any part of it and may
// start inside a tile.
__host__ __device__ __forceinline__ uint64_t slab_blocks(uint64_t n_payload_bytes) {
    return pack_blocks(n_payload_bytes + kPackTile);
}

// Stores the bytes [lo, hi) of the chunk v that starts at arena byte d0 (d0 a multiple of 16, d0 <= lo <
// hi <= d0 + 16, the arena 16-byte aligned): pack_store's aligned stores when the range starts with the
// chunk, single bytes for the call's first chunk when the cursor stood inside it.
__host__ __device__ __forceinline__ void slab_store(uint8_t* __restrict__ out, uint64_t d0, uint64_t lo, uint64_t hi,
                                                    PackChunk v) {
    if (lo == d0) {
        pack_store(out, d0, (uint32_t)(hi - d0), v);
        return;
    }
    for (uint64_t c = lo; c < hi; ++c) {
        const uint32_t i = (uint32_t)(c - d0);
        out[c] = (uint8_t)(i < 8 ? v.lo >> (8 * i) : v.hi >> (8 * (i - 8)));
    }
}

}  // namespace wq
