// pack_ops.hpp — the arithmetic of the send buffers (wq_pack.hip, wq_peer_pack_device): the frame of
// a message with its validity rules, the size of a record, the element that covers an output byte,
// the search in a tile's window of record starts and the composer of one 16-byte destination chunk.
// __host__ __device__, so tests/cpp/peer_pack_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/interest.py (peer_pack_np).
//
// Rows and ordinals are the budgets' (budget_ops.hpp: bud_len, the saturating prefix, bud_row_of,
// bud_row_start). Ordinal q has a record of rec_q bytes, an optional 4-byte little-endian size
// followed by the frame; E is the exclusive u64 prefix sum of the record sizes over the T walked
// ordinals, with E[T] the size of the whole result. Record q is out[E[q] .. E[q + 1]).
//
// The copy runs over the output bytes. A tile is kPackTile bytes, a chunk kPackChunk; the elements
// that cover a tile are consecutive ordinals from the one that covers its first byte, and they are
// taken kPackWindow at a time: W[i] = E[min(wb + i, T)] for i in [0, kPackWindow] and S[i] the
// source offset of element wb + i. The window covers the output bytes [W[0], W[kPackWindow]).
#pragma once

#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "budget_ops.hpp"

namespace wq {

constexpr uint32_t kPackChunk = 16;                       // bytes one lane stores
constexpr uint32_t kPackLanes = 64;                       // lanes of a tile: one wave
constexpr uint32_t kPackTile = kPackChunk * kPackLanes;   // 1 KiB of output
constexpr uint32_t kPackWindow = 64;                      // elements of one window
constexpr uint64_t kPackMaxBlocks = 8192;                 // one-wave blocks of the copy: 32 per CU on 256 CUs
constexpr uint64_t kPackRun = 4;                          // consecutive tiles a block takes at least
constexpr uint32_t kPackPrefix = 4;                       // bytes of the length prefix
constexpr uint32_t kPackFlagPrefix = 1u;                  // WQ_PACK_LEN_PREFIX
constexpr uint32_t kPackErrFrame = 4u;                    // error bit 2; bits 0 and 1: kBudErrRows, kBudErrMsg

// Sixteen bytes of output in little-endian order: byte i of the chunk is byte i of lo, or i - 8 of hi.
struct PackChunk {
    uint64_t lo, hi;
};

// The frame of message m: its size, and in *src where it starts in the frame bytes. Empty, with
// *err |= kBudErrMsg and fo not read, when the message does not exist; empty with kPackErrFrame when
// its offsets descend, reach past n_frame_bytes or span 2^32 bytes or more.
__host__ __device__ __forceinline__ uint32_t pack_frame(const uint64_t* __restrict__ fo, uint64_t n_msgs,
                                                        uint64_t n_frame_bytes, uint32_t m, uint64_t* src,
                                                        uint32_t* err) {
    *src = 0;
    if (m >= n_msgs) {
        *err |= kBudErrMsg;
        return 0u;
    }
    const uint64_t a = fo[m], b = fo[m + 1];
    if (a > b || b > n_frame_bytes || b - a >= (1ull << 32)) {
        *err |= kPackErrFrame;
        return 0u;
    }
    *src = a;
    return (uint32_t)(b - a);
}

__host__ __device__ __forceinline__ uint32_t pack_prefix_bytes(uint32_t flags) {
    return (flags & kPackFlagPrefix) ? kPackPrefix : 0u;
}

// The term of ordinal q in the scan of record sizes: 0 behind the T ordinals.
__host__ __device__ __forceinline__ uint64_t pack_rec_term(const uint32_t* __restrict__ size, uint32_t T, uint32_t pre,
                                                           uint64_t q) {
    return q < T ? (uint64_t)size[q] + pre : 0ull;
}

// The last q in [0, T] with E[q] <= c (E ascends from 0). For c < E[T] it is the element that covers
// byte c: E[q] <= c < E[q + 1], empty records before it stepped over. For c = capacity it is the
// number of records that lie wholly below the capacity.
__host__ __device__ __forceinline__ uint32_t pack_elem_of(const uint64_t* __restrict__ E, uint32_t T, uint64_t c) {
    uint32_t lo = 0, hi = T;
    while (hi > lo) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (E[mid] <= c)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The same element for c < E[T], searched forwards from a hint with E[hint] <= c: steps of 4, 16,
// 64 ... elements until one starts past c, then a bisection between the last two. A block walks
// consecutive tiles, so the element that covers a tile's first byte is at or a few elements past the
// one that covered the last byte of the tile before: two or three reads where the search over all
// of E takes log2(T).
__host__ __device__ __forceinline__ uint32_t pack_elem_from(const uint64_t* __restrict__ E, uint32_t T, uint32_t hint,
                                                            uint64_t c) {
    uint32_t lo = hint, hi, step = 4;
    for (;;) {
        hi = T - lo > step ? lo + step : T;
        if (E[hi] > c) break;  // E[T] > c ends it
        lo = hi;
        if (step < (1u << 28)) step <<= 2;
    }
    hi -= 1;
    while (hi > lo) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (E[mid] <= c)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// Blocks of the copy for a capacity > 0: a block per kPackRun tiles of the capacity, at most
// kPackMaxBlocks.
__host__ __device__ __forceinline__ uint64_t pack_blocks(uint64_t capacity) {
    const uint64_t tiles = (capacity - 1) / kPackTile + 1;
    const uint64_t blocks = (tiles + kPackRun - 1) / kPackRun;
    return blocks < kPackMaxBlocks ? blocks : kPackMaxBlocks;
}

// Tiles per block when `blocks` blocks share the tiles below `written` in consecutive runs.
__host__ __device__ __forceinline__ uint64_t pack_tiles_per_block(uint64_t written, uint64_t blocks) {
    const uint64_t tiles = (written + kPackTile - 1) / kPackTile;
    return (tiles + blocks - 1) / blocks;
}

// Entry i of the window that starts at element wb.
__host__ __device__ __forceinline__ uint64_t pack_win_entry(const uint64_t* __restrict__ E, uint32_t T, uint64_t wb,
                                                            uint32_t i) {
    const uint64_t q = wb + i;
    return E[q < T ? q : T];
}

// Does the payload of the element with record [r0, r1) hold the whole tile [c0, c1)?
__host__ __device__ __forceinline__ bool pack_tile_inside(uint64_t r0, uint64_t r1, uint32_t pre, uint64_t c0,
                                                          uint64_t c1) {
    return c1 - c0 == kPackTile && r0 + pre <= c0 && r1 >= c1;
}

// The last k in [0, kPackWindow) with W[k] <= c, given W[0] <= c.
__host__ __device__ __forceinline__ uint32_t pack_win_find(const uint64_t* W, uint64_t c) {
    uint32_t k = 0;
#pragma unroll
    for (uint32_t step = kPackWindow / 2; step; step >>= 1)
        if (W[k + step] <= c) k += step;
    return k;
}

// The low n bytes set, n in [0, 16].
__host__ __device__ __forceinline__ PackChunk pack_ones(uint32_t n) {
    PackChunk m;
    m.lo = n >= 8 ? ~0ull : (1ull << (8 * n)) - 1ull;
    m.hi = n <= 8 ? 0ull : n >= 16 ? ~0ull : (1ull << (8 * (n - 8))) - 1ull;
    return m;
}

// ORs the bytes [a, b) of v into *out (a < b <= 16).
__host__ __device__ __forceinline__ void pack_merge(PackChunk* out, PackChunk v, uint32_t a, uint32_t b) {
    const PackChunk hi = pack_ones(b), lo = pack_ones(a);
    out->lo |= v.lo & hi.lo & ~lo.lo;
    out->hi |= v.hi & hi.hi & ~lo.hi;
}

// Sixteen bytes from any address.
__host__ __device__ __forceinline__ PackChunk pack_load16(const uint8_t* p) {
    PackChunk v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// The chunk whose byte s + i is byte i of the little-endian u32 v, s in [-3, 15]; bytes that fall
// outside the chunk are dropped.
__host__ __device__ __forceinline__ PackChunk pack_place_u32(uint32_t v, int32_t s) {
    PackChunk c{0ull, 0ull};
    if (s < 0) {
        c.lo = (uint64_t)v >> (8 * (uint32_t)(-s));
    } else if (s < 8) {
        c.lo = (uint64_t)v << (8 * (uint32_t)s);
        c.hi = s > 4 ? (uint64_t)v >> (8 * (uint32_t)(8 - s)) : 0ull;
    } else {
        c.hi = (uint64_t)v << (8 * (uint32_t)(s - 8));
    }
    return c;
}

// The composer: ORs into *out the bytes [lo_c, hi_c) of the chunk [d0, d0 + 16) from the window's
// elements. Needs W[0] <= lo_c < hi_c <= min(d0 + 16, W[kPackWindow]) and d0 <= lo_c, so every byte
// of the range has its element inside the window. A prefix is placed from the record's size, a
// payload part comes from one 16-byte load laid over the chunk when those 16 source bytes all lie
// in [0, n_frame_bytes) (bytes outside the part are masked off), else byte by byte. Nothing outside
// [0, n_frame_bytes) of `frames` is read.
__host__ __device__ __forceinline__ void pack_compose(const uint64_t* W, const uint64_t* S,
                                                      const uint8_t* __restrict__ frames, uint64_t n_frame_bytes,
                                                      uint32_t pre, uint64_t d0, uint64_t lo_c, uint64_t hi_c,
                                                      PackChunk* out) {
    uint32_t k = pack_win_find(W, lo_c);
    uint64_t c = lo_c;
    while (c < hi_c) {
        while (W[k + 1] <= c) ++k;  // empty records; W[kPackWindow] >= hi_c > c ends it
        const uint64_t r0 = W[k], r1 = W[k + 1];
        const uint64_t e = r1 < hi_c ? r1 : hi_c;
        if (pre && c < r0 + pre) {
            const uint64_t pe = e < r0 + pre ? e : r0 + pre;
            const uint32_t size = (uint32_t)(r1 - r0 - pre);
            pack_merge(out, pack_place_u32(size, (int32_t)(int64_t)(r0 - d0)), (uint32_t)(c - d0), (uint32_t)(pe - d0));
            c = pe;
        }
        if (c < e) {
            const uint32_t a = (uint32_t)(c - d0), b = (uint32_t)(e - d0);
            const uint64_t t = S[k] + d0, u = r0 + pre;  // chunk byte i is frames[t - u + i]
            if (t >= u && t - u + kPackChunk <= n_frame_bytes) {
                pack_merge(out, pack_load16(frames + (t - u)), a, b);
            } else {
                for (uint32_t i = a; i < b; ++i) {
                    const uint64_t byte = frames[S[k] + (d0 + i - u)];
                    if (i < 8)
                        out->lo |= byte << (8 * i);
                    else
                        out->hi |= byte << (8 * (i - 8));
                }
            }
            c = e;
        }
    }
}

// Stores the first n bytes of v at out + d0 (d0 a multiple of 16, out 16-byte aligned): one 16-byte
// store for a whole chunk, else 8, 4, 2 and 1 bytes, each naturally aligned. Nothing behind d0 + n.
__host__ __device__ __forceinline__ void pack_store(uint8_t* __restrict__ out, uint64_t d0, uint32_t n, PackChunk v) {
    uint8_t* p = out + d0;
    if (n >= kPackChunk) {
        __builtin_memcpy(__builtin_assume_aligned(p, 16), &v, 16);
        return;
    }
    uint64_t w = v.lo;
    if (n & 8u) {
        __builtin_memcpy(__builtin_assume_aligned(p, 8), &w, 8);
        p += 8;
        w = v.hi;
    }
    if (n & 4u) {
        const uint32_t x = (uint32_t)w;
        __builtin_memcpy(__builtin_assume_aligned(p, 4), &x, 4);
        p += 4;
        w >>= 32;
    }
    if (n & 2u) {
        const uint16_t x = (uint16_t)w;
        __builtin_memcpy(__builtin_assume_aligned(p, 2), &x, 2);
        p += 2;
        w >>= 16;
    }
    if (n & 1u) *p = (uint8_t)w;
}

}  // namespace wq
