// export_ops.hpp — the per-cube and per-row arithmetic of the table export (wq_table_export.hip):
// which table slots hold a live cube, a cube's key and its order-preserving sort words, the cube of
// an output row, a row's peer, the 40-byte row itself and the peer bitmap test. __host__ __device__,
// so tests/cpp/table_export_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/snapshot.py.
//
// The export walks its rows in granules of 64 (one wave step). Cubes are ordered first (world, key
// x, y, z), base[c] = rows of the cubes before c in that order (an exclusive prefix of their counts,
// base[n_cubes] = every row). Row r belongs to the last cube c with base[c] <= r and is that cube's
// peer r - base[c]; a cube's peers are stored ascending, so the rows come out in canonical order.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "wq_device.hpp"

namespace wq {

constexpr uint32_t kExpGranule = 64;  // output rows per granule (one wave step)
constexpr uint32_t kExpRowWords = 5;  // a wq_op as 8-byte words

// The table as the export reads it: slot i < rcap is record i, slot rcap + j is Slot j.
struct ExpTable {
    const Record* recs;
    uint64_t rcap;
    const Slot* slots;
    uint64_t scap;
    const uint32_t* list;
    int64_t cube_size;
};

// The filter on the device: world == kWorldEmpty passes every world; bits == nullptr every peer,
// else bit p % 32 of word p / 32 for p < n_bits (ids past the bitmap match nothing).
struct ExpFilter {
    uint32_t world;
    uint32_t n_bits;
    const uint32_t* bits;
};

// i64 -> u64 keeping the order (the sign flip of a radix sort on signed keys).
__host__ __device__ __forceinline__ uint64_t exp_ord(int64_t v) { return (uint64_t)v ^ (1ull << 63); }

// World and key of table slot i (which holds a cube).
__host__ __device__ __forceinline__ void exp_cube_key(const ExpTable& t, uint64_t i, uint32_t* w, int64_t* k) {
    if (i < t.rcap) {
        const Record& r = t.recs[i];
        uint32_t a[3];
        unpack_key(r.pk, r.ext, w, a);
#pragma unroll
        for (int d = 0; d < 3; ++d) k[d] = ((int64_t)a[d] - (int64_t)kAxisBias) * t.cube_size;
    } else {
        const Slot& s = t.slots[i - t.rcap];
        *w = s.world;
        k[0] = s.k[0];
        k[1] = s.k[1];
        k[2] = s.k[2];
    }
}

// Peers of table slot i when it holds a cube that passes the world filter, else 0 (an empty slot, a
// record that kept its key after its list emptied, another world).
__host__ __device__ __forceinline__ uint32_t exp_cube_count(const ExpTable& t, uint64_t i, uint32_t world) {
    uint32_t w, n;
    if (i < t.rcap) {
        const Record& r = t.recs[i];
        if (!r.ext) return 0;
        w = (r.ext >> 8) - 1u;
        n = r.count;
    } else {
        const Slot& s = t.slots[i - t.rcap];
        if (s.world == kWorldEmpty) return 0;
        w = s.world;
        n = t.list[s.off];
    }
    return (world == kWorldEmpty || world == w) ? n : 0u;
}

// Peer j of the cube in table slot i, which holds n > j peers: a record of at most kInline peers
// keeps them in its inline words only, everything else in its list block.
__host__ __device__ __forceinline__ uint32_t exp_peer(const ExpTable& t, uint64_t i, uint32_t n, uint32_t j) {
    if (i < t.rcap) {
        const Record& r = t.recs[i];
        return n <= (uint32_t)kInline ? r.peers[j] : t.list[(uint64_t)r.list_off + 1 + j];
    }
    return t.list[(uint64_t)t.slots[i - t.rcap].off + 1 + j];
}

// The last c in [lo, hi] with base[c] <= row. Needs base[lo] <= row.
__host__ __device__ __forceinline__ uint32_t exp_cube_of(const uint32_t* __restrict__ base, uint32_t lo, uint32_t hi,
                                                          uint32_t row) {
    while (hi > lo) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (base[mid] <= row)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The cube of `row`, a row of the granule whose first row belongs to cube c0: every cube before the
// padding holds a row, so at most kExpGranule cubes start inside a granule and the search stays in
// base[c0 .. c0 + 63] (one or two cache lines the granule's lanes share). n_cubes = entries of base
// before its final total.
__host__ __device__ __forceinline__ uint32_t exp_cube_in_granule(const uint32_t* __restrict__ base, uint32_t c0,
                                                                  uint32_t n_cubes, uint32_t row) {
    const uint32_t last = n_cubes - 1 - c0 < kExpGranule - 1 ? n_cubes - 1 : c0 + (kExpGranule - 1);
    return exp_cube_of(base, c0, last, row);
}

__host__ __device__ __forceinline__ bool exp_peer_passes(const ExpFilter& f, uint32_t peer) {
    if (!f.bits) return true;
    return peer < f.n_bits && ((f.bits[peer >> 5] >> (peer & 31u)) & 1u);
}

// One exported row: SUBSCRIBE, key_is_raw = 1, the key as the table holds it, padding zero.
__host__ __device__ __forceinline__ void exp_write_row(uint64_t* __restrict__ out, uint64_t idx, uint32_t world,
                                                       uint32_t peer, const int64_t* k) {
    uint64_t* o = out + idx * kExpRowWords;
    o[0] = (uint64_t)world | ((uint64_t)peer << 32);
    o[1] = 1ull << 8;  // kind 0 (WQ_OP_SUBSCRIBE) in byte 0, key_is_raw = 1 in byte 1
    o[2] = (uint64_t)k[0];
    o[3] = (uint64_t)k[1];
    o[4] = (uint64_t)k[2];
}

// Row a before row b by cube: (world, key x, y, z). Rows of one cube compare equal.
__host__ __device__ __forceinline__ bool exp_row_cube_less(const uint64_t* a, const uint64_t* b) {
    const uint32_t wa = (uint32_t)a[0], wb = (uint32_t)b[0];
    if (wa != wb) return wa < wb;
#pragma unroll
    for (int d = 2; d < 5; ++d)
        if (a[d] != b[d]) return (int64_t)a[d] < (int64_t)b[d];
    return false;
}

}  // namespace wq
