// record_ops.hpp — the arithmetic of the record store (wq_records.hip) shared by host and device:
// the reference's two quantisers restated (database/world_region.rs:93-129), the packed (world,
// region) and (world, table) keys, the total order on rows, the bounds of a key's range in a sorted
// view and the ordinal-space helpers of a read. __host__ __device__, so
// tests/cpp/records_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/records.py. Compiled with -ffp-contract=off: clamp_region_coord_dev is an
// f64 op sequence.
//
// A view is an index array over the rows, sorted by (leading key, uuid, ts_us, seq): view 0 leads
// with the region key, view 1 with the table key. The rows of one (key, uuid) are contiguous and
// ascend in (ts_us, seq), so the last one is the row a read returns and the rows a dedupe kills are
// a prefix of the range.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/wq_router.h"
#include "wq_device.hpp"

namespace wq {

constexpr uint32_t kRecGranule = 64;    // ordinals per granule (one wave step)
constexpr uint32_t kRecLaneRange = 64;  // a delete's range up to this long is walked by its lane
constexpr uint32_t kRecMaxOrdinals = 0xFFFFFFC0u;  // the ranges of one read call hold at most this many elements

// Rust's saturating `c as i64` for c >= 0 (not NaN).
__host__ __device__ __forceinline__ int64_t rec_sat_i64(double c) {
    return c >= 9223372036854775808.0 ? INT64_MAX : (int64_t)c;
}

// clamp_region_coord (world_region.rs:93-110) for a non-NaN c: the minimum of c's region. The
// negative side is minus the region of (-c) + size, one f64 add and the positive branch: -0.1 -> -16,
// -16.0 -> -32 at size 16.
__host__ __device__ __forceinline__ int64_t clamp_region_coord_dev(double c, uint16_t size) {
    if (c == 0.0) return 0;
    const int64_t s = (int64_t)size;
    if (c >= 0.0) {
        const int64_t ci = rec_sat_i64(c);
        return ci - ci % s;
    }
    const double nc = (-c) + (double)size;
    const int64_t ci = rec_sat_i64(nc);
    return -(ci - ci % s);
}

// clamp_table_size (world_region.rs:112-129): multiples of the table size stay, the rest goes to
// the multiple below on the positive side and to minus the table of (-c) + size on the negative
// one (-1 -> -1024, -1025 -> -2048). Two's-complement arithmetic where Rust's release build wraps.
__host__ __device__ __forceinline__ int64_t clamp_table_size_dev(int64_t c, int64_t table_size) {
    if (c % table_size == 0) return c;
    if (c >= 0) return c - c % table_size;
    const int64_t nc = (int64_t)((uint64_t)0 - (uint64_t)c + (uint64_t)table_size);
    if (nc < 0) return c;  // wrapped (|c| within a table of 2^63): not a region this store packs
    return (int64_t)((uint64_t)0 - (uint64_t)(nc - nc % table_size));
}

// A store's configuration (wq_records_open).
struct RecCfg {
    uint16_t size[3];
    uint32_t table_size;
};

// A leading key: the router's 96-bit packing (wq_device.hpp pack_key) of a world and three indices.
struct RecPacked {
    uint32_t hi;
    uint64_t lo;
};

// The packed region and table keys of a position, false when it has none: a NaN coordinate, a
// region index outside [-2^23, 2^23) or a world id above kMaxPackedWorld.
__host__ __device__ __forceinline__ bool rec_pack_position(const RecCfg& cfg, uint32_t world, const double* pos,
                                                           RecPacked* region, RecPacked* table) {
    int64_t ri[3], ti[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double c = pos[d];
        if (c != c) return false;
        const int64_t r = clamp_region_coord_dev(c, cfg.size[d]);
        ri[d] = r / (int64_t)cfg.size[d];  // exact: r is a multiple of the size
        if (ri[d] < -(int64_t)kAxisBias || ri[d] >= (int64_t)kAxisBias) return false;
        ti[d] = clamp_table_size_dev(r, (int64_t)cfg.table_size) / (int64_t)cfg.table_size;
    }
    // a table index is within [-2^22 - 1, 2^23): a region minimum that is no multiple of the table
    // size means table_size >= 2 * size
    return pack_key(world, ri[0], ri[1], ri[2], 1.0, &region->lo, &region->hi) &&
           pack_key(world, ti[0], ti[1], ti[2], 1.0, &table->lo, &table->hi);
}

// The rows, a structure of arrays; k_hi / k_lo [0]: region key, [1]: table key.
struct RecRows {
    uint32_t* k_hi[2];
    uint64_t* k_lo[2];
    uint64_t* uuid_hi;
    uint64_t* uuid_lo;
    int64_t* ts;
    uint64_t* seq;
    uint32_t* handle;
    uint32_t* live;  // one byte per row, addressed in words (rec_kill)
};

// What a view sorts by.
struct RecKey {
    uint32_t k_hi;
    uint64_t k_lo, uuid_hi, uuid_lo;
    int64_t ts;
    uint64_t seq;
};

template <int V>
__host__ __device__ __forceinline__ RecKey rec_key(const RecRows& r, uint32_t row) {
    return RecKey{r.k_hi[V][row], r.k_lo[V][row], r.uuid_hi[row], r.uuid_lo[row], r.ts[row], r.seq[row]};
}

// The total order on rows: (leading key, uuid, ts_us, seq). seq is unique, so no two rows are equal.
__host__ __device__ __forceinline__ bool rec_less(const RecKey& a, const RecKey& b) {
    if (a.k_hi != b.k_hi) return a.k_hi < b.k_hi;
    if (a.k_lo != b.k_lo) return a.k_lo < b.k_lo;
    if (a.uuid_hi != b.uuid_hi) return a.uuid_hi < b.uuid_hi;
    if (a.uuid_lo != b.uuid_lo) return a.uuid_lo < b.uuid_lo;
    if (a.ts != b.ts) return a.ts < b.ts;
    return a.seq < b.seq;
}

// First position in view[0, n) whose row is not below `key`.
template <int V>
__host__ __device__ __forceinline__ uint32_t rec_lower_bound(const RecRows& r, const uint32_t* __restrict__ view,
                                                             uint32_t n, const RecKey& key) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (rec_less(rec_key<V>(r, view[mid]), key))
            a = mid + 1;
        else
            b = mid;
    }
    return a;
}

// The smallest key of a leading key, of a (leading key, uuid) and of a (leading key, uuid, ts).
__host__ __device__ __forceinline__ RecKey rec_key_min(const RecPacked& k, uint64_t uuid_hi = 0, uint64_t uuid_lo = 0,
                                                       int64_t ts = INT64_MIN) {
    return RecKey{k.hi, k.lo, uuid_hi, uuid_lo, ts, 0};
}

// The leading key after k (packed keys are below 2^96 - 1: no carry out of hi).
__host__ __device__ __forceinline__ RecPacked rec_key_next(const RecPacked& k) {
    RecPacked n{k.hi, k.lo + 1};
    if (n.lo == 0) n.hi++;
    return n;
}

// [*lo, *hi): the rows of leading key k in the view. lo <= hi <= n always.
template <int V>
__host__ __device__ __forceinline__ void rec_key_range(const RecRows& r, const uint32_t* __restrict__ view, uint32_t n,
                                                       const RecPacked& k, uint32_t* lo, uint32_t* hi) {
    *lo = rec_lower_bound<V>(r, view, n, rec_key_min(k));
    const uint32_t h = rec_lower_bound<V>(r, view, n, rec_key_min(rec_key_next(k)));
    *hi = h < *lo ? *lo : h;
}

// [*lo, *hi): the rows of (k, uuid) with ts_us < ts_end (INT64_MAX and all_ts: every row of the uuid).
template <int V>
__host__ __device__ __forceinline__ void rec_uuid_range(const RecRows& r, const uint32_t* __restrict__ view,
                                                        uint32_t n, const RecPacked& k, uint64_t uuid_hi,
                                                        uint64_t uuid_lo, int64_t ts_end, bool all_ts, uint32_t* lo,
                                                        uint32_t* hi) {
    *lo = rec_lower_bound<V>(r, view, n, rec_key_min(k, uuid_hi, uuid_lo));
    RecKey end = rec_key_min(k, uuid_hi, uuid_lo, ts_end);
    if (all_ts) {
        end.ts = INT64_MAX;
        end.seq = ~0ull;  // above every row: sequence numbers stay below 2^64 - 1
    }
    uint32_t h = rec_lower_bound<V>(r, view, n, end);
    if (all_ts && h < n) {
        const RecKey at = rec_key<V>(r, view[h]);
        if (!rec_less(end, at) && !rec_less(at, end)) ++h;
    }
    *hi = h < *lo ? *lo : h;
}

// [*lo, *hi): the rows of `row`'s (leading key, uuid) that are older than it, the rows a dedupe
// kills. One search finds the end; the start is searched only when the element before the end is of
// the same key and uuid (most rows have no older copy).
template <int V>
__host__ __device__ __forceinline__ void rec_older_range(const RecRows& r, const uint32_t* __restrict__ view,
                                                         uint32_t n, uint32_t row, uint32_t* lo, uint32_t* hi) {
    const RecPacked k{r.k_hi[V][row], r.k_lo[V][row]};
    const uint64_t uh = r.uuid_hi[row], ul = r.uuid_lo[row];
    const uint32_t b = rec_lower_bound<V>(r, view, n, rec_key_min(k, uh, ul, r.ts[row]));
    uint32_t a = b;
    if (b > 0) {
        const uint32_t p = view[b - 1];
        if (r.k_hi[V][p] == k.hi && r.k_lo[V][p] == k.lo && r.uuid_hi[p] == uh && r.uuid_lo[p] == ul) {
            a = rec_lower_bound<V>(r, view, b, rec_key_min(k, uh, ul));
        }
    }
    *lo = a;
    *hi = b;
}

// Marks a row dead; true for the one caller that found it live (an atomic clear of the row's byte
// in its word on the device, the same on the host's single thread).
__host__ __device__ __forceinline__ bool rec_kill(uint32_t* live, uint32_t row) {
    const uint32_t mask = 0xFFu << ((row & 3u) * 8u);
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t old = atomicAnd(&live[row >> 2], ~mask);
#else
    const uint32_t old = live[row >> 2];
    live[row >> 2] = old & ~mask;
#endif
    return (old & mask) != 0;
}

__host__ __device__ __forceinline__ bool rec_is_live(const uint32_t* live, uint32_t row) {
    return ((live[row >> 2] >> ((row & 3u) * 8u)) & 0xFFu) != 0;
}

// ---- vacuum and snapshots (wq_records_vacuum / _export / _import) ----

// Row `src` of `from` becomes row `dst` of `to`: the nine fields and a set live byte (no kill runs
// beside a move, and every lane writes another byte).
__host__ __device__ __forceinline__ void rec_row_move(const RecRows& from, uint32_t src, const RecRows& to,
                                                      uint32_t dst) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        to.k_hi[v][dst] = from.k_hi[v][src];
        to.k_lo[v][dst] = from.k_lo[v][src];
    }
    to.uuid_hi[dst] = from.uuid_hi[src];
    to.uuid_lo[dst] = from.uuid_lo[src];
    to.ts[dst] = from.ts[src];
    to.seq[dst] = from.seq[src];
    to.handle[dst] = from.handle[src];
    reinterpret_cast<uint8_t*>(to.live)[dst] = 1;
}

// A stored row as a snapshot carries it: the region key unpacked to the region's minimum corner.
__host__ __device__ __forceinline__ wq_rec_row rec_row_export(const RecCfg& cfg, const RecRows& r, uint32_t row) {
    wq_rec_row o;
    uint32_t a[3];
    unpack_key(r.k_lo[0][row], r.k_hi[0][row], &o.world, a);
    o.handle = r.handle[row];
#pragma unroll
    for (int d = 0; d < 3; ++d) o.region[d] = ((int64_t)a[d] - (int64_t)kAxisBias) * (int64_t)cfg.size[d];
    o.uuid_hi = r.uuid_hi[row];
    o.uuid_lo = r.uuid_lo[row];
    o.ts_us = r.ts[row];
    o.seq = r.seq[row];
    return o;
}

// The packed keys of a snapshot row in a store of configuration cfg, false when the store does not
// take it: a corner off the region grid, a region index outside [-2^23, 2^23), a world above
// kMaxPackedWorld or a seq that is not below the snapshot's op counter. The keys come from the
// integer indices, never from a position (clamp_region_coord sends -16.0 to region -32), and the
// table from the region, never from the snapshot.
__host__ __device__ __forceinline__ bool rec_row_import(const RecCfg& cfg, const wq_rec_row& in, uint64_t ops_seen,
                                                        RecPacked* region, RecPacked* table) {
    if (in.world > kMaxPackedWorld || in.seq >= ops_seen) return false;
    int64_t ri[3], ti[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int64_t s = (int64_t)cfg.size[d], c = in.region[d];
        if (c % s != 0) return false;
        ri[d] = c / s;
        if (ri[d] < -(int64_t)kAxisBias || ri[d] >= (int64_t)kAxisBias) return false;
        ti[d] = clamp_table_size_dev(c, (int64_t)cfg.table_size) / (int64_t)cfg.table_size;
    }
    return pack_key(in.world, ri[0], ri[1], ri[2], 1.0, &region->lo, &region->hi) &&
           pack_key(in.world, ti[0], ti[1], ti[2], 1.0, &table->lo, &table->hi);
}

// Do elements t - 1 and t of view 0 (t >= 1) compare equal: the same (region key, uuid, ts, seq)?
// Sorted, two such rows are neighbours; an import that holds a pair is refused.
__host__ __device__ __forceinline__ bool rec_adjacent_equal(const RecRows& r, const uint32_t* __restrict__ view,
                                                            uint32_t t) {
    const RecKey a = rec_key<0>(r, view[t - 1]), b = rec_key<0>(r, view[t]);
    return !rec_less(a, b) && !rec_less(b, a);
}

// ---- a read's ordinal space: the queries' ranges laid end to end, pre[i] = elements before query i
// (an exclusive, saturating prefix of the range lengths) ----

__host__ __device__ __forceinline__ uint32_t rec_sat_add(uint32_t a, uint32_t b) {
    const uint64_t s = (uint64_t)a + b;
    return s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
}
struct RecSatAdd {
    __host__ __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return rec_sat_add(a, b); }
};

// What the host sizes the first walk of a read for, not knowing the ranges' total: every live row
// twice (the same region may be asked twice) and a granule per query, a multiple of the granule. A
// call whose total is above it walks a second time with the total (wq_records.hip); the result is
// the same either way.
__host__ __device__ __forceinline__ uint32_t rec_ordinal_guess(uint64_t n_view, uint64_t n_queries) {
    const uint64_t l = (2 * n_view + kRecGranule * n_queries + (kRecGranule - 1)) & ~(uint64_t)(kRecGranule - 1);
    return l > kRecMaxOrdinals ? kRecMaxOrdinals : (uint32_t)l;
}

// The query of ordinal q: the last i in [lo, hi] with pre[i] <= q. Needs pre[lo] <= q.
__host__ __device__ __forceinline__ uint32_t rec_query_of(const uint32_t* __restrict__ pre, uint32_t lo, uint32_t hi,
                                                          uint32_t q) {
    while (hi > lo) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (pre[mid] <= q)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// Is element e of a query's range [.., hi) of view 0 the row the read returns for its uuid — the
// last row of the uuid in the region — and newer than `after`?
__host__ __device__ __forceinline__ bool rec_is_winner(const RecRows& r, const uint32_t* __restrict__ view, uint32_t e,
                                                       uint32_t hi, int64_t after) {
    const uint32_t row = view[e];
    if (!(r.ts[row] > after)) return false;
    if (e + 1 >= hi) return true;
    const uint32_t nx = view[e + 1];
    return r.uuid_hi[nx] != r.uuid_hi[row] || r.uuid_lo[nx] != r.uuid_lo[row];
}

// Winners before ordinal q (q <= the total): the output offset of the query that starts there.
__host__ __device__ __forceinline__ uint32_t rec_kept_before(const uint32_t* __restrict__ base,
                                                             const uint64_t* __restrict__ flags, uint32_t q) {
    const uint32_t g = q / kRecGranule, b = q % kRecGranule;
    uint32_t n = base[g];
    if (b) n += (uint32_t)__builtin_popcountll(flags[g] & ((1ull << b) - 1ull));
    return n;
}

}  // namespace wq
