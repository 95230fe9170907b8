// wq_records.hip — the record store: RecordCreate / RecordRead / RecordDelete on the GPU.
//
// The reference sends these to DatabaseClient and PostgreSQL (database/client.rs, navigation.rs,
// world_region.rs, query_constants.rs). Here a stored record is one row {region key, table key,
// uuid, ts_us, seq, handle, live byte} of a grow-only structure of arrays; its payload stays with
// the caller under `handle`. Two index arrays over the rows are kept sorted (record_ops.hpp): view 0
// by (region key, uuid, ts_us, seq), view 1 by (table key, uuid, ts_us, seq).
//
//   apply   classify  one lane per op: quantise, pack both keys, reject what has none
//           scan      the creates' row slots
//           append    the creates become rows (op order = seq order)
//           sort      the batch only: stable rocPRIM radix passes over ts, uuid and the leading key
//           merge     batch and view by rank: each side's elements binary-search their rank in the
//                     other side, element-parallel, into the view's second buffer
//           delete    one lane per delete op finds its (region, uuid) range in view 0 and kills the
//                     rows with a lower seq; a range longer than a wave goes to a wave per op
//   read    compact   rows killed since the last merge leave both views (flag / scan / scatter)
//           range     one lane per query: quantise, pack, two searches in view 0
//           scan      the ranges' lengths: the call's ordinal space
//           flag      a wave per granule of 64 ordinals: a lane's element is a winner when it is the
//                     last row of its uuid in the range and newer than `after`; the ballot is the
//                     granule's flag word
//           scan      the granule counts
//           emit      a wave per granule stores its winners as one contiguous run; one lane per query
//                     derives its offset from the same prefix
//           dedupe    each winner's (table, uuid) range in view 1: the rows older than it die
//   vacuum  flag      one lane per stored row reads its live byte
//           scan      each live row's new index, which is also the views' old-to-new map
//           move      the live rows into fresh arrays (export: into the caller's wq_rec_row array)
//           remap     both views through the map
//   import  classify  one lane per snapshot row: validate, pack both keys from the integer indices
//           scan / append / sort   as the apply, the sort keys read from the rows (seq is a pass too)
//           check     no two neighbours of view 0 compare equal
//
// No lane, wave or block owns a region. Placement comes from prefix sums alone, so two calls give
// the same bytes. An apply reads nothing back; a read reads its totals once, at its end.
#include "record_ops.hpp"
#include "table_prims.hpp"

namespace wq {

// The store's counters on the device. An apply zeroes batch_m and n_long, a read [r_returned, end).
struct RecCtl {
    uint32_t n_rows;  // rows stored
    uint32_t n_view;  // entries of each view
    uint32_t n_dead;  // entries of the dead list
    uint32_t n_view_next;
    uint64_t live;
    uint32_t batch_m;  // creates of the apply in flight
    uint32_t n_long;   // its deletes whose range is longer than a lane walks
    uint64_t created, deleted_rows, rejected;  // since the store was opened (never zeroed)
    uint32_t imp_rejected, imp_dup;            // an import's rejected rows and its pairs of equal rows
    uint64_t r_returned, r_deduped, r_rejected, r_scanned;
    uint32_t r_overflow;
    uint32_t r_cut;       // the walk stopped below the ranges' total
    uint32_t r_ordinals;  // that total (saturating)
    uint32_t pad_;
};

struct RecStore {
    RecCfg cfg;
    DevBuf k_hi[2], k_lo[2], uuid_hi, uuid_lo, ts, seq, handle, live, dead;
    uint64_t row_cap = 0;
    uint64_t dead_extra = 0;  // the dead list holds row_cap + dead_extra entries (a vacuum keeps the undrained ones)
    DevBuf view[2][2];  // [view][buffer]: `cur` is in use, a merge or compaction writes the other
    int cur = 0;
    uint64_t view_cap = 0;
    // what the host knows without reading back: upper bounds (exact after a call that reads its totals)
    uint64_t rows_ub = 0, view_ub = 0;
    uint64_t ops_seen = 0;
    bool dirty = false;  // rows may have died since the views were last compacted
    uint64_t tot_deduped = 0, tot_rejected_queries = 0;  // over every read call (each reads its totals)
    DevBuf ctl;
    RecCtl* pinned = nullptr;
    // an apply's scratch
    DevBuf b_hi[2], b_lo[2], b_flag, b_pos, b_i[3], b_key[2], b_sorted[2], b_long;
    // a read's scratch
    DevBuf q_lo, q_len, q_pre, g_cnt, g_base, g_flags;
    // host forms' staging
    DevBuf in, out;
};

namespace {

constexpr int kRecWaves = kBlock / 64;
constexpr unsigned kRecMaxBlocks = 4096;

RecRows rows_of(RecStore* s) {
    RecRows r;
    for (int v = 0; v < 2; ++v) {
        r.k_hi[v] = s->k_hi[v].as<uint32_t>();
        r.k_lo[v] = s->k_lo[v].as<uint64_t>();
    }
    r.uuid_hi = s->uuid_hi.as<uint64_t>();
    r.uuid_lo = s->uuid_lo.as<uint64_t>();
    r.ts = s->ts.as<int64_t>();
    r.seq = s->seq.as<uint64_t>();
    r.handle = s->handle.as<uint32_t>();
    r.live = s->live.as<uint32_t>();
    return r;
}

struct RecBatchKeys {
    uint32_t* hi[2];  // hi[0][i] == 0: op i has no key (rejected)
    uint64_t* lo[2];
};

uint32_t dead_cap_of(const RecStore* s) { return (uint32_t)std::min<uint64_t>(s->row_cap + s->dead_extra, 0xFFFFFFFFull); }

// Kills a row once: the caller that found it live appends its handle to the dead list.
__device__ __forceinline__ uint32_t kill_row(const RecRows& r, uint32_t row, RecCtl* ctl, uint32_t* dead,
                                             uint32_t dead_cap) {
    if (!rec_kill(r.live, row)) return 0;
    const uint32_t d = atomicAdd(&ctl->n_dead, 1u);
    if (d < dead_cap) dead[d] = r.handle[row];
    return 1;
}

// ---- apply ----

__global__ __launch_bounds__(kBlock) void k_rec_classify(RecCfg cfg, const wq_rec_op* __restrict__ ops, uint32_t n,
                                                         RecBatchKeys b, uint32_t* flag, RecCtl* ctl) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool rejected = false;
    if (i < n) {
        const wq_rec_op op = ops[i];
        RecPacked rk{0, 0}, tk{0, 0};
        const bool ok = op.kind <= WQ_RECORD_DELETE && rec_pack_position(cfg, op.world, op.pos, &rk, &tk);
        rejected = !ok;
        b.hi[0][i] = ok ? rk.hi : 0u;
        b.lo[0][i] = rk.lo;
        b.hi[1][i] = ok ? tk.hi : 0u;
        b.lo[1][i] = tk.lo;
        flag[i] = ok && op.kind == WQ_RECORD_CREATE ? 1u : 0u;
    }
    const uint64_t w = __ballot(rejected);
    if ((threadIdx.x & 63u) == 0 && w) atomicAdd((unsigned long long*)&ctl->rejected, (unsigned long long)__popcll(w));
}

__global__ __launch_bounds__(kBlock) void k_rec_append(const wq_rec_op* __restrict__ ops, uint32_t n, RecBatchKeys b,
                                                       const uint32_t* __restrict__ flag,
                                                       const uint32_t* __restrict__ pos, RecRows r, uint64_t row_cap,
                                                       uint64_t seq0, RecCtl* ctl) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) {
        const uint32_t m = pos[i] + flag[i];
        ctl->batch_m = m;
        ctl->created += m;
    }
    if (!flag[i]) return;
    const uint64_t row = (uint64_t)ctl->n_rows + pos[i];
    if (row >= row_cap) return;  // never: the host sized the rows for every op of the batch
    const wq_rec_op op = ops[i];
    for (int v = 0; v < 2; ++v) {
        r.k_hi[v][row] = b.hi[v][i];
        r.k_lo[v][row] = b.lo[v][i];
    }
    r.uuid_hi[row] = op.uuid_hi;
    r.uuid_lo[row] = op.uuid_lo;
    r.ts[row] = op.ts_us;
    r.seq[row] = seq0 + i;
    r.handle[row] = op.handle;
    reinterpret_cast<uint8_t*>(r.live)[row] = 1;  // no kill runs beside an append
}

// A snapshot row's seq; an op has none of its own (a batch ascends in it by construction).
__host__ __device__ __forceinline__ uint64_t rec_op_seq(const wq_rec_op&) { return 0; }
__host__ __device__ __forceinline__ uint64_t rec_op_seq(const wq_rec_row& r) { return r.seq; }

// One key word of the batch's ops in the order `idx`: 0 ts_us (biased), 1 uuid_lo, 2 uuid_hi, 3 / 5
// the low word of the region / table key, 4 / 6 its high word, above every key for an op that is
// no accepted create (those sort to the end). Op is wq_rec_op or, for an import, wq_rec_row, whose
// word 7 is its seq (a snapshot's rows need not ascend in it).
template <typename Op>
__global__ __launch_bounds__(kBlock) void k_rec_sortkey(const Op* __restrict__ ops,
                                                        const uint32_t* __restrict__ idx, uint32_t n, int word,
                                                        RecBatchKeys b, const uint32_t* __restrict__ flag,
                                                        uint64_t* out) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = idx[j];
    uint64_t k;
    switch (word) {
        case 0: k = (uint64_t)ops[i].ts_us ^ (1ull << 63); break;
        case 1: k = ops[i].uuid_lo; break;
        case 2: k = ops[i].uuid_hi; break;
        case 3: k = b.lo[0][i]; break;
        case 4: k = flag[i] ? b.hi[0][i] : 1ull << 32; break;
        case 5: k = b.lo[1][i]; break;
        case 7: k = rec_op_seq(ops[i]); break;
        default: k = flag[i] ? b.hi[1][i] : 1ull << 32; break;
    }
    out[j] = k;
}

// The sorted creates' op indices become their row indices.
__global__ __launch_bounds__(kBlock) void k_rec_map(uint32_t* s0, uint32_t* s1, uint32_t n,
                                                    const uint32_t* __restrict__ pos, const RecCtl* ctl) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n || j >= ctl->batch_m) return;
    s0[j] = ctl->n_rows + pos[s0[j]];
    s1[j] = ctl->n_rows + pos[s1[j]];
}

// Merge by rank: element t of the old view goes to t + its rank among the batch, element j of the
// batch to j + its rank in the old view (no two rows compare equal).
template <int V>
__global__ __launch_bounds__(kBlock) void k_rec_merge(RecRows r, const uint32_t* __restrict__ old,
                                                      const uint32_t* __restrict__ batch, uint32_t* out,
                                                      uint64_t out_cap, const RecCtl* ctl) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t nv = ctl->n_view, m = ctl->batch_m;
    if (t >= (uint64_t)nv + m) return;
    uint32_t row;
    uint64_t p;
    if (t < nv) {
        row = old[t];
        p = t + rec_lower_bound<V>(r, batch, m, rec_key<V>(r, row));
    } else {
        const uint32_t j = (uint32_t)(t - nv);
        row = batch[j];
        p = (uint64_t)j + rec_lower_bound<V>(r, old, nv, rec_key<V>(r, row));
    }
    if (p < out_cap) out[p] = row;
}

__global__ void k_rec_commit(RecCtl* ctl) {
    const uint32_t m = ctl->batch_m;
    ctl->n_rows += m;
    ctl->n_view += m;
    ctl->live += m;
}

__device__ __forceinline__ void count_kills(RecCtl* ctl, uint64_t* counter, uint32_t k) {
    if (!k) return;
    atomicAdd((unsigned long long*)counter, (unsigned long long)k);
    atomicAdd((unsigned long long*)&ctl->live, (unsigned long long)(0ull - k));
}

__global__ __launch_bounds__(kBlock) void k_rec_delete(const wq_rec_op* __restrict__ ops, uint32_t n, RecBatchKeys b,
                                                       RecRows r, const uint32_t* __restrict__ view, uint64_t seq0,
                                                       RecCtl* ctl, uint32_t* dead, uint32_t dead_cap,
                                                       uint32_t* long_ops) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || b.hi[0][i] == 0 || ops[i].kind != WQ_RECORD_DELETE) return;
    uint32_t lo, hi;
    rec_uuid_range<0>(r, view, ctl->n_view, RecPacked{b.hi[0][i], b.lo[0][i]}, ops[i].uuid_hi, ops[i].uuid_lo, 0, true,
                      &lo, &hi);
    if (hi - lo > kRecLaneRange) {
        long_ops[atomicAdd(&ctl->n_long, 1u)] = i;  // at most n entries
        return;
    }
    const uint64_t seq = seq0 + i;
    uint32_t k = 0;
    for (uint32_t e = lo; e < hi; ++e) {
        const uint32_t row = view[e];
        if (r.seq[row] < seq) k += kill_row(r, row, ctl, dead, dead_cap);
    }
    count_kills(ctl, &ctl->deleted_rows, k);
}

// The deletes with a long range: a wave per op, its lanes stride the range.
__global__ __launch_bounds__(kBlock) void k_rec_delete_long(const wq_rec_op* __restrict__ ops, RecBatchKeys b,
                                                            RecRows r, const uint32_t* __restrict__ view,
                                                            uint64_t seq0, RecCtl* ctl, uint32_t* dead,
                                                            uint32_t dead_cap, const uint32_t* __restrict__ long_ops) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * kRecWaves;
    const uint32_t n_long = ctl->n_long;
    for (uint32_t w = blockIdx.x * kRecWaves + (threadIdx.x >> 6); w < n_long; w += n_waves) {
        const uint32_t i = long_ops[w];
        uint32_t lo, hi;  // every lane runs the same search: the same addresses, one request
        rec_uuid_range<0>(r, view, ctl->n_view, RecPacked{b.hi[0][i], b.lo[0][i]}, ops[i].uuid_hi, ops[i].uuid_lo, 0,
                          true, &lo, &hi);
        const uint64_t seq = seq0 + i;
        uint32_t k = 0;
        for (uint32_t e = lo + lane; e < hi; e += 64) {
            const uint32_t row = view[e];
            if (r.seq[row] < seq) k += kill_row(r, row, ctl, dead, dead_cap);
        }
        count_kills(ctl, &ctl->deleted_rows, k);
    }
}

// ---- compaction ----

__global__ __launch_bounds__(kBlock) void k_rec_cflag(const uint32_t* __restrict__ view,
                                                      const uint32_t* __restrict__ live, uint32_t n_ub,
                                                      const RecCtl* ctl, uint32_t* flag) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_ub) return;
    flag[t] = t < ctl->n_view && rec_is_live(live, view[t]) ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void k_rec_cscatter(const uint32_t* __restrict__ view,
                                                         const uint32_t* __restrict__ flag,
                                                         const uint32_t* __restrict__ pos, uint32_t n_ub, uint32_t* out,
                                                         RecCtl* ctl) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_ub) return;
    if (flag[t]) out[pos[t]] = view[t];  // pos[t] <= t
    if (t == n_ub - 1) ctl->n_view_next = pos[t] + flag[t];
}

__global__ void k_rec_cset(RecCtl* ctl) { ctl->n_view = ctl->n_view_next; }

// ---- vacuum and export: a stable compaction of the rows by their live byte ----

// One lane per stored row; the exclusive scan of the flags is each live row's new index and the
// old-to-new map of the views.
__global__ __launch_bounds__(kBlock) void k_rec_vflag(const uint32_t* __restrict__ live, uint64_t n_rows,
                                                      uint32_t* flag) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < n_rows) flag[t] = rec_is_live(live, (uint32_t)t) ? 1u : 0u;
}

// Coalesced loads, stores in monotone runs, into fresh arrays: map[t] <= t does not make a parallel
// move in place safe.
__global__ __launch_bounds__(kBlock) void k_rec_vmove(RecRows from, RecRows to, const uint32_t* __restrict__ map,
                                                      uint64_t n_rows, uint64_t to_cap) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_rows || !rec_is_live(from.live, (uint32_t)t)) return;
    const uint32_t p = map[t];
    if (p < to_cap) rec_row_move(from, (uint32_t)t, to, p);
}

// The path's one gather: 4-byte reads over the map.
__global__ __launch_bounds__(kBlock) void k_rec_vremap(const uint32_t* __restrict__ view,
                                                       const uint32_t* __restrict__ map, uint64_t n, uint64_t n_rows,
                                                       uint32_t* out) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const uint32_t row = view[t];
    if (row < n_rows) out[t] = map[row];
}

__global__ void k_rec_vset(RecCtl* ctl, uint32_t n_rows) { ctl->n_rows = n_rows; }

// The move's walk storing one wq_rec_row per live row: four 16-byte stores.
__global__ __launch_bounds__(kBlock) void k_rec_export(RecCfg cfg, RecRows r, const uint32_t* __restrict__ map,
                                                       uint64_t n_rows, wq_rec_row* out, uint64_t capacity) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_rows || !rec_is_live(r.live, (uint32_t)t)) return;
    const uint32_t p = map[t];
    if (p >= capacity) return;
    const wq_rec_row o = rec_row_export(cfg, r, (uint32_t)t);
    auto lo = [](uint64_t v) { return (uint32_t)v; };
    auto hi = [](uint64_t v) { return (uint32_t)(v >> 32); };
    const uint64_t r0 = (uint64_t)o.region[0], r1 = (uint64_t)o.region[1], r2 = (uint64_t)o.region[2];
    uint4* dst = reinterpret_cast<uint4*>(out + p);
    dst[0] = make_uint4(o.world, o.handle, lo(r0), hi(r0));
    dst[1] = make_uint4(lo(r1), hi(r1), lo(r2), hi(r2));
    dst[2] = make_uint4(lo(o.uuid_hi), hi(o.uuid_hi), lo(o.uuid_lo), hi(o.uuid_lo));
    dst[3] = make_uint4(lo((uint64_t)o.ts_us), hi((uint64_t)o.ts_us), lo(o.seq), hi(o.seq));
}

// ---- import: the bulk build of both views from a snapshot ----

__global__ __launch_bounds__(kBlock) void k_rec_iclassify(RecCfg cfg, const wq_rec_row* __restrict__ rows, uint32_t n,
                                                          uint64_t ops_seen, RecBatchKeys b, uint32_t* flag,
                                                          RecCtl* ctl) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool rejected = false;
    if (i < n) {
        RecPacked rk{0, 0}, tk{0, 0};
        const bool ok = rec_row_import(cfg, rows[i], ops_seen, &rk, &tk);
        rejected = !ok;
        b.hi[0][i] = ok ? rk.hi : 0u;
        b.lo[0][i] = rk.lo;
        b.hi[1][i] = ok ? tk.hi : 0u;
        b.lo[1][i] = tk.lo;
        flag[i] = ok ? 1u : 0u;
    }
    const uint64_t w = __ballot(rejected);
    if ((threadIdx.x & 63u) == 0 && w) atomicAdd(&ctl->imp_rejected, (uint32_t)__popcll(w));
}

// The accepted rows in the given order, each under its own seq (the store is empty: row = pos).
__global__ __launch_bounds__(kBlock) void k_rec_iappend(const wq_rec_row* __restrict__ rows, uint32_t n,
                                                        RecBatchKeys b, const uint32_t* __restrict__ flag,
                                                        const uint32_t* __restrict__ pos, RecRows r, uint64_t row_cap,
                                                        RecCtl* ctl) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) ctl->batch_m = pos[i] + flag[i];
    if (!flag[i]) return;
    const uint32_t row = pos[i];
    if (row >= row_cap) return;  // never: the host sized the rows for the whole snapshot
    const wq_rec_row in = rows[i];
    for (int v = 0; v < 2; ++v) {
        r.k_hi[v][row] = b.hi[v][i];
        r.k_lo[v][row] = b.lo[v][i];
    }
    r.uuid_hi[row] = in.uuid_hi;
    r.uuid_lo[row] = in.uuid_lo;
    r.ts[row] = in.ts_us;
    r.seq[row] = in.seq;
    r.handle[row] = in.handle;
    reinterpret_cast<uint8_t*>(r.live)[row] = 1;
}

// The sorted snapshot indices become row indices, straight into the (empty) views.
__global__ __launch_bounds__(kBlock) void k_rec_iviews(const uint32_t* __restrict__ s0,
                                                       const uint32_t* __restrict__ s1, uint32_t n,
                                                       const uint32_t* __restrict__ pos, const RecCtl* ctl,
                                                       uint32_t* v0, uint32_t* v1, uint64_t view_cap) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n || j >= ctl->batch_m || j >= view_cap) return;
    v0[j] = pos[s0[j]];
    v1[j] = pos[s1[j]];
}

// No two neighbours of view 0 may compare equal: a ballot per wave, one atomic per wave.
__global__ __launch_bounds__(kBlock) void k_rec_icheck(RecRows r, const uint32_t* __restrict__ v0, uint32_t n,
                                                       RecCtl* ctl) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const bool dup = t >= 1 && t < n && t < ctl->batch_m && rec_adjacent_equal(r, v0, t);
    const uint64_t w = __ballot(dup);
    if ((threadIdx.x & 63u) == 0 && w) atomicAdd(&ctl->imp_dup, (uint32_t)__popcll(w));
}

// ---- read ----

__global__ __launch_bounds__(kBlock) void k_rec_range(RecCfg cfg, const uint32_t* __restrict__ world,
                                                      const double* __restrict__ pos, uint32_t n, RecRows r,
                                                      const uint32_t* __restrict__ view, RecCtl* ctl, uint32_t* q_lo,
                                                      uint32_t* q_len) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool rejected = false;
    if (i <= n) {
        uint32_t lo = 0, hi = 0;
        if (i < n) {
            const double p[3] = {pos[3ull * i], pos[3ull * i + 1], pos[3ull * i + 2]};
            RecPacked rk, tk;
            if (rec_pack_position(cfg, world[i], p, &rk, &tk))
                rec_key_range<0>(r, view, ctl->n_view, rk, &lo, &hi);
            else
                rejected = true;
        }
        q_lo[i] = lo;
        q_len[i] = hi - lo;
    }
    const uint64_t w = __ballot(rejected);
    if ((threadIdx.x & 63u) == 0 && w)
        atomicAdd((unsigned long long*)&ctl->r_rejected, (unsigned long long)__popcll(w));
}

// The element of ordinal q (below the total): its query in *qi, its position in view 0 returned and
// the end of its query's range in *hi. The granule's queries are [rlo, rhi].
__device__ __forceinline__ uint32_t ordinal_element(const uint32_t* __restrict__ pre,
                                                    const uint32_t* __restrict__ q_lo,
                                                    const uint32_t* __restrict__ q_len, uint32_t rlo, uint32_t rhi,
                                                    uint32_t q, uint32_t* qi, uint32_t* hi) {
    const uint32_t i = rec_query_of(pre, rlo, rhi, q);
    *qi = i;
    *hi = q_lo[i] + q_len[i];
    return q_lo[i] + (q - pre[i]);
}

// The queries [rlo, rhi] the granule starting at ordinal q0 touches: lane 0 searches the first
// ordinal's query and lane 63 the last one's (the other lanes repeat lane 0's search).
__device__ __forceinline__ void granule_queries(const uint32_t* __restrict__ pre, uint32_t n, uint32_t T, uint32_t q0,
                                                uint32_t lane, uint32_t& rlo, uint32_t& rhi) {
    const uint32_t last = T - q0 > kRecGranule ? q0 + kRecGranule - 1 : T - 1;
    const uint32_t i = rec_query_of(pre, 0, n - 1, lane == 63 ? last : q0);
    rlo = __shfl(i, 0);
    rhi = __shfl(i, 63);
}

__global__ __launch_bounds__(kBlock) void k_rec_flag(RecRows r, const uint32_t* __restrict__ view,
                                                     const uint32_t* __restrict__ pre,
                                                     const uint32_t* __restrict__ q_lo,
                                                     const uint32_t* __restrict__ q_len,
                                                     const int64_t* __restrict__ after, uint32_t n, uint32_t lim,
                                                     uint32_t nG, uint64_t* flags, uint32_t* cnt, RecCtl* ctl) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * kRecWaves;
    const uint32_t T = pre[n] < lim ? pre[n] : lim;
    const uint32_t nv = ctl->n_view;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->r_ordinals = pre[n];
        if (pre[n] > lim) ctl->r_cut = 1;
    }
    for (uint32_t g = blockIdx.x * kRecWaves + (threadIdx.x >> 6); g < nG; g += n_waves) {
        const uint64_t q0 = (uint64_t)g * kRecGranule;
        uint64_t word = 0;
        if (q0 < T) {  // wave-uniform
            uint32_t rlo, rhi;
            granule_queries(pre, n, T, (uint32_t)q0, lane, rlo, rhi);
            const uint32_t q = (uint32_t)q0 + lane;
            bool win = false;
            if (q < T) {
                uint32_t qi, hi;
                const uint32_t e = ordinal_element(pre, q_lo, q_len, rlo, rhi, q, &qi, &hi);
                if (e < hi && hi <= nv) win = rec_is_winner(r, view, e, hi, after ? after[qi] : INT64_MIN);
            }
            word = __ballot(win);
            if (lane == 0) flags[g] = word;
        }
        if (lane == 0) cnt[g] = (uint32_t)__popcll(word);
    }
}

__global__ __launch_bounds__(kBlock) void k_rec_emit(RecRows r, const uint32_t* __restrict__ view,
                                                     const uint32_t* __restrict__ pre,
                                                     const uint32_t* __restrict__ q_lo,
                                                     const uint32_t* __restrict__ q_len, uint32_t n, uint32_t lim,
                                                     const uint64_t* __restrict__ flags,
                                                     const uint32_t* __restrict__ base, uint32_t* offsets,
                                                     uint32_t* handles, int64_t* ts, uint64_t capacity, RecCtl* ctl) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * kRecWaves;
    const uint32_t T = pre[n] < lim ? pre[n] : lim;
    const uint32_t nGs = T / kRecGranule + (T % kRecGranule ? 1u : 0u);
    for (uint32_t g = blockIdx.x * kRecWaves + (threadIdx.x >> 6); g < nGs; g += n_waves) {
        const uint64_t word = flags[g];
        if (!word) continue;  // wave-uniform
        const uint32_t q0 = g * kRecGranule;
        uint32_t rlo, rhi;
        granule_queries(pre, n, T, q0, lane, rlo, rhi);
        if ((word >> lane) & 1ull) {
            uint32_t qi, hi;
            const uint32_t row = view[ordinal_element(pre, q_lo, q_len, rlo, rhi, q0 + lane, &qi, &hi)];
            // the winners' positions are consecutive: one contiguous run per wave
            const uint64_t p = (uint64_t)base[g] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
            if (p < capacity) {
                handles[p] = r.handle[row];
                ts[p] = r.ts[row];
            }
        }
    }
    const uint64_t n_threads = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += n_threads) {
        const uint32_t o = rec_kept_before(base, flags, pre[i] < T ? pre[i] : T);
        offsets[i] = o;
        if (i == n) {
            ctl->r_returned = o;
            ctl->r_scanned = T;
            ctl->r_overflow = o > capacity ? 1u : 0u;
        }
    }
}

// Every winner (the capacity does not matter here) kills the rows of its uuid in its table that are
// older than it: a prefix [a, b) of the (table, uuid) range in view 1. The wave walks each winner's
// prefix together, so a prefix of 5,000 rows costs what 5,000 prefixes of one row do.
__global__ __launch_bounds__(kBlock) void k_rec_dedupe(RecRows r, const uint32_t* __restrict__ view0,
                                                       const uint32_t* __restrict__ view1,
                                                       const uint32_t* __restrict__ pre,
                                                       const uint32_t* __restrict__ q_lo,
                                                       const uint32_t* __restrict__ q_len, uint32_t n, uint32_t lim,
                                                       const uint64_t* __restrict__ flags, RecCtl* ctl, uint32_t* dead,
                                                       uint32_t dead_cap) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * kRecWaves;
    const uint32_t T = pre[n] < lim ? pre[n] : lim;
    const uint32_t nGs = T / kRecGranule + (T % kRecGranule ? 1u : 0u);
    if (pre[n] > lim) return;  // a cut walk kills nothing: the call walks again with the whole total
    const uint32_t nv = ctl->n_view;
    for (uint32_t g = blockIdx.x * kRecWaves + (threadIdx.x >> 6); g < nGs; g += n_waves) {
        const uint64_t word = flags[g];
        if (!word) continue;  // wave-uniform
        const uint32_t q0 = g * kRecGranule;
        uint32_t rlo, rhi;
        granule_queries(pre, n, T, q0, lane, rlo, rhi);
        uint32_t a = 0, b = 0;
        if ((word >> lane) & 1ull) {
            uint32_t qi, hi;
            const uint32_t row = view0[ordinal_element(pre, q_lo, q_len, rlo, rhi, q0 + lane, &qi, &hi)];
            rec_older_range<1>(r, view1, nv, row, &a, &b);
        }
        uint64_t todo = __ballot(b > a);
        uint32_t k = 0;
        while (todo) {
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t sa = __shfl(a, src), sb = __shfl(b, src);
            for (uint32_t e = sa + lane; e < sb; e += 64) k += kill_row(r, view1[e], ctl, dead, dead_cap);
        }
        count_kills(ctl, &ctl->r_deduped, k);
    }
}

// ---- host side ----

// Grows a buffer to `bytes`, keeping its first `keep` bytes (DevBuf::ensure alone does not keep them).
int grow_keep(wq_router* h, DevBuf& b, size_t bytes, size_t keep) {
    if (bytes <= b.bytes) return WQ_OK;
    DevBuf nb;
    WQ_ALLOC(h, nb, bytes);
    keep = keep < b.bytes ? keep : b.bytes;
    if (b.p && keep) {
        hipError_t e = hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            nb.release();
            return set_error(h, WQ_E_HIP, "record store growth copy", e);
        }
    } else if (b.p) {
        WQ_HIP(h, hipStreamSynchronize(h->stream));  // kernels in flight may still use the old buffer
    }
    b.release();
    b = nb;
    return WQ_OK;
}

int ensure_rows(wq_router* h, RecStore* s, uint64_t need) {
    if (need <= s->row_cap) return WQ_OK;
    const uint64_t cap = (std::max<uint64_t>(2 * s->row_cap, std::max<uint64_t>(need, 1024)) + 3) & ~3ull;
    const uint64_t have = s->rows_ub;
    for (int v = 0; v < 2; ++v) {
        if (int rc = grow_keep(h, s->k_hi[v], cap * 4, have * 4)) return rc;
        if (int rc = grow_keep(h, s->k_lo[v], cap * 8, have * 8)) return rc;
    }
    for (DevBuf* b : {&s->uuid_hi, &s->uuid_lo, &s->ts, &s->seq})
        if (int rc = grow_keep(h, *b, cap * 8, have * 8)) return rc;
    if (int rc = grow_keep(h, s->handle, cap * 4, have * 4)) return rc;
    if (int rc = grow_keep(h, s->live, cap, (have + 3) & ~3ull)) return rc;
    // every row dies at most once
    if (int rc = grow_keep(h, s->dead, (cap + s->dead_extra) * 4, (have + s->dead_extra) * 4)) return rc;
    s->row_cap = cap;
    return WQ_OK;
}

int ensure_views(wq_router* h, RecStore* s, uint64_t need) {
    if (need <= s->view_cap) return WQ_OK;
    const uint64_t cap = std::max<uint64_t>(2 * s->view_cap, std::max<uint64_t>(need, 1024));
    for (int v = 0; v < 2; ++v) {
        if (int rc = grow_keep(h, s->view[v][s->cur], cap * 4, s->view_ub * 4)) return rc;
        if (int rc = grow_keep(h, s->view[v][s->cur ^ 1], cap * 4, 0)) return rc;
    }
    s->view_cap = cap;
    return WQ_OK;
}

template <typename Op>
int sort_pass(wq_router* h, RecStore* s, const Op* d_ops, uint32_t n, int word, int end_bit, RecBatchKeys b,
              const uint32_t* in, uint32_t* out) {
    hipLaunchKernelGGL(k_rec_sortkey<Op>, dim3(grid_for(n)), dim3(kBlock), 0, h->stream, d_ops, in, n, word, b,
                       s->b_flag.as<uint32_t>(), s->b_key[0].as<uint64_t>());
    WQ_HIP(h, hipGetLastError());
    return sort_pairs<uint64_t>(h, s->b_key[0].as<uint64_t>(), s->b_key[1].as<uint64_t>(), in, out, n, end_bit);
}

int read_ctl(wq_router* h, RecStore* s) {
    WQ_HIP(h, hipMemcpyAsync(s->pinned, s->ctl.p, sizeof(RecCtl), hipMemcpyDeviceToHost, h->stream));
    WQ_HIP(h, hipStreamSynchronize(h->stream));
    s->rows_ub = s->pinned->n_rows;
    s->view_ub = s->pinned->n_view;
    s->dirty = s->pinned->live != s->pinned->n_view;  // the views hold every live row and the dead not yet compacted
    return WQ_OK;
}

// The apply on a device array (the handle's device is current): asynchronous, nothing read back.
int records_apply_device(wq_router* h, const wq_rec_op* d_ops, size_t n_ops) {
    RecStore* s = h->rec;
    hipStream_t st = h->stream;
    if (n_ops == 0) return WQ_OK;
    if (s->rows_ub + n_ops >= 0xFFFFFFFFull || s->view_ub + n_ops >= 0xFFFFFFFFull)
        return set_error(h, WQ_E_CAPACITY, "the record store holds fewer than 2^32 - 1 rows");
    const uint32_t n = (uint32_t)n_ops;
    if (int rc = ensure_rows(h, s, s->rows_ub + n)) return rc;
    if (int rc = ensure_views(h, s, s->view_ub + n)) return rc;
    for (int v = 0; v < 2; ++v) {
        WQ_ALLOC(h, s->b_hi[v], (size_t)n * 4);
        WQ_ALLOC(h, s->b_lo[v], (size_t)n * 8);
        WQ_ALLOC(h, s->b_key[v], (size_t)n * 8);
        WQ_ALLOC(h, s->b_sorted[v], (size_t)n * 4);
    }
    for (DevBuf* b : {&s->b_flag, &s->b_pos, &s->b_i[0], &s->b_i[1], &s->b_i[2], &s->b_long}) WQ_ALLOC(h, *b, (size_t)n * 4);
    RecCtl* ctl = s->ctl.as<RecCtl>();
    WQ_HIP(h, hipMemsetAsync(&ctl->batch_m, 0, 2 * sizeof(uint32_t), st));
    const RecRows r = rows_of(s);
    const RecBatchKeys b{{s->b_hi[0].as<uint32_t>(), s->b_hi[1].as<uint32_t>()},
                         {s->b_lo[0].as<uint64_t>(), s->b_lo[1].as<uint64_t>()}};
    uint32_t* flag = s->b_flag.as<uint32_t>();
    uint32_t* pos = s->b_pos.as<uint32_t>();
    const uint64_t seq0 = s->ops_seen;
    const dim3 grid(grid_for(n)), block(kBlock);

    hipLaunchKernelGGL(k_rec_classify, grid, block, 0, st, s->cfg, d_ops, n, b, flag, ctl);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_u32(h, flag, pos, n, false)) return rc;
    hipLaunchKernelGGL(k_rec_append, grid, block, 0, st, d_ops, n, b, flag, pos, r, s->row_cap, seq0, ctl);
    WQ_HIP(h, hipGetLastError());
    // the batch in both views' order: iota is seq order, then stable passes from the last key word up
    uint32_t* i0 = s->b_i[0].as<uint32_t>();
    uint32_t* i1 = s->b_i[1].as<uint32_t>();
    uint32_t* i2 = s->b_i[2].as<uint32_t>();
    uint32_t* s0 = s->b_sorted[0].as<uint32_t>();
    uint32_t* s1 = s->b_sorted[1].as<uint32_t>();
    hipLaunchKernelGGL(k_iota, grid, block, 0, st, i0, (uint64_t)n);
    WQ_HIP(h, hipGetLastError());
    if (int rc = sort_pass(h, s, d_ops, n, 0, 64, b, i0, i1)) return rc;
    if (int rc = sort_pass(h, s, d_ops, n, 1, 64, b, i1, i0)) return rc;
    if (int rc = sort_pass(h, s, d_ops, n, 2, 64, b, i0, i1)) return rc;
    if (int rc = sort_pass(h, s, d_ops, n, 3, 64, b, i1, i0)) return rc;
    if (int rc = sort_pass(h, s, d_ops, n, 4, 33, b, i0, s0)) return rc;
    if (int rc = sort_pass(h, s, d_ops, n, 5, 64, b, i1, i2)) return rc;
    if (int rc = sort_pass(h, s, d_ops, n, 6, 33, b, i2, s1)) return rc;
    hipLaunchKernelGGL(k_rec_map, grid, block, 0, st, s0, s1, n, pos, ctl);
    WQ_HIP(h, hipGetLastError());
    const unsigned grid_m = grid_for(s->view_ub + n);
    const int nx = s->cur ^ 1;
    hipLaunchKernelGGL(k_rec_merge<0>, dim3(grid_m), block, 0, st, r, s->view[0][s->cur].as<uint32_t>(), s0,
                       s->view[0][nx].as<uint32_t>(), s->view_cap, ctl);
    hipLaunchKernelGGL(k_rec_merge<1>, dim3(grid_m), block, 0, st, r, s->view[1][s->cur].as<uint32_t>(), s1,
                       s->view[1][nx].as<uint32_t>(), s->view_cap, ctl);
    hipLaunchKernelGGL(k_rec_commit, dim3(1), dim3(1), 0, st, ctl);
    WQ_HIP(h, hipGetLastError());
    s->cur = nx;
    s->rows_ub += n;
    s->view_ub += n;
    s->ops_seen += n;
    uint32_t* dead = s->dead.as<uint32_t>();
    const uint32_t dead_cap = dead_cap_of(s);
    hipLaunchKernelGGL(k_rec_delete, grid, block, 0, st, d_ops, n, b, r, s->view[0][nx].as<uint32_t>(), seq0, ctl, dead,
                       dead_cap, s->b_long.as<uint32_t>());
    const unsigned grid_l = std::min<unsigned>(kRecMaxBlocks, (n + kRecWaves - 1) / kRecWaves);
    hipLaunchKernelGGL(k_rec_delete_long, dim3(grid_l), block, 0, st, d_ops, b, r, s->view[0][nx].as<uint32_t>(), seq0,
                       ctl, dead, dead_cap, s->b_long.as<uint32_t>());
    WQ_HIP(h, hipGetLastError());
    s->dirty = true;  // whether a row died is known on the device only
    return WQ_OK;
}

// Rows killed since the last merge leave both views: a stable compaction into the other buffer.
int records_compact(wq_router* h, RecStore* s) {
    if (!s->dirty || s->view_ub == 0) {
        s->dirty = false;
        return WQ_OK;
    }
    const uint32_t n_ub = (uint32_t)s->view_ub;
    WQ_ALLOC(h, s->b_flag, (size_t)n_ub * 4);
    WQ_ALLOC(h, s->b_pos, (size_t)n_ub * 4);
    RecCtl* ctl = s->ctl.as<RecCtl>();
    const dim3 grid(grid_for(n_ub)), block(kBlock);
    const int nx = s->cur ^ 1;
    for (int v = 0; v < 2; ++v) {
        hipLaunchKernelGGL(k_rec_cflag, grid, block, 0, h->stream, s->view[v][s->cur].as<uint32_t>(),
                           s->live.as<uint32_t>(), n_ub, ctl, s->b_flag.as<uint32_t>());
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_u32(h, s->b_flag.as<uint32_t>(), s->b_pos.as<uint32_t>(), n_ub, false)) return rc;
        hipLaunchKernelGGL(k_rec_cscatter, grid, block, 0, h->stream, s->view[v][s->cur].as<uint32_t>(),
                           s->b_flag.as<uint32_t>(), s->b_pos.as<uint32_t>(), n_ub, s->view[v][nx].as<uint32_t>(), ctl);
        WQ_HIP(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_rec_cset, dim3(1), dim3(1), 0, h->stream, ctl);
    WQ_HIP(h, hipGetLastError());
    s->cur = nx;
    s->dirty = false;
    return WQ_OK;
}

// The read on device arrays; the call's totals arrive in s->pinned (its only host read).
int records_read_device(wq_router* h, size_t n_q, const uint32_t* d_world, const double* d_pos, const int64_t* d_after,
                        uint32_t flags, uint32_t* d_offsets, uint32_t* d_handles, int64_t* d_ts, size_t capacity,
                        wq_rec_read_result* out) {
    RecStore* s = h->rec;
    hipStream_t st = h->stream;
    const uint32_t n = (uint32_t)n_q;
    if (int rc = records_compact(h, s)) return rc;
    if (int rc = ensure_views(h, s, 1)) return rc;
    if (int rc = ensure_rows(h, s, 1)) return rc;
    WQ_ALLOC(h, s->q_lo, ((size_t)n + 1) * 4);
    WQ_ALLOC(h, s->q_len, ((size_t)n + 1) * 4);
    WQ_ALLOC(h, s->q_pre, ((size_t)n + 1) * 4);
    RecCtl* ctl = s->ctl.as<RecCtl>();
    WQ_HIP(h, hipMemsetAsync(&ctl->r_returned, 0, sizeof(RecCtl) - offsetof(RecCtl, r_returned), st));
    const RecRows r = rows_of(s);
    const uint32_t* v0 = s->view[0][s->cur].as<uint32_t>();
    const uint32_t* v1 = s->view[1][s->cur].as<uint32_t>();
    uint32_t* q_lo = s->q_lo.as<uint32_t>();
    uint32_t* q_len = s->q_len.as<uint32_t>();
    uint32_t* pre = s->q_pre.as<uint32_t>();
    const dim3 block(kBlock);

    hipLaunchKernelGGL(k_rec_range, dim3(grid_for((uint64_t)n + 1)), block, 0, st, s->cfg, d_world, d_pos, n, r, v0,
                       ctl, q_lo, q_len);
    WQ_HIP(h, hipGetLastError());
    {
        size_t bytes = 0;
        WQ_HIP(h, rocprim::exclusive_scan(nullptr, bytes, q_len, pre, 0u, (size_t)n + 1, RecSatAdd(), st));
        WQ_ALLOC(h, h->sort_tmp, bytes);
        WQ_HIP(h, rocprim::exclusive_scan(h->sort_tmp.p, bytes, q_len, pre, 0u, (size_t)n + 1, RecSatAdd(), st));
    }
    // flag / scan / emit / dedupe over the ordinals below `lim`. The granule arrays are sized on the
    // host, which does not know the ranges' total: the first walk takes rec_ordinal_guess. When the
    // total is above it, the flag pass says so, the dedupe does nothing, and the walk is run again
    // with the total the call's read-back brought (the ranges and their prefix stay as they are).
    auto walk = [&](uint32_t lim) -> int {
        const uint32_t nG = lim / kRecGranule + 1;  // + 1: the exclusive prefix's last entry is the total
        WQ_ALLOC(h, s->g_cnt, (size_t)nG * 4);
        WQ_ALLOC(h, s->g_base, (size_t)nG * 4);
        WQ_ALLOC(h, s->g_flags, (size_t)nG * 8);
        uint32_t* cnt = s->g_cnt.as<uint32_t>();
        uint32_t* base = s->g_base.as<uint32_t>();
        uint64_t* fl = s->g_flags.as<uint64_t>();
        const unsigned grid_g = std::min<unsigned>(kRecMaxBlocks, (nG + kRecWaves - 1) / kRecWaves);
        if (n) {
            hipLaunchKernelGGL(k_rec_flag, dim3(grid_g), block, 0, st, r, v0, pre, q_lo, q_len, d_after, n, lim, nG, fl,
                               cnt, ctl);
            WQ_HIP(h, hipGetLastError());
        } else {
            WQ_HIP(h, hipMemsetAsync(cnt, 0, (size_t)nG * 4, st));
        }
        if (int rc = scan_u32(h, cnt, base, nG, false)) return rc;
        const unsigned grid_e = std::min<unsigned>(kRecMaxBlocks, std::max(grid_g, grid_for((uint64_t)n + 1)));
        hipLaunchKernelGGL(k_rec_emit, dim3(grid_e), block, 0, st, r, v0, pre, q_lo, q_len, n, lim, fl, base, d_offsets,
                           d_handles, d_ts, (uint64_t)capacity, ctl);
        WQ_HIP(h, hipGetLastError());
        if (n && (flags & WQ_RECORD_READ_DEDUPE)) {
            hipLaunchKernelGGL(k_rec_dedupe, dim3(grid_g), block, 0, st, r, v0, v1, pre, q_lo, q_len, n, lim, fl, ctl,
                               s->dead.as<uint32_t>(), dead_cap_of(s));
            WQ_HIP(h, hipGetLastError());
        }
        return read_ctl(h, s);
    };
    if (int rc = walk(rec_ordinal_guess(s->view_ub, n))) return rc;
    if (s->pinned->r_cut) {
        const uint32_t total = s->pinned->r_ordinals;
        if (total > kRecMaxOrdinals)  // nothing died: the dedupe of a cut walk does nothing
            return set_error(h, WQ_E_CAPACITY, "the regions of one read call hold 2^32 - 64 rows or more: split the call");
        WQ_HIP(h, hipMemsetAsync(&ctl->r_cut, 0, sizeof(uint32_t), st));
        if (int rc = walk((total + (kRecGranule - 1)) & ~(kRecGranule - 1))) return rc;
    }
    const RecCtl& c = *s->pinned;
    s->tot_deduped += c.r_deduped;
    s->tot_rejected_queries += c.r_rejected;
    if (out) *out = wq_rec_read_result{c.r_returned, c.r_deduped, c.r_rejected, c.r_scanned, c.r_overflow, 0};
    return WQ_OK;
}

// ---- vacuum, export, import ----

// The buffers a vacuum reallocates: the row arrays, the dead list and the views.
uint64_t store_bytes(const RecStore* s) {
    uint64_t b = 0;
    for (int v = 0; v < 2; ++v) b += s->k_hi[v].bytes + s->k_lo[v].bytes + s->view[v][0].bytes + s->view[v][1].bytes;
    for (const DevBuf* d : {&s->uuid_hi, &s->uuid_lo, &s->ts, &s->seq, &s->handle, &s->live, &s->dead}) b += d->bytes;
    return b;
}

// Flag and scan over the stored rows: s->b_pos[t] is live row t's index among the live rows.
int rows_map(wq_router* h, RecStore* s, uint64_t n_rows) {
    WQ_ALLOC(h, s->b_flag, n_rows * 4);
    WQ_ALLOC(h, s->b_pos, n_rows * 4);
    hipLaunchKernelGGL(k_rec_vflag, dim3(grid_for(n_rows)), dim3(kBlock), 0, h->stream, s->live.as<uint32_t>(), n_rows,
                       s->b_flag.as<uint32_t>());
    WQ_HIP(h, hipGetLastError());
    return scan_u32(h, s->b_flag.as<uint32_t>(), s->b_pos.as<uint32_t>(), n_rows, false);
}

int records_vacuum(wq_router* h, wq_rec_vacuum_result* out) {
    RecStore* s = h->rec;
    hipStream_t st = h->stream;
    if (int rc = records_compact(h, s)) return rc;  // both views hold live rows only
    if (int rc = read_ctl(h, s)) return rc;         // the one read: the live count sizes the new arrays
    const uint64_t S = s->pinned->n_rows, L = s->pinned->live, P = s->pinned->n_dead;
    wq_rec_vacuum_result res{S, S, store_bytes(s), store_bytes(s)};
    if (out) *out = res;
    if (S == L) return WQ_OK;  // nothing dead (an empty store too): nothing moves, nothing is allocated
    if (int rc = rows_map(h, s, S)) return rc;
    const uint64_t cap = (std::max<uint64_t>(L, 1024) + 3) & ~3ull;
    // fresh arrays, all of them before anything moves: a failed allocation leaves the store as it was
    RecStore f;
    hipError_t e = hipSuccess;
    auto get = [&](DevBuf& b, uint64_t bytes) {
        if (e == hipSuccess) e = b.ensure(bytes);
    };
    for (int v = 0; v < 2; ++v) {
        get(f.k_hi[v], cap * 4);
        get(f.k_lo[v], cap * 8);
        get(f.view[v][0], cap * 4);
        get(f.view[v][1], cap * 4);
    }
    for (DevBuf* b : {&f.uuid_hi, &f.uuid_lo, &f.ts, &f.seq}) get(*b, cap * 8);
    get(f.handle, cap * 4);
    get(f.live, cap);
    get(f.dead, (cap + P) * 4);  // the pending entries plus one per row
    auto swap_all = [&]() {  // f's arrays <-> the store's
        for (int v = 0; v < 2; ++v) {
            std::swap(f.k_hi[v], s->k_hi[v]);
            std::swap(f.k_lo[v], s->k_lo[v]);
            std::swap(f.view[v][0], s->view[v][0]);
            std::swap(f.view[v][1], s->view[v][1]);
        }
        for (DevBuf RecStore::*m : {&RecStore::uuid_hi, &RecStore::uuid_lo, &RecStore::ts, &RecStore::seq,
                                    &RecStore::handle, &RecStore::live, &RecStore::dead})
            std::swap(f.*m, s->*m);
    };
    auto drop = [&]() {
        for (int v = 0; v < 2; ++v)
            for (DevBuf* b : {&f.k_hi[v], &f.k_lo[v], &f.view[v][0], &f.view[v][1]}) b->release();
        for (DevBuf* b : {&f.uuid_hi, &f.uuid_lo, &f.ts, &f.seq, &f.handle, &f.live, &f.dead}) b->release();
    };
    if (e != hipSuccess) {
        drop();
        return set_error(h, WQ_E_OOM, "record store vacuum", e);
    }
    const uint32_t* map = s->b_pos.as<uint32_t>();
    hipLaunchKernelGGL(k_rec_vmove, dim3(grid_for(S)), dim3(kBlock), 0, st, rows_of(s), rows_of(&f), map, S, cap);
    if (L) {
        for (int v = 0; v < 2; ++v)
            hipLaunchKernelGGL(k_rec_vremap, dim3(grid_for(L)), dim3(kBlock), 0, st, s->view[v][s->cur].as<uint32_t>(), map,
                               L, S, f.view[v][0].as<uint32_t>());
    }
    hipLaunchKernelGGL(k_rec_vset, dim3(1), dim3(1), 0, st, s->ctl.as<RecCtl>(), (uint32_t)L);
    e = hipGetLastError();
    if (e == hipSuccess && P) e = hipMemcpyAsync(f.dead.p, s->dead.p, P * 4, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {  // (the counter may already say L: the handle is in error either way)
        drop();
        return set_error(h, WQ_E_HIP, "record store vacuum", e);
    }
    swap_all();
    drop();  // the old arrays
    s->cur = 0;
    s->row_cap = s->view_cap = cap;
    s->dead_extra = P;
    s->rows_ub = s->view_ub = L;
    res.rows_after = L;
    res.bytes_after = store_bytes(s);
    if (out) *out = res;
    return WQ_OK;
}

// The live rows as wq_rec_row into d_out (device memory); the count is read first.
int records_export_device(wq_router* h, wq_rec_row* d_out, size_t capacity, size_t* n, uint64_t* ops_seen) {
    RecStore* s = h->rec;
    if (int rc = read_ctl(h, s)) return rc;
    const uint64_t S = s->pinned->n_rows, L = s->pinned->live;
    *n = (size_t)L;
    if (ops_seen) *ops_seen = s->ops_seen;
    if (L > capacity) return set_error(h, WQ_E_CAPACITY, "snapshot capacity too small (required size in *n)");
    if (!L) return WQ_OK;
    if (int rc = rows_map(h, s, S)) return rc;
    hipLaunchKernelGGL(k_rec_export, dim3(grid_for(S)), dim3(kBlock), 0, h->stream, s->cfg, rows_of(s),
                       s->b_pos.as<uint32_t>(), S, d_out, (uint64_t)capacity);
    WQ_HIP(h, hipGetLastError());
    WQ_HIP(h, hipStreamSynchronize(h->stream));
    return WQ_OK;
}

// The bulk build from a snapshot on the device: classify, scan, append, sort, check; one read-back.
int records_import_device(wq_router* h, const wq_rec_row* d_rows, size_t n_rows, uint64_t ops_seen,
                          wq_rec_import_result* out) {
    RecStore* s = h->rec;
    hipStream_t st = h->stream;
    if (out) *out = wq_rec_import_result{0, 0};
    if (int rc = read_ctl(h, s)) return rc;
    if (s->ops_seen != 0 || s->pinned->n_rows != 0)
        return set_error(h, WQ_E_INVALID, "an import needs a store that has received no op");
    if (n_rows >= 0xFFFFFFFFull) return set_error(h, WQ_E_CAPACITY, "the record store holds fewer than 2^32 - 1 rows");
    if (n_rows == 0) {
        s->ops_seen = ops_seen;
        return WQ_OK;
    }
    const uint32_t n = (uint32_t)n_rows;
    if (int rc = ensure_rows(h, s, n)) return rc;
    if (int rc = ensure_views(h, s, n)) return rc;
    for (int v = 0; v < 2; ++v) {
        WQ_ALLOC(h, s->b_hi[v], (size_t)n * 4);
        WQ_ALLOC(h, s->b_lo[v], (size_t)n * 8);
        WQ_ALLOC(h, s->b_key[v], (size_t)n * 8);
        WQ_ALLOC(h, s->b_sorted[v], (size_t)n * 4);
    }
    for (DevBuf* b : {&s->b_flag, &s->b_pos, &s->b_i[0], &s->b_i[1], &s->b_i[2]}) WQ_ALLOC(h, *b, (size_t)n * 4);
    RecCtl* ctl = s->ctl.as<RecCtl>();
    WQ_HIP(h, hipMemsetAsync(&ctl->imp_rejected, 0, 2 * sizeof(uint32_t), st));
    WQ_HIP(h, hipMemsetAsync(&ctl->batch_m, 0, 2 * sizeof(uint32_t), st));
    const RecRows r = rows_of(s);
    const RecBatchKeys b{{s->b_hi[0].as<uint32_t>(), s->b_hi[1].as<uint32_t>()},
                         {s->b_lo[0].as<uint64_t>(), s->b_lo[1].as<uint64_t>()}};
    uint32_t* flag = s->b_flag.as<uint32_t>();
    uint32_t* pos = s->b_pos.as<uint32_t>();
    const dim3 grid(grid_for(n)), block(kBlock);
    hipLaunchKernelGGL(k_rec_iclassify, grid, block, 0, st, s->cfg, d_rows, n, ops_seen, b, flag, ctl);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_u32(h, flag, pos, n, false)) return rc;
    hipLaunchKernelGGL(k_rec_iappend, grid, block, 0, st, d_rows, n, b, flag, pos, r, s->row_cap, ctl);
    WQ_HIP(h, hipGetLastError());
    // both views' order by stable passes from the last key word up; a snapshot's rows need not ascend
    // in seq, so seq is a pass too
    uint32_t* i0 = s->b_i[0].as<uint32_t>();
    uint32_t* i1 = s->b_i[1].as<uint32_t>();
    uint32_t* i2 = s->b_i[2].as<uint32_t>();
    uint32_t* s0 = s->b_sorted[0].as<uint32_t>();
    uint32_t* s1 = s->b_sorted[1].as<uint32_t>();
    hipLaunchKernelGGL(k_iota, grid, block, 0, st, i0, (uint64_t)n);
    WQ_HIP(h, hipGetLastError());
    if (int rc = sort_pass(h, s, d_rows, n, 7, 64, b, i0, i1)) return rc;
    if (int rc = sort_pass(h, s, d_rows, n, 0, 64, b, i1, i0)) return rc;
    if (int rc = sort_pass(h, s, d_rows, n, 1, 64, b, i0, i1)) return rc;
    if (int rc = sort_pass(h, s, d_rows, n, 2, 64, b, i1, i0)) return rc;
    if (int rc = sort_pass(h, s, d_rows, n, 3, 64, b, i0, i1)) return rc;
    if (int rc = sort_pass(h, s, d_rows, n, 4, 33, b, i1, s0)) return rc;
    if (int rc = sort_pass(h, s, d_rows, n, 5, 64, b, i0, i2)) return rc;
    if (int rc = sort_pass(h, s, d_rows, n, 6, 33, b, i2, s1)) return rc;
    uint32_t* v0 = s->view[0][s->cur].as<uint32_t>();
    uint32_t* v1 = s->view[1][s->cur].as<uint32_t>();
    hipLaunchKernelGGL(k_rec_iviews, grid, block, 0, st, s0, s1, n, pos, ctl, v0, v1, s->view_cap);
    hipLaunchKernelGGL(k_rec_icheck, grid, block, 0, st, r, v0, n, ctl);
    hipLaunchKernelGGL(k_rec_commit, dim3(1), dim3(1), 0, st, ctl);
    WQ_HIP(h, hipGetLastError());
    if (int rc = read_ctl(h, s)) return rc;  // the one read-back of the build
    const uint64_t imported = s->pinned->n_rows, rejected = s->pinned->imp_rejected;
    if (s->pinned->imp_dup) {
        WQ_HIP(h, hipMemsetAsync(ctl, 0, sizeof(RecCtl), st));
        WQ_HIP(h, hipStreamSynchronize(st));
        s->rows_ub = s->view_ub = 0;
        s->dirty = false;
        return set_error(h, WQ_E_INVALID, "the snapshot holds two rows with the same region, uuid, time and seq");
    }
    s->ops_seen = ops_seen;
    if (out) *out = wq_rec_import_result{imported, rejected};
    return WQ_OK;
}

int records_check(wq_router* h) {
    if (!h) return WQ_E_INVALID;
    if (!h->rec) return set_error(h, WQ_E_INVALID, "no record store is open (wq_records_open)");
    return WQ_OK;
}

}  // namespace

void records_release(wq_router* h) {
    RecStore* s = h->rec;
    if (!s) return;
    for (int v = 0; v < 2; ++v)
        for (DevBuf* b : {&s->k_hi[v], &s->k_lo[v], &s->view[v][0], &s->view[v][1], &s->b_hi[v], &s->b_lo[v],
                          &s->b_key[v], &s->b_sorted[v]})
            b->release();
    for (DevBuf* b : {&s->uuid_hi, &s->uuid_lo, &s->ts, &s->seq, &s->handle, &s->live, &s->dead, &s->ctl, &s->b_flag,
                      &s->b_pos, &s->b_i[0], &s->b_i[1], &s->b_i[2], &s->b_long, &s->q_lo, &s->q_len, &s->q_pre,
                      &s->g_cnt, &s->g_base, &s->g_flags, &s->in, &s->out})
        b->release();
    if (s->pinned) (void)hipHostFree(s->pinned);
    delete s;
    h->rec = nullptr;
}

// The open store's configuration, for the record dispatch's packability test; false without a store.
bool records_config(const wq_router* h, RecCfg* cfg) {
    if (!h->rec) return false;
    *cfg = h->rec->cfg;
    return true;
}

}  // namespace wq

using namespace wq;

extern "C" {

int wq_records_open(wq_router* h, uint16_t rx, uint16_t ry, uint16_t rz, uint32_t table_size) {
    if (!h) return WQ_E_INVALID;
    if (h->multi) return set_error(h, WQ_E_INVALID, "a multi-GPU handle has no record store");
    if (h->rec) return set_error(h, WQ_E_INVALID, "the record store is already open");
    if (!rx || !ry || !rz || !table_size || table_size % rx || table_size % ry || table_size % rz)
        return set_error(h, WQ_E_INVALID, "region sizes must be >= 1 and divide the table size");
    WQ_HIP(h, hipSetDevice(h->device));
    RecStore* s = new (std::nothrow) RecStore();
    if (!s) return set_error(h, WQ_E_OOM, "record store");
    s->cfg = RecCfg{{rx, ry, rz}, table_size};
    h->rec = s;
    hipError_t e = s->ctl.ensure(sizeof(RecCtl));
    if (e == hipSuccess) e = hipMemsetAsync(s->ctl.p, 0, sizeof(RecCtl), h->stream);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&s->pinned), sizeof(RecCtl), hipHostMallocDefault);
    if (e != hipSuccess) {
        records_release(h);
        return set_error(h, WQ_E_HIP, "record store open", e);
    }
    return WQ_OK;
}

int wq_records_close(wq_router* h) {
    if (int rc = records_check(h)) return rc;
    WQ_HIP(h, hipSetDevice(h->device));
    WQ_HIP(h, hipStreamSynchronize(h->stream));
    records_release(h);
    return WQ_OK;
}

int wq_records_apply_device(wq_router* h, const wq_rec_op* d_ops, size_t n) {
    if (int rc = records_check(h)) return rc;
    if (n && !d_ops) return set_error(h, WQ_E_INVALID, "null op array");
    WQ_HIP(h, hipSetDevice(h->device));
    return records_apply_device(h, d_ops, n);
}

int wq_records_apply(wq_router* h, const wq_rec_op* ops, size_t n, wq_rec_apply_result* out) {
    if (int rc = records_check(h)) return rc;
    if (n && !ops) return set_error(h, WQ_E_INVALID, "null op array");
    WQ_HIP(h, hipSetDevice(h->device));
    RecStore* s = h->rec;
    // the device counts since the store was opened: this call's share is what it adds to them
    if (int rc = read_ctl(h, s)) return rc;
    const RecCtl before = *s->pinned;
    if (n) {
        WQ_ALLOC(h, s->in, n * sizeof(wq_rec_op));
        WQ_HIP(h, hipMemcpyAsync(s->in.p, ops, n * sizeof(wq_rec_op), hipMemcpyHostToDevice, h->stream));
        if (int rc = records_apply_device(h, s->in.as<wq_rec_op>(), n)) return rc;
        if (int rc = read_ctl(h, s)) return rc;
    }
    const RecCtl& c = *s->pinned;
    if (out)
        *out = wq_rec_apply_result{c.created - before.created, c.deleted_rows - before.deleted_rows,
                                   c.rejected - before.rejected, c.live};
    return WQ_OK;
}

int wq_records_read_device(wq_router* h, size_t n, const uint32_t* d_world, const double* d_pos,
                           const int64_t* d_after_us, uint32_t flags, uint32_t* d_offsets, uint32_t* d_handles,
                           int64_t* d_ts_us, size_t capacity, wq_rec_read_result* out) {
    if (int rc = records_check(h)) return rc;
    if (!d_offsets || (n && (!d_world || !d_pos)) || (capacity && (!d_handles || !d_ts_us)))
        return set_error(h, WQ_E_INVALID, "null array");
    if (n >= 0xFFFFFFFFull) return set_error(h, WQ_E_INVALID, "a read call holds fewer than 2^32 - 1 queries");
    WQ_HIP(h, hipSetDevice(h->device));
    return records_read_device(h, n, d_world, d_pos, d_after_us, flags, d_offsets, d_handles, d_ts_us, capacity, out);
}

int wq_records_read(wq_router* h, size_t n, const uint32_t* world, const double* pos, const int64_t* after_us,
                    uint32_t flags, uint32_t* offsets, uint32_t* handles, int64_t* ts_us, size_t capacity,
                    wq_rec_read_result* out) {
    if (int rc = records_check(h)) return rc;
    if (!offsets || (n && (!world || !pos)) || (capacity && (!handles || !ts_us)))
        return set_error(h, WQ_E_INVALID, "null array");
    if (n >= 0xFFFFFFFFull) return set_error(h, WQ_E_INVALID, "a read call holds fewer than 2^32 - 1 queries");
    WQ_HIP(h, hipSetDevice(h->device));
    RecStore* s = h->rec;
    hipStream_t st = h->stream;
    auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t o_pos = 0, o_after = up(n * 24), o_world = o_after + up(n * 8);
    WQ_ALLOC(h, s->in, o_world + up(n * 4) + 256);
    const size_t o_ts = 0, o_off = up(capacity * 8), o_h = o_off + up((n + 1) * 4);
    WQ_ALLOC(h, s->out, o_h + up(capacity * 4) + 256);
    char* in = s->in.as<char>();
    char* ob = s->out.as<char>();
    if (n) {
        WQ_HIP(h, hipMemcpyAsync(in + o_pos, pos, n * 24, hipMemcpyHostToDevice, st));
        WQ_HIP(h, hipMemcpyAsync(in + o_world, world, n * 4, hipMemcpyHostToDevice, st));
        if (after_us) WQ_HIP(h, hipMemcpyAsync(in + o_after, after_us, n * 8, hipMemcpyHostToDevice, st));
    }
    wq_rec_read_result res{};
    int rc = records_read_device(h, n, reinterpret_cast<const uint32_t*>(in + o_world),
                                 reinterpret_cast<const double*>(in + o_pos),
                                 after_us ? reinterpret_cast<const int64_t*>(in + o_after) : nullptr, flags,
                                 reinterpret_cast<uint32_t*>(ob + o_off), reinterpret_cast<uint32_t*>(ob + o_h),
                                 reinterpret_cast<int64_t*>(ob + o_ts), capacity, &res);
    if (rc) return rc;
    const size_t k = (size_t)std::min<uint64_t>(res.returned, capacity);
    WQ_HIP(h, hipMemcpyAsync(offsets, ob + o_off, (n + 1) * 4, hipMemcpyDeviceToHost, st));
    if (k) {
        WQ_HIP(h, hipMemcpyAsync(handles, ob + o_h, k * 4, hipMemcpyDeviceToHost, st));
        WQ_HIP(h, hipMemcpyAsync(ts_us, ob + o_ts, k * 8, hipMemcpyDeviceToHost, st));
    }
    WQ_HIP(h, hipStreamSynchronize(st));
    if (out) *out = res;
    return WQ_OK;
}

int wq_records_drain_dead(wq_router* h, uint32_t* out, size_t capacity, size_t* n) {
    if (int rc = records_check(h)) return rc;
    if (!n || (capacity && !out)) return set_error(h, WQ_E_INVALID, "null array");
    WQ_HIP(h, hipSetDevice(h->device));
    RecStore* s = h->rec;
    if (int rc = read_ctl(h, s)) return rc;
    const size_t k = s->pinned->n_dead;
    *n = k;
    if (k > capacity) return set_error(h, WQ_E_CAPACITY, "dead list capacity too small (required size in *n)");
    if (!k) return WQ_OK;
    WQ_ALLOC(h, s->b_i[0], k * 4);
    size_t bytes = 0;
    WQ_HIP(h, rocprim::radix_sort_keys(nullptr, bytes, s->dead.as<uint32_t>(), s->b_i[0].as<uint32_t>(), k, 0, 32,
                                       h->stream));
    WQ_ALLOC(h, h->sort_tmp, bytes);
    WQ_HIP(h, rocprim::radix_sort_keys(h->sort_tmp.p, bytes, s->dead.as<uint32_t>(), s->b_i[0].as<uint32_t>(), k, 0, 32,
                                       h->stream));
    WQ_HIP(h, hipMemcpyAsync(out, s->b_i[0].p, k * 4, hipMemcpyDeviceToHost, h->stream));
    WQ_HIP(h, hipMemsetAsync(&s->ctl.as<RecCtl>()->n_dead, 0, 4, h->stream));
    WQ_HIP(h, hipStreamSynchronize(h->stream));
    return WQ_OK;
}

int wq_records_stats(wq_router* h, uint64_t* rows_live, uint64_t* rows_stored, uint64_t* ops_seen) {
    if (int rc = records_check(h)) return rc;
    WQ_HIP(h, hipSetDevice(h->device));
    RecStore* s = h->rec;
    if (int rc = read_ctl(h, s)) return rc;
    if (rows_live) *rows_live = s->pinned->live;
    if (rows_stored) *rows_stored = s->pinned->n_rows;
    if (ops_seen) *ops_seen = s->ops_seen;
    return WQ_OK;
}

int wq_records_totals(wq_router* h, wq_rec_totals* out) {
    if (int rc = records_check(h)) return rc;
    if (!out) return set_error(h, WQ_E_INVALID, "null result");
    WQ_HIP(h, hipSetDevice(h->device));
    RecStore* s = h->rec;
    if (int rc = read_ctl(h, s)) return rc;
    const RecCtl& c = *s->pinned;
    *out = wq_rec_totals{c.created, c.deleted_rows, s->tot_deduped, c.rejected, s->tot_rejected_queries};
    return WQ_OK;
}

int wq_records_vacuum(wq_router* h, wq_rec_vacuum_result* out) {
    if (int rc = records_check(h)) return rc;
    WQ_HIP(h, hipSetDevice(h->device));
    return records_vacuum(h, out);
}

int wq_records_export_device(wq_router* h, wq_rec_row* d_out, size_t capacity, size_t* n, uint64_t* ops_seen) {
    if (int rc = records_check(h)) return rc;
    if (!n || (capacity && !d_out)) return set_error(h, WQ_E_INVALID, "null array");
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return set_error(h, WQ_E_INVALID, "the snapshot array is 16-byte aligned");
    WQ_HIP(h, hipSetDevice(h->device));
    return records_export_device(h, d_out, capacity, n, ops_seen);
}

int wq_records_export(wq_router* h, wq_rec_row* out, size_t capacity, size_t* n, uint64_t* ops_seen) {
    if (int rc = records_check(h)) return rc;
    if (!n || (capacity && !out)) return set_error(h, WQ_E_INVALID, "null array");
    WQ_HIP(h, hipSetDevice(h->device));
    RecStore* s = h->rec;
    if (int rc = read_ctl(h, s)) return rc;
    const size_t k = (size_t)s->pinned->live;
    if (k <= capacity) WQ_ALLOC(h, s->out, k * sizeof(wq_rec_row));  // the staging fits the rows exactly
    if (int rc = records_export_device(h, s->out.as<wq_rec_row>(), k <= capacity ? k : 0, n, ops_seen)) return rc;
    if (k) {
        WQ_HIP(h, hipMemcpyAsync(out, s->out.p, k * sizeof(wq_rec_row), hipMemcpyDeviceToHost, h->stream));
        WQ_HIP(h, hipStreamSynchronize(h->stream));
    }
    return WQ_OK;
}

int wq_records_import_device(wq_router* h, const wq_rec_row* d_rows, size_t n, uint64_t ops_seen,
                             wq_rec_import_result* out) {
    if (int rc = records_check(h)) return rc;
    if (n && !d_rows) return set_error(h, WQ_E_INVALID, "null snapshot");
    WQ_HIP(h, hipSetDevice(h->device));
    return records_import_device(h, d_rows, n, ops_seen, out);
}

int wq_records_import(wq_router* h, const wq_rec_row* rows, size_t n, uint64_t ops_seen, wq_rec_import_result* out) {
    if (int rc = records_check(h)) return rc;
    if (n && !rows) return set_error(h, WQ_E_INVALID, "null snapshot");
    if (n >= 0xFFFFFFFFull) return set_error(h, WQ_E_CAPACITY, "the record store holds fewer than 2^32 - 1 rows");
    WQ_HIP(h, hipSetDevice(h->device));
    RecStore* s = h->rec;
    if (n) {
        WQ_ALLOC(h, s->in, n * sizeof(wq_rec_row));
        WQ_HIP(h, hipMemcpyAsync(s->in.p, rows, n * sizeof(wq_rec_row), hipMemcpyHostToDevice, h->stream));
    }
    return records_import_device(h, s->in.as<wq_rec_row>(), n, ops_seen, out);
}

int wq_region_quantize(const double* coords, size_t n, uint16_t size, int64_t* out) {
    if ((n && (!coords || !out)) || !size) return WQ_E_INVALID;
    for (size_t i = 0; i < n; ++i) {
        if (coords[i] != coords[i]) return WQ_E_INVALID;
        out[i] = clamp_region_coord_dev(coords[i], size);
    }
    return WQ_OK;
}

int wq_table_quantize(const int64_t* region, size_t n, uint32_t table_size, int64_t* out) {
    if ((n && (!region || !out)) || !table_size) return WQ_E_INVALID;
    for (size_t i = 0; i < n; ++i) out[i] = clamp_table_size_dev(region[i], (int64_t)table_size);
    return WQ_OK;
}

}  // extern "C"
