// wq_table_export.hip — the subscription table as a canonical op stream (include/wq_router.h
// wq_table_export*).
//
// Cubes, not entries, are sorted; rows are emitted element-parallel:
//   1. k_exp_flag     one lane per table slot (records, then slots): 1 for a live cube that passes the
//                     world filter; an exclusive scan compacts them
//   2. k_exp_gather   per live cube its order-preserving sort words (world, key x, y, z), count and
//                     table slot
//   3. four stable radix passes over the cube ids (z, y, x, world; rocPRIM), padding cubes last
//   4. k_exp_order    count and table slot in that order; an exclusive scan gives the row bases
//   5. k_exp_emit     one lane per output row, a wave per granule of 64 rows: the granule finds its
//                     first cube with one search over the bases, each lane its own cube within the
//                     next 64 bases, reads its peer (record inline words or list) and stores one
//                     whole 40-byte row. No lane, wave or block owns a cube: a 5,000-peer list and
//                     5,000 single-peer cubes cost the same per row.
// With a peer filter step 5 runs twice: a pass that flags the rows (the wave's ballot is the
// granule's word) and counts them, a scan of the granule counts, and a pass that stores each
// granule's survivors as one run.
// Grids are sized from what the host knows (table slots, live cubes and entries of the handle's
// stats); the exact totals are read on the device and come back in the call's one read-back.
// Scratch is O(table slots) + O(rows / 64); the sorted State arrays are neither read nor built.
#include <algorithm>

#include "export_ops.hpp"
#include "table_prims.hpp"

namespace wq {
namespace {

__global__ void k_exp_flag(ExpTable t, uint32_t world, uint64_t D, uint32_t* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < D)
        flag[i] = exp_cube_count(t, i, world) ? 1u : 0u;
    else if (i == D)
        flag[i] = 0u;  // the scan's last element: pos[D] = live cubes
}

__global__ void k_exp_gather(ExpTable t, uint32_t world, uint64_t D, const uint32_t* __restrict__ flag,
                             const uint32_t* __restrict__ pos, uint32_t n_cubes, uint64_t* __restrict__ keys,
                             uint32_t* __restrict__ cnt, uint32_t* __restrict__ src) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= D || !flag[i]) return;
    const uint32_t j = pos[i];
    if (j >= n_cubes) return;  // more live cubes than the handle's stats: reported by the totals
    uint32_t w;
    int64_t k[3];
    exp_cube_key(t, i, &w, k);
    keys[j] = (uint64_t)w;
    keys[(uint64_t)n_cubes + j] = exp_ord(k[0]);
    keys[2ull * n_cubes + j] = exp_ord(k[1]);
    keys[3ull * n_cubes + j] = exp_ord(k[2]);
    cnt[j] = exp_cube_count(t, i, world);
    src[j] = (uint32_t)i;
}

// Count and table slot of the cubes in sorted order; the count array gets a final 0 for the scan.
__global__ void k_exp_order(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ cnt,
                            const uint32_t* __restrict__ src, uint32_t n_cubes, uint32_t* __restrict__ ocnt,
                            uint32_t* __restrict__ osrc) {
    const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c < n_cubes) {
        const uint32_t j = idx[c];
        ocnt[c] = cnt[j];
        osrc[c] = src[j];
    } else if (c == n_cubes) {
        ocnt[c] = 0u;
    }
}

enum { kEmitAll = 0, kEmitFlag = 1, kEmitKept = 2 };

// base[n_cubes] = every row. Granules [0, n_gran) are launched (four per block).
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_exp_emit(ExpTable t, const uint32_t* __restrict__ base,
                                                     const uint32_t* __restrict__ ocnt,
                                                     const uint32_t* __restrict__ osrc, uint32_t n_cubes,
                                                     uint32_t n_gran, ExpFilter f, uint64_t* __restrict__ gword,
                                                     uint32_t* __restrict__ gcnt, const uint32_t* __restrict__ gbase,
                                                     uint64_t* __restrict__ out, uint32_t capacity) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t g64 = (uint64_t)blockIdx.x * (kBlock / kExpGranule) + (threadIdx.x >> 6);
    if (g64 >= n_gran) return;  // wave-uniform
    const uint32_t g = (uint32_t)g64;
    const uint32_t total = base[n_cubes];
    const uint64_t row0 = (uint64_t)g * kExpGranule;
    const bool live = row0 + lane < total;
    uint64_t word = 0;
    if (MODE == kEmitKept) {
        word = gword[g];
        if (!((word >> lane) & 1ull)) return;  // (a set bit implies a live row)
    }
    uint32_t w = 0, peer = 0;
    int64_t k[3] = {0, 0, 0};
    bool keep = false;
    if (live) {
        const uint32_t row = (uint32_t)row0 + lane;
        const uint32_t c0 = exp_cube_of(base, 0, n_cubes - 1, (uint32_t)row0);  // the same for every lane
        const uint32_t c = exp_cube_in_granule(base, c0, n_cubes, row);
        const uint64_t i = osrc[c];
        peer = exp_peer(t, i, ocnt[c], row - base[c]);
        keep = MODE == kEmitAll || exp_peer_passes(f, peer);
        if (MODE != kEmitFlag && keep) exp_cube_key(t, i, &w, k);
    }
    if (MODE == kEmitFlag) {
        const uint64_t b = __ballot(keep);
        if (lane == 0) {
            gword[g] = b;
            gcnt[g] = (uint32_t)__popcll(b);
        }
        return;
    }
    if (!keep) return;
    const uint64_t idx = MODE == kEmitAll ? row0 + lane : (uint64_t)gbase[g] + __popcll(word & ((1ull << lane) - 1ull));
    if (idx < capacity) exp_write_row(out, idx, w, peer, k);
}

// {live cubes, rows, rows kept by the peer filter} for the call's one read-back.
__global__ void k_exp_totals(const uint32_t* __restrict__ pos, uint64_t D, const uint32_t* __restrict__ base,
                             uint32_t n_cubes, const uint32_t* __restrict__ gbase, uint32_t n_gran,
                             uint64_t* __restrict__ tot) {
    if (blockIdx.x || threadIdx.x) return;
    tot[0] = pos[D];
    tot[1] = base[n_cubes];
    tot[2] = gbase ? gbase[n_gran] : base[n_cubes];
}

// The merge of G canonical exports whose cubes are disjoint: row i of segment g lands at its index
// within the segment plus, for every other segment, that segment's rows of smaller cubes.
// at[0 .. n_segs]: the segments' first rows in `rows`.
__global__ void k_exp_merge(const uint64_t* __restrict__ rows, const uint32_t* __restrict__ at, uint32_t n_segs,
                            uint64_t* __restrict__ out, uint32_t capacity) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= at[n_segs]) return;
    uint32_t g = 0;
    while (i >= at[g + 1]) ++g;
    const uint64_t* me = rows + i * kExpRowWords;
    uint64_t rank = i - at[g];
    for (uint32_t o = 0; o < n_segs; ++o) {
        if (o == g) continue;
        uint32_t lo = at[o], hi = at[o + 1];
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (exp_row_cube_less(rows + (uint64_t)mid * kExpRowWords, me))
                lo = mid + 1;
            else
                hi = mid;
        }
        rank += lo - at[o];
    }
    if (rank < capacity) {
        uint64_t* o = out + rank * kExpRowWords;
#pragma unroll
        for (uint32_t q = 0; q < kExpRowWords; ++q) o[q] = me[q];
    }
}

template <int MODE>
void launch_emit(wq_router* h, const ExpTable& t, uint32_t n_cubes, uint32_t n_gran, const ExpFilter& f,
                 uint64_t* out, uint32_t capacity) {
    ExportWs& x = h->exp;
    const unsigned grid = (unsigned)(((uint64_t)n_gran + 3) / 4);
    hipLaunchKernelGGL(k_exp_emit<MODE>, dim3(grid), dim3(kBlock), 0, h->stream, t, x.base.as<uint32_t>(),
                       x.ocnt.as<uint32_t>(), x.osrc.as<uint32_t>(), n_cubes, n_gran, f, x.gword.as<uint64_t>(),
                       x.gcnt.as<uint32_t>(), x.gbase.as<uint32_t>(), out, capacity);
}

// One handle's table to device memory on its device (the handle's device is current). *n = rows.
int export_one(wq_router* h, const wq_export_filter* f, wq_op* d_out, size_t capacity, size_t* n) {
    *n = 0;
    int rc = table_sync_delta_stats(h);  // folds the pending batch in (table_resolve(h, true))
    if (rc) return rc;
    const bool by_peer = f && f->peers;
    if (by_peer && f->n_peers == 0) return WQ_OK;
    Table& tb = h->tab;
    ExportWs& x = h->exp;
    hipStream_t s = h->stream;
    const uint64_t D = tb.rec_cap + tb.cap;
    const uint64_t rows_max = h->st.n;  // the table keeps its entries below 2^32 - 1
    if (!D || !rows_max || !tb.n_cubes) return WQ_OK;
    if (D >= 0xFFFFFFFFull || rows_max >= 0xFFFFFFFFull) return set_error(h, WQ_E_INVALID, "table too large to export");
    const uint32_t C = (uint32_t)std::min<uint64_t>(tb.n_cubes, D);
    const uint32_t n_gran = (uint32_t)((rows_max + kExpGranule - 1) / kExpGranule);
    const uint32_t cap32 = (uint32_t)std::min<uint64_t>(capacity, 0xFFFFFFFFull);
    const ExpTable t{tb.recs.as<Record>(), tb.rec_cap, tb.slots.as<Slot>(), tb.cap, tb.list.as<uint32_t>(),
                     (int64_t)h->cube_size};
    ExpFilter flt{f ? f->world : kWorldEmpty, 0u, nullptr};

    std::vector<uint32_t> bits;  // read by an asynchronous copy: lives until the read-back below
    if (by_peer) {
        uint32_t top = 0;
        for (uint32_t i = 0; i < f->n_peers; ++i) top = std::max(top, f->peers[i]);
        const uint64_t words = (uint64_t)top / 32 + 1;
        bits.assign(words, 0u);
        for (uint32_t i = 0; i < f->n_peers; ++i) bits[f->peers[i] >> 5] |= 1u << (f->peers[i] & 31u);
        WQ_ALLOC(h, x.bits, words * 4);
        WQ_HIP(h, hipMemcpyAsync(x.bits.p, bits.data(), words * 4, hipMemcpyHostToDevice, s));
        flt.bits = x.bits.as<uint32_t>();
        flt.n_bits = (uint32_t)std::min<uint64_t>(words * 32, 0xFFFFFFFFull);
    }

    WQ_ALLOC(h, x.flag, (D + 1) * 4);
    WQ_ALLOC(h, x.pos, (D + 1) * 4);
    WQ_ALLOC(h, x.keys, 4ull * C * 8);
    WQ_ALLOC(h, x.cnt, (uint64_t)C * 4);
    WQ_ALLOC(h, x.src, (uint64_t)C * 4);
    WQ_ALLOC(h, x.ocnt, ((uint64_t)C + 1) * 4);
    WQ_ALLOC(h, x.osrc, (uint64_t)C * 4);
    WQ_ALLOC(h, x.base, ((uint64_t)C + 1) * 4);
    WQ_ALLOC(h, x.tot, 32);
    WQ_ALLOC(h, h->key64_a, (uint64_t)C * 8);
    WQ_ALLOC(h, h->key64_b, (uint64_t)C * 8);
    WQ_ALLOC(h, h->idx_a, (uint64_t)C * 4);
    WQ_ALLOC(h, h->idx_b, (uint64_t)C * 4);
    if (!x.pinned) WQ_HIP(h, hipHostMalloc(&x.pinned, 32, hipHostMallocDefault));

    // 1-2: the live cubes. Cubes the world filter leaves unused pad the arrays: world all ones (no
    // real world id), so the last radix pass puts them behind every real cube, with no row.
    hipLaunchKernelGGL(k_exp_flag, dim3(grid_for(D + 1)), dim3(kBlock), 0, s, t, flt.world, D, x.flag.as<uint32_t>());
    WQ_HIP(h, hipGetLastError());
    if ((rc = scan_u32(h, x.flag.as<uint32_t>(), x.pos.as<uint32_t>(), D + 1, false))) return rc;
    WQ_HIP(h, hipMemsetAsync(x.keys.p, 0xFF, 4ull * C * 8, s));
    WQ_HIP(h, hipMemsetAsync(x.cnt.p, 0, (uint64_t)C * 4, s));
    WQ_HIP(h, hipMemsetAsync(x.src.p, 0, (uint64_t)C * 4, s));
    hipLaunchKernelGGL(k_exp_gather, dim3(grid_for(D)), dim3(kBlock), 0, s, t, flt.world, D, x.flag.as<uint32_t>(),
                       x.pos.as<uint32_t>(), C, x.keys.as<uint64_t>(), x.cnt.as<uint32_t>(), x.src.as<uint32_t>());
    // 3: least significant word first; every pass is stable
    uint32_t *ia = h->idx_a.as<uint32_t>(), *ib = h->idx_b.as<uint32_t>();
    hipLaunchKernelGGL(k_iota, dim3(grid_for(C)), dim3(kBlock), 0, s, ia, (uint64_t)C);
    for (int word = 3; word >= 0; --word) {
        hipLaunchKernelGGL(k_gather<uint64_t>, dim3(grid_for(C)), dim3(kBlock), 0, s,
                           x.keys.as<uint64_t>() + (uint64_t)word * C, ia, h->key64_a.as<uint64_t>(), (uint64_t)C);
        WQ_HIP(h, hipGetLastError());
        if ((rc = sort_pairs<uint64_t>(h, h->key64_a.as<uint64_t>(), h->key64_b.as<uint64_t>(), ia, ib, C,
                                       word ? 64 : 32)))
            return rc;
        std::swap(ia, ib);
    }
    // 4: counts in canonical order, their prefix
    hipLaunchKernelGGL(k_exp_order, dim3(grid_for((uint64_t)C + 1)), dim3(kBlock), 0, s, ia, x.cnt.as<uint32_t>(),
                       x.src.as<uint32_t>(), C, x.ocnt.as<uint32_t>(), x.osrc.as<uint32_t>());
    WQ_HIP(h, hipGetLastError());
    if ((rc = scan_u32(h, x.ocnt.as<uint32_t>(), x.base.as<uint32_t>(), (uint64_t)C + 1, false))) return rc;
    // 5: the rows
    uint64_t* out = reinterpret_cast<uint64_t*>(d_out);
    if (!by_peer) {
        const uint32_t gr = (uint32_t)((std::min<uint64_t>(cap32, rows_max) + kExpGranule - 1) / kExpGranule);
        if (gr) launch_emit<kEmitAll>(h, t, C, gr, flt, out, cap32);
    } else {
        WQ_ALLOC(h, x.gword, (uint64_t)n_gran * 8);
        WQ_ALLOC(h, x.gcnt, ((uint64_t)n_gran + 1) * 4);
        WQ_ALLOC(h, x.gbase, ((uint64_t)n_gran + 1) * 4);
        WQ_HIP(h, hipMemsetAsync(x.gcnt.as<uint32_t>() + n_gran, 0, 4, s));
        launch_emit<kEmitFlag>(h, t, C, n_gran, flt, out, cap32);
        WQ_HIP(h, hipGetLastError());
        if ((rc = scan_u32(h, x.gcnt.as<uint32_t>(), x.gbase.as<uint32_t>(), (uint64_t)n_gran + 1, false))) return rc;
        if (cap32) launch_emit<kEmitKept>(h, t, C, n_gran, flt, out, cap32);
    }
    hipLaunchKernelGGL(k_exp_totals, dim3(1), dim3(64), 0, s, x.pos.as<uint32_t>(), D, x.base.as<uint32_t>(), C,
                       by_peer ? x.gbase.as<uint32_t>() : nullptr, n_gran, x.tot.as<uint64_t>());
    WQ_HIP(h, hipGetLastError());
    // the call's one read-back
    uint64_t* tot = static_cast<uint64_t*>(x.pinned);
    WQ_HIP(h, hipMemcpyAsync(tot, x.tot.p, 24, hipMemcpyDeviceToHost, s));
    WQ_HIP(h, hipStreamSynchronize(s));
    if (tot[0] > C || tot[1] > rows_max)
        return set_error(h, WQ_E_HIP, "export: the table holds more cubes or entries than its stats");
    *n = (size_t)tot[2];
    if (*n > capacity) return set_error(h, WQ_E_CAPACITY, "export capacity too small (required size in *n)");
    return WQ_OK;
}

// h->device is current; src lives on device `from`.
int copy_rows(wq_router* h, void* dst, const void* src, int from, size_t rows) {
    if (!rows) return WQ_OK;
    if (from == h->device)
        WQ_HIP(h, hipMemcpyAsync(dst, src, rows * sizeof(wq_op), hipMemcpyDeviceToDevice, h->stream));
    else
        WQ_HIP(h, hipMemcpyPeerAsync(dst, h->device, src, from, rows * sizeof(wq_op), h->stream));
    return WQ_OK;
}

// A multi-GPU handle: replica 0, or the canonical merge of the shards (their cubes are disjoint).
int export_multi(wq_router* h, const wq_export_filter* f, wq_op* d_out, size_t capacity, size_t* n) {
    wq_router** sub;
    const int* dev;
    int mode;
    const uint32_t G = multi_subs(h, &sub, &dev, &mode);
    *n = 0;
    const uint32_t used = mode == WQ_MULTI_REPLICATE ? 1u : G;
    // every shard's whole export in its own scratch, on its own device
    std::vector<size_t> cnt(used, 0);
    for (uint32_t g = 0; g < used; ++g) {
        wq_router* s = sub[g];
        WQ_HIP(h, hipSetDevice(dev[g]));
        int rc = table_sync_delta_stats(s);
        if (!rc) {
            const hipError_t e = s->exp.stage.ensure((s->st.n ? s->st.n : 1) * sizeof(wq_op));
            rc = e == hipSuccess ? export_one(s, f, s->exp.stage.as<wq_op>(), s->st.n, &cnt[g])
                                 : set_error(s, WQ_E_OOM, "hipMalloc export staging", e);
        }
        (void)hipSetDevice(h->device);
        if (rc) {
            h->err = "device " + std::to_string(g) + ": " + s->err;
            return rc;
        }
    }
    size_t total = 0;
    for (size_t c : cnt) total += c;
    if (total >= 0xFFFFFFFFull) return set_error(h, WQ_E_INVALID, "table too large to export");
    *n = total;
    const uint32_t cap32 = (uint32_t)std::min<uint64_t>(capacity, 0xFFFFFFFFull);
    std::vector<uint32_t> at;
    uint32_t holders = 0, only = 0;
    for (uint32_t g = 0; g < used; ++g)
        if (cnt[g]) {
            ++holders;
            only = g;
        }
    if (holders == 1) {
        if (int rc = copy_rows(h, d_out, sub[only]->exp.stage.p, dev[only], std::min<size_t>(total, cap32))) return rc;
    } else if (holders > 1 && cap32) {
        WQ_ALLOC(h, h->exp.merge, total * sizeof(wq_op));
        WQ_ALLOC(h, h->exp.base, ((uint64_t)used + 1) * 4);
        at.assign(used + 1, 0u);
        for (uint32_t g = 0; g < used; ++g) {
            if (int rc = copy_rows(h, h->exp.merge.as<wq_op>() + at[g], sub[g]->exp.stage.p, dev[g], cnt[g])) return rc;
            at[g + 1] = at[g] + (uint32_t)cnt[g];
        }
        WQ_HIP(h, hipMemcpyAsync(h->exp.base.p, at.data(), ((size_t)used + 1) * 4, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_exp_merge, dim3(grid_for(total)), dim3(kBlock), 0, h->stream,
                           h->exp.merge.as<uint64_t>(), h->exp.base.as<uint32_t>(), used,
                           reinterpret_cast<uint64_t*>(d_out), cap32);
        WQ_HIP(h, hipGetLastError());
    }
    WQ_HIP(h, hipStreamSynchronize(h->stream));  // (`at` is read by a copy until here)
    if (total > capacity) return set_error(h, WQ_E_CAPACITY, "export capacity too small (required size in *n)");
    return WQ_OK;
}

int export_any(wq_router* h, const wq_export_filter* f, wq_op* d_out, size_t capacity, size_t* n) {
    return h->multi ? export_multi(h, f, d_out, capacity, n) : export_one(h, f, d_out, capacity, n);
}

}  // namespace

void export_release(wq_router* h) {
    ExportWs& x = h->exp;
    for (DevBuf* b : {&x.flag, &x.pos, &x.keys, &x.cnt, &x.src, &x.ocnt, &x.osrc, &x.base, &x.gword, &x.gcnt, &x.gbase,
                      &x.bits, &x.tot, &x.stage, &x.merge})
        b->release();
    if (x.pinned) (void)hipHostFree(x.pinned);
    x.pinned = nullptr;
}

}  // namespace wq

using namespace wq;

extern "C" {

int wq_table_export_device(wq_router* h, const wq_export_filter* f, wq_op* d_out, size_t capacity, size_t* n) {
    if (!h || !n || (capacity && !d_out)) return WQ_E_INVALID;
    WQ_HIP(h, hipSetDevice(h->device));
    return export_any(h, f, d_out, capacity, n);
}

int wq_table_export(wq_router* h, const wq_export_filter* f, wq_op* out, size_t capacity, size_t* n) {
    if (!h || !n || (capacity && !out)) return WQ_E_INVALID;
    WQ_HIP(h, hipSetDevice(h->device));
    // the rows' device image: never more than the table's entries
    uint64_t bound = 0;
    if (h->multi) {
        wq_stats st;
        if (int rc = wq_get_stats(h, &st)) return rc;
        bound = st.n_entries;
    } else {
        if (int rc = table_sync_delta_stats(h)) return rc;
        bound = h->st.n;
    }
    const size_t room = (size_t)std::min<uint64_t>(capacity, bound);
    DevBuf& img = h->exp.stage;  // (a multi-GPU handle's sub-handles stage in their own)
    WQ_ALLOC(h, img, (room ? room : 1) * sizeof(wq_op));
    const int rc = export_any(h, f, img.as<wq_op>(), room, n);
    if (rc != WQ_OK && rc != WQ_E_CAPACITY) return rc;
    const size_t got = std::min<size_t>(*n, room);
    if (got) {
        WQ_HIP(h, hipMemcpyAsync(out, img.p, got * sizeof(wq_op), hipMemcpyDeviceToHost, h->stream));
        WQ_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (*n > capacity) return set_error(h, WQ_E_CAPACITY, "export capacity too small (required size in *n)");
    return WQ_OK;
}

}  // extern "C"
