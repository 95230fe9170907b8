// wq_sharded_slots.hip — the sharded ticks on compact slots: the slot tick (the default form of
// wq_sharded_route_tick_device and wq_sharded_route_tick_async) and the owner form on slots
// (wq_sharded_route_owner_slots[_async]). Both are built on one scaffold — a per-tick frame, the
// budgeted slot exchange X1, and the synchronous and asynchronous ends — so the invariants they
// share are kept in one place each:
//   * every rank makes the same exchanges on every path, after a local failure too (Late);
//   * host memory an asynchronous copy reads outlives the copy (TickFrame::st_host);
//   * every shard queues the same ticks in the snapshot ring (finish_async, async_drain).
// The exchanges themselves are wq_shard_exchange.hip's.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "route_count.hpp"
#include "route_emit.hpp"
#include "route_gather.hpp"
#include "route_radius.hpp"
#include "route_scan.hpp"
#include "shard_ctx.hpp"

// (asynchronous tick) the end-of-tick snapshot kernel, when the tile scan could not take it
// (route_async.hpp async_result_block: a scan over more tiles than one block takes, or no scan).
// It keeps the unmangled name profiles and traces know it by.
extern "C" __global__ __launch_bounds__(256) void k_async_result(wq::AsyncResultParams p) { wq::async_result_block(p); }

namespace wq {
namespace {

// ---------------------------------------------------------------------------------------------
// kernels of the slot tick: compact slots to the owners, row references and cube-list pools back
// ---------------------------------------------------------------------------------------------
// What an owner returns per received slot (12 bytes, uint3 {x, y, z}): the message's recipients as
// a row of words — z = kind << 30 | skipped index (kRefSkipNone: none), y = the row's source length
// (OnlySelf: the recipient count, 0 or 1), x = where the source is:
//   POOL    word offset in the pool the owner ships to this source (remote owners only): each cube
//           a source's messages hit is shipped to it ONCE per tick, whatever the number of messages
//   LIST    the cube's list in this handle's table (an owner's own messages: nothing is copied)
//   INLINE  the record slot whose inline peers are the row (ditto)
//   SELF    the sender itself (OnlySelf, when subscribed), or an empty row
// The ingesting GPU turns every reference into a {len, skip, pointer} descriptor in message order
// and gathers the CSR with gather_rows_kernel (route_gather.hpp).
constexpr uint32_t kRefPool = 0, kRefList = 1, kRefInline = 2, kRefSelf = 3;
constexpr uint32_t kRefSkipNone = 0x3FFFFFFFu;
constexpr int kRefClaimTagBits = 26;  // claim words: tag << 38 | source << 32 | cube locator

// Largest s < G with sb.b[s] <= i (segments may be empty).
__device__ __forceinline__ uint32_t seg_find(const SegBounds& sb, uint32_t G, uint32_t i) {
    uint32_t lo = 0, hi = G;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sb.b[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct RefOwnerParams {
    const uint32_t* e;     // count pass: filtered recipients per received slot (remote slots)
    const uint2* info;     // count pass: locator per received slot (route_count.hpp finish_message)
    const uint32_t* list;
    const Record* recs;
    SegBounds rrem;        // the remote slots per source shard, in remote index (own segment empty)
    uint32_t G, n_rem;     // remote slots
    uint32_t self_lo, n_self;  // the own segment of the received slots (skipped)
    uint32_t tag;
    unsigned long long* claim;  // (cube, source) claims of this tick, open addressing
    uint32_t* lead;             // claim slot -> the remote slot that claimed it
    uint64_t cmask;
    uint32_t* cnt;         // per remote slot: the cube's peer count (OnlySelf: e)
    uint32_t* hslot;       // per remote slot: its claim slot
    uint32_t* plen;        // per remote slot: words it adds to its source's pool (n_rem + 1 entries)
    const uint32_t* poff;  // exclusive scan of plen
    uint3* ref_send;       // per remote slot: its reference
    uint4* desc_fill;      // pool rows: the claiming slot copies its cube's peers
};

__device__ __forceinline__ uint32_t slot_cnt(const uint2 inf, uint32_t e) {
    if (inf.x & kLocSelf) return e;
    // a list row: e is the count less the sender's entry when the row skips it (finish_message),
    // so no read of the list's count word is needed
    if (inf.x & kLocGlobal) return e + (inf.y != kNone ? 1u : 0u);
    return inf.y == kNone ? 0u : inf.y >> 24;  // inline record, or no subscriber at all
}

// (owner, remote slots) the cube's peer count and the claim of the slot's (source, cube) pair: the
// first claimer ships the cube's peers in that source's pool, the others point at them. The block's
// slots first meet in an LDS table, so each distinct pair of the block claims once in global memory:
// C3's hot cubes put thousands of a source's slots on one claim word, and device-scope atomics on
// one word serialise.
constexpr uint32_t kClaimLds = 2 * kBlock;  // LDS table slots (a block has at most kBlock keys)
constexpr unsigned long long kClaimEmpty = ~0ull;

__global__ __launch_bounds__(kBlock) void k_ref_claim(RefOwnerParams p) {
    __shared__ unsigned long long lkey[kClaimLds];
    __shared__ uint32_t lres[kClaimLds];  // the pair's claim slot | leader bit 31 (set by its representative)
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    for (uint32_t k = threadIdx.x; k < kClaimLds; k += kBlock) lkey[k] = kClaimEmpty;
    if (t == p.n_rem) p.plen[t] = 0;
    const bool live = t < p.n_rem;
    const uint32_t i = t < p.self_lo ? t : t + p.n_self;  // the received slot
    uint2 inf = make_uint2(kLocSelf, kNone);
    uint32_t cnt = 0, s = 0;
    if (live) {
        s = seg_find(p.rrem, p.G, t);
        inf = p.info[i];
        cnt = slot_cnt(inf, p.e[i]);
    }
    const bool claims = live && !(inf.x & kLocSelf) && cnt;
    const unsigned long long pair = ((unsigned long long)s << 32) | inf.x;  // s < G: never kClaimEmpty
    __syncthreads();
    // the block's table: the thread that inserts a pair represents it
    bool rep = false;
    uint32_t lh = 0;
    if (claims) {
        uint64_t hv = pair * 0x9E3779B97F4A7C15ull;
        lh = (uint32_t)(hv >> 40) & (kClaimLds - 1);
        for (;;) {
            const unsigned long long old = atomicCAS(&lkey[lh], kClaimEmpty, pair);
            if (old == kClaimEmpty) {
                rep = true;
                break;
            }
            if (old == pair) break;
            lh = (lh + 1) & (kClaimLds - 1);
        }
    }
    uint64_t hs = 0;
    if (rep) {
        const unsigned long long key = ((unsigned long long)p.tag << 38) | pair;
        uint64_t hv = ((uint64_t)inf.x | ((uint64_t)s << 32)) * 0x9E3779B97F4A7C15ull;
        hv ^= hv >> 29;
        hs = hv & p.cmask;
        bool leader = false;
        for (;;) {
            unsigned long long v = __hip_atomic_load(p.claim + hs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((v >> 38) != p.tag) {  // a previous tick's word: free
                const unsigned long long old = atomicCAS(p.claim + hs, v, key);
                if (old == v) {
                    leader = true;
                    break;
                }
                v = old;
            }
            if (v == key) break;
            if ((v >> 38) == p.tag) hs = (hs + 1) & p.cmask;
        }
        if (leader) p.lead[hs] = t;
        lres[lh] = (uint32_t)hs | (leader ? 0x80000000u : 0u);
    }
    __syncthreads();
    if (!live) return;
    bool leader = false;
    if (claims) {
        const uint32_t r = lres[lh];
        hs = r & 0x7FFFFFFFu;
        leader = rep && (r >> 31);
    }
    p.cnt[t] = cnt;
    p.hslot[t] = (uint32_t)hs;
    p.plen[t] = leader ? cnt : 0u;
}

// The row of a slot from its count-pass locator: kind, source offset (list word / record slot) and
// skipped index (local_message.rs:60-86 as finish_message encoded it).
__device__ __forceinline__ void slot_row(const uint2 inf, uint32_t* kind, uint32_t* off, uint32_t* skip) {
    *kind = kRefSelf;
    *off = 0;
    *skip = kRefSkipNone;
    if (inf.x & kLocSelf) return;
    if (inf.x & kLocGlobal) {
        *kind = kRefList;
        *off = (inf.x & ~kLocGlobal) + 1;
        *skip = inf.y == kNone ? kRefSkipNone : inf.y;
    } else if (inf.y != kNone) {
        *kind = kRefInline;
        *off = inf.x;
        const uint32_t s24 = inf.y & kSkipNone24;
        *skip = s24 == kSkipNone24 ? kRefSkipNone : s24;
    }  // else: no subscriber — an empty SELF row
}

__device__ __forceinline__ const uint32_t* row_src(uint32_t kind, uint32_t off, const uint32_t* list, const Record* recs) {
    return kind == kRefList ? list + off : reinterpret_cast<const uint32_t*>(recs) + ((uint64_t)off * 32 + kInlineWord0);
}

// (owner, remote slots) a remote source's slot becomes its reference into the source's pool and,
// for the claiming slot, the pool row copying its cube's peers.
__global__ __launch_bounds__(kBlock) void k_ref_make(RefOwnerParams p) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= p.n_rem) return;
    const uint32_t i = t < p.self_lo ? t : t + p.n_self;  // the received slot
    const uint32_t s = seg_find(p.rrem, p.G, t);
    uint32_t kind, off, skip;
    slot_row(p.info[i], &kind, &off, &skip);
    const uint32_t cnt = p.cnt[t];
    uint3 ref;
    if (kind == kRefList || kind == kRefInline) {
        const uint32_t j = p.lead[p.hslot[t]];
        ref = make_uint3(p.poff[j] - p.poff[p.rrem.b[s]], cnt, (kRefPool << 30) | skip);
        if (j == t) {
            const uint64_t a = reinterpret_cast<uint64_t>(row_src(kind, off, p.list, p.recs));
            p.desc_fill[t] = make_uint4(cnt, kNone, (uint32_t)a, (uint32_t)(a >> 32));
        }
    } else {
        ref = make_uint3(0, cnt, (kRefSelf << 30) | kRefSkipNone);
    }
    p.ref_send[t] = ref;
}

// (owner) the C vector of the pool-size exchange, per source d: {pool words for d, status}. The
// status carries the owner's device error bits (8: stale table, plus its count pass's bits) and the
// budget bit when this shard knows of ANY budget that was too small — its own slot segments (A
// sent), any source's (A received: every shard receives every A vector), or its own pools here — so
// after the exchange every shard knows the same: redo the tick exactly, or not.
struct CVecParams {
    const uint32_t* a_send;  // 2G words
    const uint32_t* a_recv;  // 2G words
    const uint32_t* poff;    // nullable: no remote slots
    SegBounds rb;            // the receive layout's segments (remote slot index per source)
    uint64_t b2[WQ_MAX_SHARDS];  // pool word budgets me -> d (~0: no budget, the exact pass)
    uint32_t G;
    const uint32_t* stale;
    const wq_route_counters* cnt;  // the owner count pass's counters (nullable)
    uint32_t* c_send;        // out: 2G words
};

__global__ void k_c_vector(CVecParams p) {
    const uint32_t d = threadIdx.x;
    const bool in = d < p.G;
    uint32_t pool = 0;
    bool over = false;
    if (in) {
        pool = p.poff ? p.poff[p.rb.b[d + 1]] - p.poff[p.rb.b[d]] : 0u;
        over = (uint64_t)pool > p.b2[d] || (p.a_send[2 * d + 1] & kStBudget) || (p.a_recv[2 * d + 1] & kStBudget);
    }
    const bool any_over = __any(over);
    uint32_t bits = (p.stale && *p.stale) ? kErrStale : 0u;
    if (p.cnt) bits |= p.cnt->error;
    if (in) {
        p.c_send[2 * d] = pool;
        p.c_send[2 * d + 1] = ((bits & 0xFFFFu) << 8) | (any_over ? kStBudget : 0u);
    }
}

// (owner) per 256-slot block of the receive layout (segments are whole blocks): where its pool rows
// go in the send buffer (the source's budgeted segment) and where that segment ends.
struct PoolBlocksParams {
    const uint32_t* poff;
    SegBounds rb;
    uint64_t pb[WQ_MAX_SHARDS + 1];  // pool segment bases (words) in the send buffer
    uint32_t G, nblk;
    uint64_t* base;
    uint64_t* lim;
};

__global__ void k_pool_blocks(PoolBlocksParams p) {
    const uint32_t b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= p.nblk) return;
    const uint32_t i0 = b * kBlock;
    const uint32_t s = seg_find(p.rb, p.G, i0);
    p.base[b] = p.pb[s] + (p.poff[i0] - p.poff[p.rb.b[s]]);
    p.lim[b] = p.pb[s + 1];
}

// (ingesting GPU) the row of every slot it sent, from its owner's reference: e and the locator in
// message order (emit_map_kernel's info: a pool row as kLocPool | word offset into the received
// pools). A reference that does not lie inside its owner's pool segment — an owner that failed, or
// a tick whose budgets were too small (both reported after the tick) — routes to nobody, so no
// kernel ever reads outside the pools.
struct ResolveParams {
    const uint32_t* perm;     // sent slot -> message (kNone: tails, padding)
    const uint3* ref_recv;    // references, in the send layout
    SegBounds sb;             // the send layout's segments (slot index per owner)
    uint32_t G, n;            // n = slots in the send layout
    uint64_t prb[WQ_MAX_SHARDS + 1];  // pool segment bases (words) in the receive buffer
    uint32_t* e_msg;
    uint2* info_msg;
    // RADIUS: the pool rows are filtered here, where the message positions and every peer's position
    // are (the owner has neither the message position nor a reason to need it)
    const uint32_t* pool = nullptr;
    const double* pos = nullptr;
    const uint32_t* sender = nullptr;
    const uint8_t* repl = nullptr;
    TableView tv{};
};

// RADIUS: a pool row keeps its full length (the emit re-filters it, as count_radius_kernel's list
// rows) and e counts the candidates within the radius that replication keeps; an OnlySelf row the
// sender, if subscribed and within the radius of its own message.
template <bool RADIUS>
__global__ __launch_bounds__(kBlock) void k_ref_resolve(ResolveParams p) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= p.n) return;
    const uint32_t m = p.perm[k];
    if (m == kNone) return;
    const uint3 ref = p.ref_recv[k];
    const uint32_t kind = ref.z >> 30, sk = ref.z & kRefSkipNone;
    if (kind == kRefSelf) {  // OnlySelf: the sender when subscribed (y = 0 or 1), or an empty row
        uint32_t e = ref.y <= 1u ? ref.y : 0u;
        if (RADIUS && e) {
            const uint32_t me = p.sender[m];
            e = within_radius(p.tv, p.pos[3ull * m], p.pos[3ull * m + 1], p.pos[3ull * m + 2], me) ? 1u : 0u;
        }
        p.e_msg[m] = e;
        p.info_msg[m] = make_uint2(kLocSelf, kNone);
        return;
    }
    const uint32_t o = seg_find(p.sb, p.G, k);
    const uint64_t at = p.prb[o] + ref.x;
    const uint32_t skip = sk == kRefSkipNone ? kNone : sk;
    const bool ok = kind == kRefPool && at + ref.y <= p.prb[o + 1] && ref.y && (skip == kNone || skip < ref.y);
    if (RADIUS) {
        uint32_t e = 0, mask = 0;
        const uint32_t len = ref.y;
        if (ok) {
            const uint32_t me = p.sender[m];
            const uint8_t rp = p.repl[m];
            const double mx = p.pos[3ull * m], my = p.pos[3ull * m + 1], mz = p.pos[3ull * m + 2];
            const uint32_t* row = p.pool + at;
            for (uint32_t i = 0; i < len; ++i) {
                const uint32_t q = row[i];
                const bool keep = repl_keeps(rp, q, me) && within_radius(p.tv, mx, my, mz, q);
                e += keep ? 1u : 0u;
                if (keep && i < (uint32_t)kInline) mask |= 1u << i;
            }
        }
        p.e_msg[m] = e;
        // a short row carries its survivor mask (staged like an inline record's, kPoolShort), a long
        // one its length (re-filtered by the emit)
        p.info_msg[m] = !e ? make_uint2(0, kNone)
                       : len <= (uint32_t)kInline ? make_uint2(kLocPool | (uint32_t)at, kPoolShort | (len << 24) | mask)
                                                  : make_uint2(kLocPool | (uint32_t)at, len);
        return;
    }
    p.e_msg[m] = ok ? ref.y - (skip != kNone ? 1u : 0u) : 0u;
    p.info_msg[m] = ok ? make_uint2(kLocPool | (uint32_t)at, skip) : make_uint2(0, kNone);
}

// (ingesting GPU, G > 1, no radius) the own-cube count and the slot grouping's owner histogram in
// ONE pass over the messages (both quantise every message): block b takes the kHistTiles count
// tiles of histogram tile b (launch_budget_slots' 4 x 256 messages), counts its own cubes' messages
// as count_kernel<OWN> does, and adds every other message's slot weight (2 for an unpacked key) to
// its owner's column, hist[d * nblk + b], as slot_count_kernel would.
constexpr uint32_t kHistTiles = 4;

template <bool RAW>
__global__ __launch_bounds__(kBlock, 8) void own_count_hist_kernel(CountParams p, uint32_t nblk,
                                                                   uint32_t* __restrict__ hist) {
    __shared__ uint64_t wave_F[kWaves];
    __shared__ uint64_t wave_E[kWaves];
    __shared__ uint32_t hcnt[WQ_MAX_SHARDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t G = p.in.own_G;
    for (uint32_t d = tid; d < G; d += kBlock) hcnt[d] = 0;
    if (blockIdx.x == 0 && tid == 0) {
        p.cnt_next->n_pairs = 0;
        p.cnt_next->n_candidates = 0;
        p.cnt_next->overflow = 0;
        p.cnt_next->error = 0;
    }
    __syncthreads();
    for (uint32_t k = 0; k < kHistTiles; ++k) {
        const uint32_t blk = blockIdx.x * kHistTiles + k;  // block-uniform
        if (blk >= p.n_tiles) break;
        const uint32_t m0 = blk * kBlock, m = m0 + tid;
        uint64_t F_local = 0;
        uint32_t E_local = 0;
        uint32_t e_out[1], own[1];
        uint2 inf_out[1];
        count_rows<RAW, 1, 0, false, false, true>(p.in, p.t, m0, e_out, inf_out, F_local, E_local, nullptr, own);
        if (m < p.in.M) {
            p.e[m] = e_out[0];
            p.info[m] = inf_out[0];
        }
        // the other shards' messages, one LDS add per distinct owner in the wave
        const uint32_t ow = own[0] & 0x7FFFFFFFu;
        const bool rem = m < p.in.M && ow != p.in.own_me;
        const uint64_t wide = __ballot(rem && (own[0] >> 31));
        uint64_t todo = __ballot(rem);
        while (todo) {
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const uint32_t d = __shfl(ow, leader, 64);
            const uint64_t mask = __ballot(rem && ow == d);
            if (lane == leader) atomicAdd(&hcnt[d], (uint32_t)(__popcll(mask) + __popcll(mask & wide)));
            todo &= ~mask;
        }
        const uint64_t Fw = wave_sum_u64(F_local);
        const uint64_t Ew = wave_sum_u64(E_local);
        if (lane == 0) {
            wave_F[wave] = Fw;
            wave_E[wave] = Ew;
        }
        __syncthreads();
        if (tid == 0) {
            uint64_t Fb = 0, Eb = 0;
#pragma unroll
            for (int u = 0; u < kWaves; ++u) {
                Fb += wave_F[u];
                Eb += wave_E[u];
            }
            p.tile_F[blk] = Fb > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)Fb;
            p.tile_total[blk] = Eb > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)Eb;
            if (Eb > 0xFFFFFFFFull) flag_route(p.cnt, p.health, 2u, 0u);
        }
        __syncthreads();  // the next tile rewrites wave_F / wave_E
    }
    for (uint32_t d = tid; d < G; d += kBlock) hist[(uint64_t)d * nblk + blockIdx.x] = hcnt[d];
}

}  // namespace

// The slot tick's CSR from its rows in message order (e_msg, info_msg; per-256-message totals in
// mtiles): the tile scan (offsets[M] = P, the counters at kCntScan: P, the overflow / error bits),
// then emit_map_kernel — rows of this shard's own cubes read the table, the others the pools
// received (outputs beyond capacity are not written).
int slots_copy_out(wq_router* h, uint32_t* d_offsets, uint32_t* d_peers, uint32_t* d_msgs, size_t capacity,
                   const AsyncResultParams* ar, bool* ar_done) {
    ShardCtx& sc = *h->shard;
    const uint64_t M = sc.last_M;
    hipStream_t s = h->stream;
    wq_route_counters* cnt = reinterpret_cast<wq_route_counters*>(sc.small.as<char>() + kSmallCnt) + kCntScan;
    if (M == 0) {
        WQ_HIP(h, hipMemsetAsync(cnt, 0, sizeof(*cnt), s));
        WQ_HIP(h, hipMemsetAsync(d_offsets, 0, 4, s));
        return WQ_OK;
    }
    const uint32_t nt = (uint32_t)((M + kBlock - 1) / kBlock);
    uint32_t* tile_total = sc.mtiles.as<uint32_t>();
    uint32_t* tile_prefix = tile_total + nt;
    TileScanParams tp;
    tp.tile_total = tile_total;
    tp.tile_F = tile_total;  // F is reported as P on this path
    tp.tile_prefix = tile_prefix;
    tp.n_tiles = nt;
    tp.offsets = d_offsets;
    tp.M = (uint32_t)M;
    tp.capacity = capacity;
    tp.cnt = cnt;
    tp.health = h->rws.buf.p ? route_health(h) : nullptr;
    tp.stale = h->tab.stale.as<uint32_t>();  // error bit 8: the table still misses a device batch
    if (ar) {  // an asynchronous tick: the scan ends it (if it is the one-block scan)
        tp.ar = *ar;
        tp.async_end = true;
    }
    if (int rc = launch_tile_scan(h, tp, ar_done)) return rc;
    EmitParams ep;
    ep.sender = sc.last_sender;
    ep.pos = sc.last_radius ? sc.last_pos : nullptr;
    ep.repl = sc.last_radius ? sc.last_repl : nullptr;
    ep.M = (uint32_t)M;
    ep.t = table_view(h);
    ep.e = sc.e_msg.as<uint32_t>();
    ep.tile_prefix = tile_prefix;
    ep.count_tile = kBlock;
    ep.offsets = d_offsets;
    ep.info = sc.info_msg.as<uint2>();
    ep.peers = capacity ? d_peers : nullptr;
    ep.msgs = d_msgs;
    ep.capacity = capacity;
    ep.n_blocks = nt;
    ep.pool = sc.G > 1 ? sc.pool_recv.as<uint32_t>() : nullptr;  // pool rows (kLocPool) only at G > 1
    if (sc.last_radius)  // the radius filter's emit: masks of inline rows, list and pool rows re-filtered
        hipLaunchKernelGGL((emit_kernel<4096, 2, true>), dim3(nt), dim3(kBlock), 0, s, ep);
    else
        hipLaunchKernelGGL((emit_map_kernel<16>), dim3(pass_blocks(nt)), dim3(kBlock), 0, s, ep);
    WQ_HIP(h, hipGetLastError());
    return WQ_OK;
}

namespace {

// ---------------------------------------------------------------------------------------------
// the scaffold of a tick on slots
// ---------------------------------------------------------------------------------------------
inline uint32_t whole_blocks(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock * kBlock); }
inline uint32_t slot_budget(uint64_t n) { return whole_blocks(n + n / 16 + kBlock); }
inline uint64_t pool_budget(uint64_t n) { return n + n / 16 + 1024; }

// The caller's messages of one tick.
struct TickIn {
    const double* pos;
    const int64_t* keys;
    const uint32_t* world;
    const uint32_t* sender;
    const uint8_t* repl;
    size_t M;
};

// X1's layout: owner d's segment of the slots sent (L, sb) and source s's of the slots received
// (rb), Sb and Rb slots in all. self_in_place / a_in_place: set by a form whose grouping wrote this
// shard's own segment (and its A entry) straight into the receive buffers.
struct SlotSegs {
    SlotLayout L{};
    SegBounds sb{}, rb{};
    uint64_t Sb = 0, Rb = 0;
    bool self_in_place = false, a_in_place = false;
};

struct TickPicture {
    uint32_t code = 0, bits = 0, code_from = 0, bits_from = 0;
    bool over = false;
};
TickPicture fold_tick(ShardCtx& sc, const char* hs, bool self_seg);

// One tick's frame, on the tick function's stack: the local failure so far, the small vectors
// carved, the host source of the status copies, and the steps both forms share. put_status copies
// asynchronously out of st_host, so the frame must live until the stream has been synchronised on
// every return path that issued one: read_back and finish_async synchronise before they report a
// local failure, and a status is only ever issued for one.
struct TickFrame {
    wq_router* const h;
    ShardCtx& sc;
    const hipStream_t s;
    const uint32_t G, me;
    const bool exact;  // the sizes are exchanged alone and read back first; else they are the budgets
    const int inject;  // wq_debug_inject_shard_failure: the step to fail (0: none)
    Late late;
    char* const small;
    uint32_t *const a_send, *const a_recv, *const c_send, *const c_recv;
    wq_route_counters* const cnts;
    const std::vector<size_t> eight;  // the A and C vectors' segments: 8 bytes per shard
    std::vector<uint32_t> st_host;
    // A, C (both directions) and the counters
    static constexpr size_t kSmallUsed = kSmallCnt + 4 * sizeof(wq_route_counters);
    static_assert(kSmallC + 16 * WQ_MAX_SHARDS <= kSmallCnt, "the C vectors lie inside the zeroed span");

    TickFrame(wq_router* h_, bool exact_, int inject_)
        : h(h_), sc(*h_->shard), s(h_->stream), G(sc.G), me(sc.rank), exact(exact_), inject(inject_),
          small(sc.small.as<char>()), a_send(reinterpret_cast<uint32_t*>(small + kSmallA)), a_recv(a_send + 2 * G),
          c_send(reinterpret_cast<uint32_t*>(small + kSmallC)), c_recv(c_send + 2 * G),
          cnts(reinterpret_cast<wq_route_counters*>(small + kSmallCnt)), eight(G, 8), st_host(2 * G, 0) {}

    // The small vectors zeroed (an asynchronous tick's last kernel zeroes them itself), the health
    // words in place, the tick counted.
    int begin() {
        if (!sc.small_zeroed) WQ_HIP(h, hipMemsetAsync(small, 0, kSmallUsed, s));
        sc.small_zeroed = false;
        RouteWs& rw = h->rws;
        if (!rw.buf.p) {  // as route_counters lays it out: health words first
            WQ_ALLOC(h, rw.buf, 128);
            WQ_HIP(h, hipMemsetAsync(rw.buf.p, 0, 128, s));
            rw.calls = 0;
        }
        if (exact) sc.n_exact++;
        else sc.n_budget++;
        return WQ_OK;
    }
    int fail(int rc) { return late.fail(h, rc); }
    int alloc(DevBuf& b, size_t bytes) {
        return b.ensure(bytes) == hipSuccess ? WQ_OK : set_error(h, WQ_E_OOM, "hipMalloc (sharded tick workspace)");
    }
    // This shard's failed step as the status of every segment of an A or C vector it sends.
    int put_status(uint32_t* dst) {
        for (uint32_t d = 0; d < G; ++d) st_host[2 * d + 1] = status_of(late.code);
        WQ_HIP(h, hipMemcpyAsync(dst, st_host.data(), 8 * G, hipMemcpyHostToDevice, s));
        return WQ_OK;
    }
    // A count pass's parameters: e / locator per message or slot of `in`, the tile sums at `tiles`
    // (candidates F_at words further on), the counters in block `slot` of the small vectors.
    CountParams count_params(const TableView& tv, const RouteIn& in, uint32_t* e, uint2* info, uint32_t* tiles,
                             uint64_t F_at, uint32_t n_tiles, size_t slot, const uint32_t* perm = nullptr) {
        CountParams cp{};
        cp.in = in;
        cp.t = tv;
        cp.e = e;
        cp.info = info;
        cp.tile_total = tiles;
        cp.tile_F = tiles + F_at;
        cp.cnt = cnts + slot;
        cp.cnt_next = cnts + kCntScratch;
        cp.health = route_health(h);
        cp.n_tiles = n_tiles;
        cp.perm = perm;
        return cp;
    }
    // ... over n compact slots (min(n, *m_dev) when m_dev is set)
    RouteIn slots_in(const uint32_t* slots, uint32_t n, const uint32_t* m_dev = nullptr) {
        RouteIn r{nullptr, nullptr, nullptr, nullptr, nullptr, n, (int64_t)h->cube_size};
        r.slots = slots;
        r.m_dev = m_dev;
        return r;
    }
    template <class Group>
    int exchange_slots(bool self_seg, SlotSegs& x, Group group);
    AsyncResultParams async_params(bool statuses, bool has_msgs, uint64_t capacity, wq_route_counters* d_result);
    int finish_async(const AsyncResultParams& ar, bool ar_done);
    int read_back(bool self_seg, bool* redo, const wq_route_counters** hcnt);
};

// X1: {A: slots + status per owner, the slots in budgeted segments}. An exact tick exchanges A alone
// first and reads it back (the budgets become the true counts in whole blocks); a budgeted tick
// sends both in one exchange. self_seg: this shard's own segment is budgeted like the others (the
// owner form) or empty (the slot tick). group(phases, L) is the form's launch_budget_slots call:
// phases 1 = the counts only, under no budget; 2 / 3 = the scatter into x.L, after / with them.
// A shard that has failed sends tail slots and its status, in the same exchanges.
template <class Group>
int TickFrame::exchange_slots(bool self_seg, SlotSegs& x, Group group) {
    int rc;
    if (exact) {  // the true counts first (A alone, read back): budgets = the counts, whole blocks
        SlotLayout inf{};
        for (uint32_t d = 0; d < G; ++d) inf.budget[d] = 0xFFFFFFFFu;
        if (!late) fail(group(1, inf));
        if (late && (rc = put_status(a_send))) return rc;
        Xfer xa{{a_send}, {eight.data()}, {a_recv}, {eight.data()}, 1};
        if ((rc = exchange(h, xa))) return rc;
        uint32_t* hv = static_cast<uint32_t*>(sc.hsmall);
        WQ_HIP(h, hipMemcpyAsync(hv, a_send, 16 * G, hipMemcpyDeviceToHost, s));
        WQ_HIP(h, hipStreamSynchronize(s));
        for (uint32_t d = 0; d < G; ++d) {
            const bool none = !self_seg && d == me;
            sc.b1_out[d] = none ? 0u : whole_blocks(hv[2 * d]);
            sc.b1_in[d] = none ? 0u : whole_blocks(hv[2 * G + 2 * d]);
        }
    }
    uint64_t so = 0, ro = 0;
    for (uint32_t d = 0; d < G; ++d) {
        x.L.base[d] = (uint32_t)so;
        x.L.budget[d] = sc.b1_out[d];
        x.sb.b[d] = (uint32_t)so;
        x.rb.b[d] = (uint32_t)ro;
        so += sc.b1_out[d];
        ro += sc.b1_in[d];
    }
    x.L.base[G] = x.sb.b[G] = (uint32_t)so;
    x.rb.b[G] = (uint32_t)ro;
    if (so >= (1ull << 31) || ro >= (1ull << 31)) return fatal_receive(h, "sharded tick: more than 2^31 slots");
    const uint64_t Sb = x.Sb = so, Rb = x.Rb = ro;
    if (alloc(sc.slots, (Sb + 2) * kSlotWords * 4) || alloc(sc.perm, (Sb + 2) * 4) ||
        alloc(sc.rslots, (Rb + 2) * kSlotWords * 4))
        return fatal_receive(h, "hipMalloc of the sharded tick's slots");
    if (!late) fail(group(exact ? 2 : 3, x.L));
    if (late) {  // nothing to send: tail slots everywhere (zero words route to nobody either way)
        WQ_HIP(h, hipMemsetAsync(sc.slots.p, 0, (Sb + 1) * kSlotWords * 4, s));
        WQ_HIP(h, hipMemsetAsync(sc.perm.p, 0xFF, (Sb + 1) * 4, s));
        if (!exact && (rc = put_status(a_send))) return rc;
    }
    std::vector<size_t> sbytes(G), rbytes(G);
    for (uint32_t d = 0; d < G; ++d) {
        sbytes[d] = (size_t)sc.b1_out[d] * kSlotWords * 4;
        rbytes[d] = (size_t)sc.b1_in[d] * kSlotWords * 4;
    }
    if (exact) {
        Xfer xs{{sc.slots.p}, {sbytes.data()}, {sc.rslots.p}, {rbytes.data()}, 1};
        xs.skip_self[0] = x.self_in_place && !late;
        return exchange(h, xs);
    }
    Xfer xs{{a_send, sc.slots.p}, {eight.data(), sbytes.data()}, {a_recv, sc.rslots.p}, {eight.data(), rbytes.data()}, 2};
    xs.skip_self[0] = x.a_in_place && !late;
    xs.skip_self[1] = x.self_in_place && !late;
    return exchange(h, xs);
}

// The global picture of a finished tick from its small vectors (the same on every shard: codes and
// device bits from every shard's A and C), and the next tick's budgets from its true sizes when it
// was clean; a tick whose sizes outgrew a budget leaves the budgets off (the next tick is exact).
// self_seg: the owner form on slots — A only, and the self segment budgeted like the others (so
// G = 1 has statuses too); else this shard's own segments are empty.
TickPicture fold_tick(ShardCtx& sc, const char* hs, bool self_seg) {
    const uint32_t G = sc.G, me = sc.rank;
    const uint32_t* ha = reinterpret_cast<const uint32_t*>(hs + kSmallA);
    const uint32_t* hc = reinterpret_cast<const uint32_t*>(hs + kSmallC);
    TickPicture t;
    if (G == 1 && !self_seg) return t;  // nothing was exchanged
    for (uint32_t d = 0; d < G; ++d) {
        for (uint32_t st : {ha[2 * G + 2 * d + 1], self_seg ? 0u : hc[2 * G + 2 * d + 1]}) {
            if ((st & kStCodeMask) && !t.code) t.code = st & kStCodeMask, t.code_from = d;
            if (((st >> 8) & 0xFFFFu) && !t.bits) t.bits = (st >> 8) & 0xFFFFu, t.bits_from = d;
            t.over |= (st & kStBudget) != 0;
        }
    }
    if (!t.code && !t.over) {  // next tick's budgets from this tick's true sizes
        for (uint32_t d = 0; d < G; ++d) {
            const bool none = !self_seg && d == me;
            sc.b1_out[d] = none ? 0u : slot_budget(ha[2 * d]);
            sc.b1_in[d] = none ? 0u : slot_budget(ha[2 * G + 2 * d]);
            if (self_seg) continue;
            sc.b2_out[d] = none ? 0 : pool_budget(hc[2 * d]);
            sc.b2_in[d] = none ? 0 : pool_budget(hc[2 * G + 2 * d]);
        }
        sc.budgets = true;
    }
    if (t.over) sc.budgets = false;
    return t;
}

// Folds in the snapshots of asynchronous ticks until at most `keep` are in flight (oldest first,
// waiting for each; every shard makes the same calls, so every shard folds the same ticks).
int async_drain(wq_router* h, uint32_t keep) {
    ShardCtx& sc = *h->shard;
    while (sc.acount > keep) {
        const uint32_t k = sc.ahead;
        // k_async_result writes the snapshot, then its sequence word (system-scope release)
        const volatile uint64_t* seq =
            reinterpret_cast<const volatile uint64_t*>(static_cast<const char*>(sc.asnap[k]) + kSmallBytes);
        const auto t0 = std::chrono::steady_clock::now();
        while (*seq != sc.aseq[k]) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
                // name everything a post-mortem needs: which tick, which ring slot, what the word holds,
                // and whether the stream still had work (idle + wrong word = the snapshot was never written)
                const hipError_t q = hipStreamQuery(h->stream);
                char msg[320];
                snprintf(msg, sizeof msg,
                         "asynchronous sharded tick: its result never arrived (tick %llu of this handle, ring slot %u "
                         "of %u, %u in flight; sequence word expected %llu, observed %llu; stream %s)",
                         (unsigned long long)sc.aseq[k], k, ShardCtx::kRing, sc.acount, (unsigned long long)sc.aseq[k],
                         (unsigned long long)*seq,
                         q == hipSuccess ? "idle" : q == hipErrorNotReady ? "busy" : hipGetErrorString(q));
                return set_error(h, WQ_E_TIMEOUT, msg);
            }
            std::this_thread::yield();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        const char* snap = static_cast<const char*>(sc.asnap[k]);
        (void)fold_tick(sc, snap, sc.budget_form == 1);  // the ring only ever holds one form's ticks
        if (sc.budget_form == 1) {  // the owner form: a pair buffer that was short grows for the next tick
            const uint64_t P = reinterpret_cast<const wq_route_counters*>(snap + kSmallCnt)[kCntScan].n_pairs;
            if (P > sc.own_cap) sc.own_cap = std::min<uint64_t>(P + P / 4 + 4096, 0xFFFFFFFFull);
        }
        sc.ahead = (k + 1) % ShardCtx::kRing;
        sc.acount--;
    }
    return WQ_OK;
}

// The asynchronous end of a budgeted tick: no host read; the small vectors go to a pinned snapshot
// the next calls fold in (budgets), P and the statuses to the caller's counters and the health
// words — at the end of the tile scan when one block runs it (the tick hands these parameters to
// it), else by k_async_result. The snapshot is the ring's next free slot (async_drain left one).
AsyncResultParams TickFrame::async_params(bool statuses, bool has_msgs, uint64_t capacity, wq_route_counters* d_result) {
    AsyncResultParams ar{};
    ar.a_recv = a_recv;
    ar.c_recv = c_recv;  // the owner form: zero, no second exchange
    ar.G = G;
    ar.statuses = statuses ? 1u : 0u;
    ar.cnt = cnts;
    ar.has_msgs = has_msgs ? 1u : 0u;
    ar.capacity = capacity;
    ar.out = d_result;
    ar.health = route_health(h);
    ar.small = reinterpret_cast<const uint32_t*>(small);
    ar.snap = static_cast<uint32_t*>(sc.asnap[(sc.ahead + sc.acount) % ShardCtx::kRing]);
    ar.seq = sc.n_async + 1;
    ar.zero = reinterpret_cast<uint32_t*>(small);
    return ar;
}

// ... and its ring commit. A shard whose local step failed takes this end too, and then returns its
// error: whether a tick is queued in the snapshot ring must be decided by state every shard shares,
// or the shards would fold different ticks and size their next exchanges differently.
int TickFrame::finish_async(const AsyncResultParams& ar, bool ar_done) {
    if (!ar_done) {
        hipLaunchKernelGGL(k_async_result, dim3(1), dim3(256), 0, s, ar);
        WQ_HIP(h, hipGetLastError());
    }
    const uint32_t ak = (sc.ahead + sc.acount) % ShardCtx::kRing;
    sc.acount++;
    sc.n_async++;
    sc.aseq[ak] = sc.n_async;
    sc.small_zeroed = true;
    if (late) {  // st_host (the status copies' source) lives on the frame: let them finish first
        WQ_HIP(h, hipStreamSynchronize(s));
        return late.report(h);
    }
    return WQ_OK;
}

// The synchronous end, the tick's one host read: the small vectors (*hcnt: their counter blocks —
// P, the statuses, the true sizes), folded into the next tick's budgets. Returns this shard's own
// failure, else the first failed shard's; *redo when a budget was short anywhere (every shard saw
// it: all of them redo the tick exactly); then any shard's device error bits.
int TickFrame::read_back(bool self_seg, bool* redo, const wq_route_counters** hcnt) {
    WQ_HIP(h, hipMemcpyAsync(sc.hsmall, small, kSmallUsed, hipMemcpyDeviceToHost, s));
    WQ_HIP(h, hipStreamSynchronize(s));
    const char* hs = static_cast<const char*>(sc.hsmall);
    *hcnt = reinterpret_cast<const wq_route_counters*>(hs + kSmallCnt);
    const TickPicture tp = fold_tick(sc, hs, self_seg);
    if (late) return late.report(h);
    if (tp.code) return status_error(h, tp.code, tp.code_from);
    if (tp.over) {
        *redo = true;
        return WQ_OK;
    }
    if (tp.bits) return status_error(h, (uint64_t)tp.bits << 32, tp.bits_from);
    return WQ_OK;
}

// One call of either form (0 the slot tick, 1 the owner form on slots). Earlier asynchronous ticks
// first: a synchronous tick folds them all in; an asynchronous one keeps the latest in flight (its
// budgets come from the tick before), unless it must run exact — as the first tick after the other
// form does, whose budgets treat the self segment differently (the ring then holds only one form's
// ticks). Then tick(exact, inject, &redo, async), redone exactly when a budget was short.
template <class Tick>
int budgeted_call(wq_router* h, int form, bool async, Tick tick) {
    ShardCtx& sc = *h->shard;
    if (sc.budget_form != form) {
        if (int rc = async_drain(h, 0)) return rc;
        sc.budgets = false;
        sc.budget_form = form;
    } else if (int rc = async_drain(h, async && sc.budgets ? 1u : 0u)) {
        return rc;
    }
    const int inject = h->shard_inject;
    h->shard_inject = 0;
    bool redo = false;
    // (the slot tick at G = 1 exchanges nothing: it has no sizes to learn)
    int rc = tick((form == 1 || sc.G > 1) && !sc.budgets, inject, &redo, async);
    if (rc == WQ_OK && redo) rc = tick(true, 0, &redo, false);
    return rc;
}

// An asynchronous call that ran synchronously (exact, redone, or a local failure) leaves its result
// in the caller's counters all the same.
int put_result(wq_router* h, wq_route_counters* d_result, const wq_route_counters& c) {
    WQ_HIP(h, hipMemcpyAsync(d_result, &c, sizeof(c), hipMemcpyHostToDevice, h->stream));
    WQ_HIP(h, hipStreamSynchronize(h->stream));  // c lives on the caller's stack frame
    return WQ_OK;
}

// ---------------------------------------------------------------------------------------------
// The slot tick (radius filter off) — wq_sharded_route_tick_device's result, built as
//   own     this shard's own cubes: count_kernel<OWN> over the caller's messages, on a side stream
//           beside the exchanges (no slot, nothing crosses a link)
//   X1      {A: slots + status per owner, the slots: 20 B per remote message, budgeted segments}
//   owner   count the received slots (count_kernel<SLOTS>), claim each (source, cube) once
//           (k_ref_claim), a 12-byte reference per slot and per source ONE pool of cube lists
//   X2      {C: pool words + status per source, the references, the pools}
//   ingest  references -> rows (k_ref_resolve), tile scan, emit_map_kernel over own + pool rows
//   end     ONE host read: P, every shard's status, the true sizes (the next tick's budgets)
// so a long list crosses xGMI once per (tick, destination), and the exchanges are enqueued without
// reading anything back: their sizes are the budgets, fixed on the host before the tick (the
// previous tick's true sizes + 1/16 + a block; identical on both ends of every pair, since both saw
// the same sizes). A tick whose sizes outgrow a budget is flagged on the device; the status reaches
// every shard through C, and all of them redo the tick exactly: A and C exchanged alone first and
// read back, as the first tick does. Local failures keep the collective going: a failed step sends
// its status (zero slots / empty pools) and every shard returns the error after X2.
// ---------------------------------------------------------------------------------------------
struct CsrOut {
    uint32_t* offsets;
    uint32_t* peers;
    uint32_t* msgs;
    size_t capacity;
};

struct SlotTick : TickFrame {
    const TickIn in;
    const size_t M;
    TableView tv{};
    bool radius = false;
    uint32_t nt = 0;          // 256-message tiles
    bool own_slots = false;   // this shard's own messages are grouped as slots too (never exchanged)
    bool hist_ready = false;  // the fused own-cube count left the grouping's histogram
    bool forked = false;      // the side stream counts the own cubes: join before their rows are read
    SlotSegs x;
    std::vector<uint64_t> pb, prb;  // pool segment bases (words) in the send / receive buffer
    SlotTick(wq_router* h_, const TickIn& in_, bool exact_, int inject_)
        : TickFrame(h_, exact_, inject_), in(in_), M(in_.M), pb(G + 1, 0), prb(G + 1, 0) {}
    int own_cubes();
    void owner_count();
    int own_slots_count();
    void owner_refs();
    int exchange_pools();
    int ingest_rows();
    int run(const CsrOut& out, size_t* n_pairs, bool* redo, bool async, wq_route_counters* d_result);
};

// ---- own cubes. G > 1 without the radius filter (own slots): the grouping pass writes this
// shard's own messages as slots of a segment that is never exchanged, and the side stream counts
// them once grouped (own_slots_count), beside the exchanges and the owner's work — the grouping's
// histogram pass quantises every message, but probes nothing. Otherwise the own-cube count runs
// over every message on the side stream (count_kernel<OWN>), or (diagnostics,
// WQ_SHARD_OWN_FUSED) in one pass with the histogram on the tick's stream, as in round 4 ----
int SlotTick::own_cubes() {
    static const bool two_pass = getenv("WQ_DEBUG_NO_OWN_HIST") != nullptr;  // diagnostics
    static const bool fused_env = getenv("WQ_SHARD_OWN_FUSED") != nullptr;   // diagnostics
    own_slots = G > 1 && !radius && !two_pass && !fused_env;
    const bool fuse = G > 1 && !radius && budget_slot_tile() == kHistTiles * kBlock && !two_pass && fused_env;
    if (!late && M && own_slots) {
        // (a message no step writes a row for — its slot was over budget, the tick is redone —
        // routes to nobody: the histogram pass zeroes every e)
        const uint64_t nto = (2 * M + kBlock - 1) / kBlock;
        if (!fail(alloc(sc.own_slots, (2 * M + 2) * kSlotWords * 4)) && !fail(alloc(sc.own_perm, (2 * M + 2) * 4)))
            fail(alloc(sc.own_tiles, (nto + 1) * 8));
    }
    if (late || !M || (own_slots && !fuse)) return WQ_OK;
    RouteIn rin{in.pos, in.keys, in.world, in.sender, in.repl, (uint32_t)M, (int64_t)h->cube_size};
    rin.own_G = G;
    rin.own_me = me;
    const CountParams cp = count_params(tv, rin, sc.e_msg.as<uint32_t>(), sc.info_msg.as<uint2>(), sc.mtiles.as<uint32_t>(),
                                        2 * (uint64_t)nt, nt, kCntSelf);
    if (fuse) {
        const uint32_t nblk = (uint32_t)((M + kHistTiles * kBlock - 1) / (kHistTiles * kBlock));
        if (fail(alloc(h->shard_hist, (uint64_t)nblk * G * 4))) return WQ_OK;
        if (in.keys)
            hipLaunchKernelGGL(own_count_hist_kernel<true>, dim3(nblk), dim3(kBlock), 0, s, cp, nblk,
                               h->shard_hist.as<uint32_t>());
        else
            hipLaunchKernelGGL(own_count_hist_kernel<false>, dim3(nblk), dim3(kBlock), 0, s, cp, nblk,
                               h->shard_hist.as<uint32_t>());
        WQ_HIP(h, hipGetLastError());
        hist_ready = true;
        return WQ_OK;
    }
    WQ_HIP(h, hipEventRecord(sc.ev_fork, s));
    WQ_HIP(h, hipStreamWaitEvent(sc.side, sc.ev_fork, 0));
    const dim3 grid(pass_blocks(nt));  // as launch_route
    if (radius && G == 1)
        hipLaunchKernelGGL(count_radius_kernel<false>, dim3(nt), dim3(kBlock), 0, sc.side, cp);
    else if (radius)
        hipLaunchKernelGGL(count_radius_kernel<true>, dim3(nt), dim3(kBlock), 0, sc.side, cp);
    else if (G == 1 && in.keys)
        hipLaunchKernelGGL((count_kernel<true, 1, 8>), grid, dim3(kBlock), 0, sc.side, cp);
    else if (G == 1)
        hipLaunchKernelGGL((count_kernel<false, 1, 8>), grid, dim3(kBlock), 0, sc.side, cp);
    else if (in.keys)
        hipLaunchKernelGGL((count_kernel<true, 1, 8, 0, false, false, true>), grid, dim3(kBlock), 0, sc.side, cp);
    else
        hipLaunchKernelGGL((count_kernel<false, 1, 8, 0, false, false, true>), grid, dim3(kBlock), 0, sc.side, cp);
    WQ_HIP(h, hipGetLastError());
    WQ_HIP(h, hipEventRecord(sc.ev_join, sc.side));
    forked = true;
    return WQ_OK;
}

// ---- the owner, first half: count the received slots (local_message.rs:52-86 per slot) ----
void SlotTick::owner_count() {
    RouteWs& rw = h->rws;
    const uint64_t Rb = x.Rb;
    const uint32_t nto = (uint32_t)(Rb / kBlock);  // whole blocks
    if (fail(alloc(rw.e, Rb * 4)) || fail(alloc(rw.info, Rb * 8)) || fail(alloc(sc.otiles, (uint64_t)nto * 8)) ||
        fail(alloc(sc.ocnt, Rb * 4)) || fail(alloc(sc.hslot, Rb * 4)) || fail(alloc(sc.desc_fill, (Rb + 1) * 16)))
        return;
    const CountParams cp = count_params(tv, slots_in(sc.rslots.as<uint32_t>(), (uint32_t)Rb), rw.e.as<uint32_t>(),
                                        rw.info.as<uint2>(), sc.otiles.as<uint32_t>(), nto, nto, kCntOwner);
    hipLaunchKernelGGL((count_kernel<false, 1, 8, 0, false, true>), dim3(pass_blocks(nto)), dim3(kBlock), 0, s, cp);
    if (hipGetLastError() != hipSuccess) fail(set_error(h, WQ_E_HIP, "count launch (sharded tick)"));
}

// ---- the own slots (their count: the own column of this tick's histogram, a_send[2 me], known on
// the device only) counted on the side stream, e / locator straight to message order. After the
// owner count: beside the claims, references, pool gather and X2 (beside the owner count, the two
// probe passes only slowed each other down) ----
int SlotTick::own_slots_count() {
    WQ_HIP(h, hipEventRecord(sc.ev_fork, s));
    WQ_HIP(h, hipStreamWaitEvent(sc.side, sc.ev_fork, 0));
    const uint32_t n_max = (uint32_t)(2 * M);
    const uint32_t nto = (n_max + kBlock - 1) / kBlock;
    const CountParams cp = count_params(tv, slots_in(sc.own_slots.as<uint32_t>(), n_max, a_send + 2 * me),
                                        sc.e_msg.as<uint32_t>(), sc.info_msg.as<uint2>(), sc.own_tiles.as<uint32_t>(), nto,
                                        nto, kCntSelf, sc.own_perm.as<uint32_t>());
    hipLaunchKernelGGL((count_kernel<false, 1, 8, 0, false, true>), dim3(std::min<uint32_t>(nto, 4096u)),
                       dim3(kBlock), 0, sc.side, cp);
    WQ_HIP(h, hipGetLastError());
    WQ_HIP(h, hipEventRecord(sc.ev_join, sc.side));
    forked = true;
    return WQ_OK;
}

// ---- the owner, second half: claim each (source, cube) once, the references ----
void SlotTick::owner_refs() {
    RouteWs& rw = h->rws;
    const uint64_t Rb = x.Rb;
    uint64_t C = 1024;  // claim table: load <= 1/2
    while (C < 2 * Rb) C <<= 1;
    if (!late && C > sc.claim_cap) {
        if (!fail(alloc(sc.claim, C * 8)) && !fail(alloc(sc.lead, C * 4))) {
            if (hipMemsetAsync(sc.claim.p, 0, C * 8, s) != hipSuccess) fail(set_error(h, WQ_E_HIP, "memset"));
            sc.claim_cap = C;
        }
    }
    C = sc.claim_cap;
    if (late) return;
    const uint64_t period = (1ull << kRefClaimTagBits) - 1;
    if (sc.ticks && sc.ticks % period == 0 && hipMemsetAsync(sc.claim.p, 0, sc.claim_cap * 8, s) != hipSuccess)
        fail(set_error(h, WQ_E_HIP, "memset"));  // the tags wrap: forget them all
    RefOwnerParams rp{};
    rp.e = rw.e.as<uint32_t>();
    rp.info = rw.info.as<uint2>();
    rp.list = tv.list;
    rp.recs = tv.recs;
    rp.rrem = x.rb;
    rp.G = G;
    rp.n_rem = (uint32_t)Rb;
    rp.self_lo = (uint32_t)Rb;  // no own segment: received slot t is remote slot t
    rp.n_self = 0;
    rp.tag = (uint32_t)(sc.ticks % period) + 1u;
    rp.claim = sc.claim.as<unsigned long long>();
    rp.lead = sc.lead.as<uint32_t>();
    rp.cmask = C - 1;
    rp.cnt = sc.ocnt.as<uint32_t>();
    rp.hslot = sc.hslot.as<uint32_t>();
    rp.plen = sc.plen.as<uint32_t>();
    rp.poff = sc.poff.as<uint32_t>();
    rp.ref_send = sc.ref_send.as<uint3>();
    rp.desc_fill = sc.desc_fill.as<uint4>();
    sc.ticks++;
    hipLaunchKernelGGL(k_ref_claim, dim3((unsigned)((Rb + kBlock) / kBlock)), dim3(kBlock), 0, s, rp);
    if (hipGetLastError() != hipSuccess) fail(set_error(h, WQ_E_HIP, "claim launch (sharded tick)"));
    if (!late) fail(scan_excl(h, sc.tmp, sc.plen.as<uint32_t>(), sc.poff.as<uint32_t>(), Rb + 1));
    if (!late) {
        hipLaunchKernelGGL(k_ref_make, dim3((unsigned)(Rb / kBlock)), dim3(kBlock), 0, s, rp);
        if (hipGetLastError() != hipSuccess) fail(set_error(h, WQ_E_HIP, "reference launch (sharded tick)"));
    }
}

// ---- X2: C + the references and pools (G > 1) ----
int SlotTick::exchange_pools() {
    const uint64_t Sb = x.Sb, Rb = x.Rb;
    int rc;
    const bool owner_ok = Rb && !late;
    if (!late) {
        CVecParams cv{};
        cv.a_send = a_send;
        cv.a_recv = a_recv;
        cv.poff = owner_ok ? sc.poff.as<uint32_t>() : nullptr;
        cv.rb = x.rb;
        for (uint32_t d = 0; d < G; ++d) cv.b2[d] = exact ? ~0ull : sc.b2_out[d];
        cv.G = G;
        cv.stale = tv.stale;
        cv.cnt = owner_ok ? cnts + kCntOwner : nullptr;
        cv.c_send = c_send;
        hipLaunchKernelGGL(k_c_vector, dim3(1), dim3(64), 0, s, cv);
        if (hipGetLastError() != hipSuccess) fail(set_error(h, WQ_E_HIP, "size launch (sharded tick)"));
    }
    if (late) {
        if ((rc = put_status(c_send))) return rc;
        WQ_HIP(h, hipMemsetAsync(sc.ref_send.p, 0, (Rb + 1) * 12, s));  // references that route to nobody
    }
    if (exact) {  // the true pool sizes first (C alone, read back)
        Xfer xc{{c_send}, {eight.data()}, {c_recv}, {eight.data()}, 1};
        if ((rc = exchange(h, xc))) return rc;
        uint32_t* hv = static_cast<uint32_t*>(sc.hsmall);
        WQ_HIP(h, hipMemcpyAsync(hv, c_send, 16 * G, hipMemcpyDeviceToHost, s));
        WQ_HIP(h, hipStreamSynchronize(s));
        for (uint32_t d = 0; d < G; ++d) {
            sc.b2_out[d] = d == me ? 0 : hv[2 * d];
            sc.b2_in[d] = d == me ? 0 : hv[2 * G + 2 * d];
        }
    }
    for (uint32_t d = 0; d < G; ++d) {
        pb[d + 1] = pb[d] + sc.b2_out[d];
        prb[d + 1] = prb[d] + sc.b2_in[d];
    }
    if (prb[G] >= (1ull << 30)) return fatal_receive(h, "sharded tick: more than 2^30 pool words to receive");
    if (alloc(sc.pool_send, (pb[G] + 1) * 4) || alloc(sc.pool_recv, (prb[G] + 1) * 4) || alloc(sc.ref_recv, (Sb + 1) * 12))
        return fatal_receive(h, "hipMalloc of the references / pools");
    if (owner_ok && !late && pb[G]) {
        const uint32_t nbo = (uint32_t)(Rb / kBlock);
        if (alloc(sc.blk, (uint64_t)nbo * 16 + 16)) return fatal_receive(h, "hipMalloc of the pool blocks");
        PoolBlocksParams bp{};
        bp.poff = sc.poff.as<uint32_t>();
        bp.rb = x.rb;
        for (uint32_t d = 0; d <= G; ++d) bp.pb[d] = pb[d];
        bp.G = G;
        bp.nblk = nbo;
        bp.base = sc.blk.as<uint64_t>();
        bp.lim = bp.base + nbo;
        hipLaunchKernelGGL(k_pool_blocks, dim3((nbo + kBlock - 1) / kBlock), dim3(kBlock), 0, s, bp);
        GatherParams gp{sc.poff.as<uint32_t>(), sc.desc_fill.as<uint4>(), (uint32_t)Rb, sc.pool_send.as<uint32_t>(),
                        nullptr, pb[G]};
        gp.blk_base = bp.base;
        gp.blk_lim = bp.lim;
        hipLaunchKernelGGL((gather_rows_kernel<16, false>), dim3(nbo), dim3(kBlock), 0, s, gp);
        if (hipGetLastError() != hipSuccess) return fatal_receive(h, "pool gather launch");
    }
    std::vector<size_t> rs(G), rr(G), ps(G), pr(G);
    uint64_t sent = 0, recvd = 0;
    for (uint32_t d = 0; d < G; ++d) {
        rs[d] = (size_t)sc.b1_in[d] * 12;   // references for the slots d sent here
        rr[d] = (size_t)sc.b1_out[d] * 12;  // references for the slots sent to d
        ps[d] = (size_t)sc.b2_out[d] * 4;
        pr[d] = (size_t)sc.b2_in[d] * 4;
        if (d != me) {
            sent += 16 + (uint64_t)sc.b1_out[d] * kSlotWords * 4 + rs[d] + ps[d];
            recvd += 16 + (uint64_t)sc.b1_in[d] * kSlotWords * 4 + rr[d] + pr[d];
        }
    }
    if (exact) {
        Xfer xp{{sc.ref_send.p, sc.pool_send.p}, {rs.data(), ps.data()}, {sc.ref_recv.p, sc.pool_recv.p},
                {rr.data(), pr.data()}, 2};
        if ((rc = exchange(h, xp))) return rc;
    } else {
        Xfer xp{{c_send, sc.ref_send.p, sc.pool_send.p}, {eight.data(), rs.data(), ps.data()},
                {c_recv, sc.ref_recv.p, sc.pool_recv.p}, {eight.data(), rr.data(), pr.data()}, 3};
        if ((rc = exchange(h, xp))) return rc;
    }
    sc.last_sent = sent;
    sc.last_recv = recvd;
    return WQ_OK;
}

// ---- the ingesting side: rows in message order (then the CSR: slots_copy_out) ----
int SlotTick::ingest_rows() {
    const uint64_t Sb = x.Sb;
    if (forked && !own_slots) WQ_HIP(h, hipStreamWaitEvent(s, sc.ev_join, 0));  // own rows written (remote: e = 0)
    if (!late && G > 1 && Sb) {
        ResolveParams rv{};
        rv.perm = sc.perm.as<uint32_t>();
        rv.ref_recv = sc.ref_recv.as<uint3>();
        rv.sb = x.sb;
        rv.G = G;
        rv.n = (uint32_t)Sb;
        for (uint32_t d = 0; d <= G; ++d) rv.prb[d] = prb[d];
        rv.e_msg = sc.e_msg.as<uint32_t>();
        rv.info_msg = sc.info_msg.as<uint2>();
        const dim3 rg((unsigned)((Sb + kBlock - 1) / kBlock));
        if (radius) {
            rv.pool = sc.pool_recv.as<uint32_t>();
            rv.pos = in.pos;
            rv.sender = in.sender;
            rv.repl = in.repl;
            rv.tv = tv;
            hipLaunchKernelGGL(k_ref_resolve<true>, rg, dim3(kBlock), 0, s, rv);
        } else {
            hipLaunchKernelGGL(k_ref_resolve<false>, rg, dim3(kBlock), 0, s, rv);
        }
        WQ_HIP(h, hipGetLastError());
    }
    if (forked && own_slots) WQ_HIP(h, hipStreamWaitEvent(s, sc.ev_join, 0));  // own rows written
    // the per-tile totals of every row (a count pass's held its own rows only)
    if (!late && G > 1 && M && (Sb || own_slots)) {
        hipLaunchKernelGGL(row_tile_sums_kernel, dim3(nt), dim3(kBlock), 0, s, sc.e_msg.as<uint32_t>(), (uint32_t)M,
                           sc.mtiles.as<uint32_t>());
        WQ_HIP(h, hipGetLastError());
    }
    if (!late) {
        sc.last_M = M;
        sc.last_sender = in.sender;
        sc.last_pos = in.pos;
        sc.last_repl = in.repl;
        sc.last_radius = radius;
        sc.last_gen = h->table_gen;
    }
    return WQ_OK;
}

int SlotTick::run(const CsrOut& out, size_t* n_pairs, bool* redo, bool async, wq_route_counters* d_result) {
    *redo = false;
    sc.last_ready = false;
    sc.last_slots = true;
    int rc;
    if ((rc = begin())) return rc;

    if (inject == 1) fail(set_error(h, WQ_E_INVALID, "injected failure at step 1 (test hook)"));
    // the radius filter (C5): own cubes by count_radius_kernel, remote rows filtered where they land
    radius = h->radius > 0.0;
    if (radius && M && !in.pos && !late) fail(set_error(h, WQ_E_INVALID, "the radius filter needs message positions"));
    // fold in a finished incremental batch first (it may rebuild the table the rows point into)
    if (!late) fail(table_resolve(h, false));
    if (!late && G > 1 && h->tab.list.bytes / 4 >= (1ull << 30))
        fail(set_error(h, WQ_E_CAPACITY, "sharded tick: more than 2^30 list words on one shard"));
    tv = table_view(h);
    nt = (uint32_t)((M + kBlock - 1) / kBlock);
    if (!late && !fail(alloc(sc.e_msg, (M + 1) * 4)) && !fail(alloc(sc.info_msg, (M + 1) * 8)))
        fail(alloc(sc.mtiles, ((uint64_t)nt * 3 + 4) * 4));

    if ((rc = own_cubes())) return rc;

    // ---- X1: A + the slots (this shard's own messages take none: its segments are empty) ----
    if (G > 1) {
        uint32_t* zero_e = own_slots ? sc.e_msg.as<uint32_t>() : nullptr;
        rc = exchange_slots(false, x, [&](int phases, const SlotLayout& L) {
            if (phases == 1)
                return launch_budget_slots(h, in.pos, in.keys, in.world, in.sender, in.repl, M, G, me, L, nullptr, nullptr,
                                           a_send, 1, hist_ready, own_slots, nullptr, nullptr, zero_e);
            return launch_budget_slots(h, in.pos, in.keys, in.world, in.sender, in.repl, M, G, me, L, sc.slots.as<uint32_t>(),
                                       sc.perm.as<uint32_t>(), a_send, phases, hist_ready, own_slots,
                                       sc.own_slots.as<uint32_t>(), sc.own_perm.as<uint32_t>(), exact ? nullptr : zero_e);
        });
        if (rc) return rc;
    }

    // ---- the owner: count the received slots, claims, references ----
    if (inject == 3) fail(set_error(h, WQ_E_INVALID, "injected failure at step 3 (test hook)"));
    const uint64_t Rb = x.Rb;
    if (G > 1 && (alloc(sc.ref_send, (Rb + 1) * 12) || alloc(sc.plen, (Rb + 1) * 4) || alloc(sc.poff, (Rb + 1) * 4)))
        return fatal_receive(h, "hipMalloc of the owner's references");
    if (G > 1 && Rb && !late) owner_count();
    if (G > 1 && !late && M && own_slots && (rc = own_slots_count())) return rc;
    if (G > 1 && Rb && !late) owner_refs();

    // ---- X2, then the rows in message order ----
    if (G == 1) sc.last_sent = sc.last_recv = 0;
    if (G > 1 && (rc = exchange_pools())) return rc;
    if ((rc = ingest_rows())) return rc;

    // ---- asynchronous end (wq_sharded_route_tick_async, a budgeted tick) ----
    if (async && !exact) {
        const AsyncResultParams ar = async_params(G > 1, M != 0, out.capacity, d_result);
        bool ar_done = false;
        if (!late && (rc = slots_copy_out(h, out.offsets, out.peers, out.msgs, out.capacity, &ar, &ar_done))) return rc;
        sc.last_ready = false;  // no copy-out of an unread tick (its P is on the device)
        *n_pairs = 0;
        return finish_async(ar, ar_done);
    }
    if (!late && (rc = slots_copy_out(h, out.offsets, out.peers, out.msgs, out.capacity))) return rc;

    // ---- the one host read: P, the statuses, the true sizes ----
    const wq_route_counters* hcnt;
    if ((rc = read_back(false, redo, &hcnt)) || *redo) return rc;
    const uint32_t err = hcnt[kCntScan].error | hcnt[kCntSelf].error | hcnt[kCntOwner].error;
    const uint64_t P = M ? hcnt[kCntScan].n_pairs : 0;
    sc.last_P = P;
    sc.last_ready = true;
    *n_pairs = P;
    if (err) return status_error(h, (uint64_t)err << 32, me);
    if (P > out.capacity) return set_error(h, WQ_E_CAPACITY, "sharded tick: output capacity too small (required size in *n_pairs)");
    return WQ_OK;
}

// ---------------------------------------------------------------------------------------------
// The owner form on budgeted slots (wq_sharded_route_owner_slots).
// Every message becomes a 20-byte slot of its owner's budgeted segment — this shard's own messages
// included (the self segment is a device copy) — and X1 {A, the slots} is the tick's only exchange:
// each owner routes what it received where it is (count_kernel<SLOTS>, the tile scan and
// emit_map_kernel over the received slots) and the pairs stay there (first
// option; area_map.rs:52-60 per slot). No claims, references, pools or second exchange. The budgets
// work as in the slot tick (the previous tick's true sizes + headroom, the first tick exact); a short
// budget anywhere reaches every shard through X1 (ShardIn::a_or) and all of them redo the tick
// exactly. One host read at the end: P, the statuses, the true sizes.
// ---------------------------------------------------------------------------------------------
int owner_emit(wq_router* h, uint64_t Rb, const TableView& tv, const AsyncResultParams* ar = nullptr,
               bool* ar_done = nullptr) {
    ShardCtx& sc = *h->shard;
    RouteWs& rw = h->rws;
    hipStream_t s = h->stream;
    const uint32_t nto = (uint32_t)(Rb / kBlock);
    uint32_t* tiles = sc.otiles.as<uint32_t>();
    TileScanParams tp;
    tp.tile_total = tiles;
    tp.tile_F = tiles + nto;
    tp.tile_prefix = tiles + 2 * (uint64_t)nto;
    tp.n_tiles = nto;
    tp.offsets = sc.own_off.as<uint32_t>();
    tp.M = (uint32_t)Rb;
    tp.capacity = sc.own_cap;
    tp.cnt = reinterpret_cast<wq_route_counters*>(sc.small.as<char>() + kSmallCnt) + kCntScan;
    tp.health = nullptr;  // a short pair buffer is grown and emitted again, not an overflow
    tp.stale = tv.stale;
    if (ar) {  // an asynchronous tick: the scan ends it (if it is the one-block scan)
        tp.ar = *ar;
        tp.async_end = true;
    }
    if (int rc = launch_tile_scan(h, tp, ar_done)) return rc;
    EmitParams ep;
    ep.sender = sc.rslots.as<uint32_t>() + 3;  // OnlySelf rows: the slot's sender word
    ep.sender_stride = kSlotWords;
    ep.pos = nullptr;
    ep.repl = nullptr;
    ep.M = (uint32_t)Rb;
    ep.t = tv;
    ep.e = rw.e.as<uint32_t>();
    ep.tile_prefix = tp.tile_prefix;
    ep.count_tile = kBlock;
    ep.offsets = tp.offsets;
    ep.info = rw.info.as<uint2>();
    ep.peers = sc.own_peers.as<uint32_t>();
    ep.msgs = nullptr;  // the CSR over the received slots says whose each pair is
    ep.capacity = sc.own_cap;
    ep.n_blocks = nto;
    hipLaunchKernelGGL((emit_map_kernel<16>), dim3(pass_blocks(nto)), dim3(kBlock), 0, s, ep);
    WQ_HIP(h, hipGetLastError());
    return WQ_OK;
}

int owner_slot_tick(wq_router* h, const TickIn& in, bool exact, int inject, bool* redo, wq_owner_slot_view* out,
                    bool async, wq_route_counters* d_result) {
    ShardCtx& sc = *h->shard;
    *redo = false;
    sc.last_ready = false;
    sc.last_slots = false;
    TickFrame f(h, exact, inject);
    hipStream_t s = f.s;
    const uint32_t G = f.G, me = f.me;
    const size_t M = in.M;
    int rc;
    if ((rc = f.begin())) return rc;
    if (inject == 1) f.fail(set_error(h, WQ_E_INVALID, "injected failure at step 1 (test hook)"));
    if (h->radius > 0.0 && !f.late)
        f.fail(set_error(h, WQ_E_INVALID, "the owner form on slots has no radius filter (wq_sharded_route_owner_device has)"));
    if (!f.late) f.fail(table_resolve(h, false));
    const TableView tv = table_view(h);

    // ---- X1: A + the slots (every owner's segment budgeted, this shard's own included) ----
    SlotSegs x;
    rc = f.exchange_slots(true, x, [&](int phases, const SlotLayout& L) {
        if (phases == 1)
            return launch_budget_slots(h, in.pos, in.keys, in.world, in.sender, in.repl, M, G, G, L, nullptr, nullptr,
                                       f.a_send, 1, false, true);
        // the self segment straight into the receive buffer (not through the exchange's self copy), except
        // with the caller's callback, which copies every segment itself
        const bool in_place = x.self_in_place = sc.kind != kXCallback;
        // ... and its A entry too, on a budgeted tick (the one-pass grouping's last block writes it)
        x.a_in_place = in_place && !exact && M && !f.late && !getenv("WQ_DEBUG_SLOT_3PASS");
        uint32_t* a_self = x.a_in_place ? f.a_recv + 2 * me : nullptr;
        return launch_budget_slots(h, in.pos, in.keys, in.world, in.sender, in.repl, M, G, in_place ? me : G, L,
                                   sc.slots.as<uint32_t>(), sc.perm.as<uint32_t>(), f.a_send, phases, false, true,
                                   in_place ? sc.rslots.as<uint32_t>() + (uint64_t)kSlotWords * x.rb.b[me] : nullptr,
                                   in_place ? sc.perm.as<uint32_t>() + L.base[me] : nullptr, nullptr, !exact,
                                   in_place ? L.budget[me] : 0xFFFFFFFFu, a_self);
    });
    if (rc) return rc;
    const uint64_t Rb = x.Rb;
    sc.last_sent = sc.last_recv = 0;
    for (uint32_t d = 0; d < G; ++d)
        if (d != me) {
            sc.last_sent += 8 + (uint64_t)sc.b1_out[d] * kSlotWords * 4;
            sc.last_recv += 8 + (uint64_t)sc.b1_in[d] * kSlotWords * 4;
        }

    // ---- the owner: count the received slots, the tile scan, the emit; the pairs stay here ----
    if (inject == 3) f.fail(set_error(h, WQ_E_INVALID, "injected failure at step 3 (test hook)"));
    RouteWs& rw = h->rws;
    const uint32_t nto = (uint32_t)(Rb / kBlock);  // whole blocks
    if (!sc.own_cap) sc.own_cap = std::min<uint64_t>(8 * Rb + 4096, 0xFFFFFFFFull);
    if (!f.late && !f.fail(f.alloc(rw.e, (Rb + 1) * 4)) && !f.fail(f.alloc(rw.info, (Rb + 1) * 8)) &&
        !f.fail(f.alloc(sc.otiles, ((uint64_t)nto * 3 + 4) * 4)) && !f.fail(f.alloc(sc.own_off, (Rb + 1) * 4)))
        f.fail(f.alloc(sc.own_peers, sc.own_cap * 4));
    // the asynchronous end's snapshot (below), taken by the tile scan when one block runs it; every
    // segment is budgeted, this shard's own included, so the statuses count at G = 1 too
    const bool async_end = async && !exact;
    const AsyncResultParams ar = async_end ? f.async_params(true, Rb != 0, sc.own_cap, d_result) : AsyncResultParams{};
    bool ar_done = false;
    if (!f.late && Rb) {
        const CountParams cp = f.count_params(tv, f.slots_in(sc.rslots.as<uint32_t>(), (uint32_t)Rb), rw.e.as<uint32_t>(),
                                              rw.info.as<uint2>(), sc.otiles.as<uint32_t>(), nto, nto, kCntOwner);
        hipLaunchKernelGGL((count_kernel<false, 1, 8, 0, false, true>), dim3(pass_blocks(nto)), dim3(kBlock), 0, s, cp);
        if (hipGetLastError() != hipSuccess) f.fail(set_error(h, WQ_E_HIP, "count launch (owner form)"));
        if (!f.late) f.fail(owner_emit(h, Rb, tv, async_end ? &ar : nullptr, &ar_done));
    }

    auto fill_view = [&](uint64_t P) {
        out->slots = sc.rslots.as<uint32_t>();
        out->offsets = sc.own_off.as<uint32_t>();
        out->peers = sc.own_peers.as<uint32_t>();
        out->send_perm = sc.perm.as<uint32_t>();
        out->n_slots = Rb;
        out->n_pairs = P;
        for (uint32_t d = 0; d <= G; ++d) {
            out->seg[d] = x.rb.b[d];
            out->send_seg[d] = x.sb.b[d];
        }
    };
    // ---- asynchronous end (a budgeted tick): as the slot tick's; a pair buffer that was short
    // shows as overflow, and is grown when the snapshot is folded in (async_drain) ----
    if (async_end) {
        if (!Rb && !f.late) WQ_HIP(h, hipMemsetAsync(sc.own_off.p, 0, 4, s));
        if ((rc = f.finish_async(ar, ar_done))) return rc;
        fill_view(~0ull);  // P: in the caller's counters
        return WQ_OK;
    }

    // ---- the one host read ----
    const wq_route_counters* hcnt;
    if ((rc = f.read_back(true, redo, &hcnt)) || *redo) return rc;
    const uint32_t err = Rb ? (hcnt[kCntScan].error | hcnt[kCntOwner].error) : 0u;
    if (err) return status_error(h, (uint64_t)err << 32, me);
    const uint64_t P = Rb ? hcnt[kCntScan].n_pairs : 0;
    if (P > sc.own_cap) {  // the pair buffers were short: grow them and emit again (the rows are kept)
        sc.own_cap = std::min<uint64_t>(P + P / 4 + 4096, 0xFFFFFFFFull);
        if (f.alloc(sc.own_peers, sc.own_cap * 4)) return WQ_E_OOM;
        if ((rc = owner_emit(h, Rb, tv))) return rc;
        WQ_HIP(h, hipStreamSynchronize(s));
    }
    if (!Rb) WQ_HIP(h, hipMemsetAsync(sc.own_off.p, 0, 4, s));
    fill_view(P);
    return WQ_OK;
}

int owner_slots_call(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                     const uint32_t* d_sender, const uint8_t* d_repl, size_t n_msgs, wq_owner_slot_view* out, bool async,
                     wq_route_counters* d_result) {
    if (int rc = begin_owner_tick(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs, out)) return rc;
    const TickIn in{d_pos, d_keys, d_world, d_sender, d_repl, n_msgs};
    const int rc = budgeted_call(h, 1, async, [&](bool exact, int inject, bool* redo, bool as) {
        return owner_slot_tick(h, in, exact, inject, redo, out, as, d_result);
    });
    if (async && d_result && rc == WQ_OK && out->n_pairs != ~0ull) {
        wq_route_counters c{};
        c.n_pairs = out->n_pairs;
        if (int e = put_result(h, d_result, c)) return e;
    }
    return rc;
}

}  // namespace

int sharded_tick_slots(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                       const uint32_t* d_sender, const uint8_t* d_repl, size_t M, uint32_t* d_offsets,
                       uint32_t* d_peers, uint32_t* d_msgs, size_t capacity, size_t* n_pairs, bool async,
                       wq_route_counters* d_result) {
    const TickIn in{d_pos, d_keys, d_world, d_sender, d_repl, M};
    const CsrOut out{d_offsets, d_peers, d_msgs, capacity};
    const int rc = budgeted_call(h, 0, async, [&](bool exact, int inject, bool* redo, bool as) {
        return SlotTick(h, in, exact, inject).run(out, n_pairs, redo, as, d_result);
    });
    if (async && d_result && (rc == WQ_OK || rc == WQ_E_CAPACITY) && h->shard->last_ready) {
        wq_route_counters c{};
        c.n_pairs = *n_pairs;
        c.overflow = *n_pairs > capacity ? 1u : 0u;
        if (int e = put_result(h, d_result, c)) return e;
    }
    return rc;
}

}  // namespace wq

using namespace wq;

extern "C" {

int wq_sharded_route_tick_async(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                                const uint32_t* d_sender, const uint8_t* d_repl, size_t n_msgs, uint32_t* d_offsets,
                                uint32_t* d_peers, uint32_t* d_msgs, size_t capacity, wq_route_counters* d_counters) {
    if (int rc = check_csr_tick(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs, d_offsets, d_peers, capacity))
        return rc;
    if (!h->shard || h->shard_expanded)
        return set_error(h, WQ_E_INVALID, "wq_sharded_route_tick_async: no exchange attached, or the expanded form");
    WQ_HIP(h, hipSetDevice(h->device));
    if (capacity > 0xFFFFFFFFull) capacity = 0xFFFFFFFFull;
    size_t P = 0;
    return sharded_tick_slots(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs, d_offsets, d_peers, d_msgs, capacity,
                              &P, true, d_counters);
}

int wq_sharded_route_owner_slots(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                                 const uint32_t* d_sender, const uint8_t* d_repl, size_t n_msgs,
                                 wq_owner_slot_view* out) {
    return owner_slots_call(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs, out, false, nullptr);
}

int wq_sharded_route_owner_slots_async(wq_router* h, const double* d_pos, const int64_t* d_keys,
                                       const uint32_t* d_world, const uint32_t* d_sender, const uint8_t* d_repl,
                                       size_t n_msgs, wq_route_counters* d_counters, wq_owner_slot_view* out) {
    return owner_slots_call(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs, out, true, d_counters);
}

}  // extern "C"
