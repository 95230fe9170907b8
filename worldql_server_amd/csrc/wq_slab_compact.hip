// wq_slab_compact.hip — the record payload slab rewritten in its canonical form: live payloads back to back
// in handle order, dead entries zeroed (wq_slab_compact_device). Into a second arena it is compaction, into a
// buffer the host reads it is an export, from an uploaded file it is a validated import. An extension the
// reference does not have: its records live in PostgreSQL (database/client.rs). All arithmetic is
// compact_ops.hpp.
//
//   size     four lanes per source entry, each with one 16-byte chunk of it: lane 3 takes the bits from lane
//            2 and writes the entry's term (live, size under the range rule); a wave walks 16 chunks a lane
//            and ends with one atomic max of its highest live handle and one OR of its error bits
//   scan     one exclusive scan of (live, size) over the handles: K, the rank among the live, and E, the byte
//   decide   one lane: the total, the two overflow bits, the cursor, the counters. The passes behind it return
//            at once after an overflow: all or nothing
//   entries  four lanes per destination entry: aligned 16-byte stores of the moved entry or of zeros over all
//            of dst->n_entries; lane 3 of a kept entry also writes its element of the dense list
//   copy     over the destination bytes [0, total) in the send buffers' shape (wq_pack.hip): a wave owns a
//            1 KiB tile and a lane one 16-byte chunk. The elements are the dense list of live entries, so dead
//            handles are never walked. A tile inside one payload is 64 unaligned 16-byte loads and 64 aligned
//            stores; otherwise the tile's elements go through LDS 64 at a time
//
// No lane, wave or block owns an entry or a payload. Placement comes from the scan alone; the only atomics
// are a max and an OR into the control block.
#include "compact_ops.hpp"
#include "send_rows.hpp"

namespace wq {

namespace {

static_assert(sizeof(wq_slab_compact_counters) == 40, "abi.SLAB_COMPACT_COUNTERS_DTYPE mirrors this layout");
static_assert(sizeof(wq_slab_entry) == kCmpQuad * sizeof(CmpChunk), "an entry is four chunks");
static_assert(kCmpOverArena == 1u && kCmpOverEntries == 2u && kCmpErrRange == 1u, "the header's bits");
static_assert(kBlock % 64 == 0 && 64 % kCmpQuad == 0, "a quad lies inside one wave");

struct CmpWs {
    uint64_t* term;  // [n] per source handle
    CmpKE* KE;       // [n + 1]
    uint64_t* dE;    // [n + 1] the dense list: where each live entry's payload goes, then the total
    uint64_t* dS;    // [n] and where it lies in the source arena
    CmpCtrl* ctrl;
};

struct CmpTerm {
    const uint64_t* term;
    uint64_t n;
    __host__ __device__ __forceinline__ CmpKE operator()(uint64_t i) const { return cmp_ke(term, n, i); }
};

// Chunks a lane of the size pass walks, kBlock apart: a wave keeps its highest live handle and its error
// bits in registers and ends with one atomic each, 1 per kCmpRun * 16 entries, so the one word every wave
// raises does not serialize the pass.
constexpr uint32_t kCmpRun = 16;

__global__ __launch_bounds__(kBlock) void k_cmp_size(wq_slab_view src, CmpWs ws) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t top = 0;
    bool any_bad = false;
    for (uint32_t it = 0; it < kCmpRun; ++it) {
        const uint64_t t = ((uint64_t)blockIdx.x * kCmpRun + it) * kBlock + threadIdx.x;
        const uint64_t i = t / kCmpQuad;
        const uint32_t c = (uint32_t)(t % kCmpQuad);
        const bool in = i < src.n_entries;
        CmpChunk v{0u, 0u, 0u, 0u};
        if (in) v = reinterpret_cast<const CmpChunk*>(src.entries)[t];
        const uint32_t bits = (uint32_t)__shfl((int)v.w, (int)((lane & ~3u) | 2u));  // chunk 2 ends with the bits
        uint32_t err = 0;
        bool live = false;
        if (in && c == 3) {
            const uint64_t term = cmp_term(bits, cmp_chunk_off(v), v.z, v.w, src.n_payload_bytes, &err);
            ws.term[i] = term;
            live = cmp_live(term);
        }
        const uint64_t m = __ballot(live);
        any_bad |= __ballot(err != 0) != 0;
        // the wave's highest live handle so far: lane l holds handle (t - lane + l) / 4, and t ascends with `it`
        if (m) top = (t - lane + (63u - (uint32_t)__clzll(m))) / kCmpQuad + 1ull;
    }
    if (lane == 0) {
        if (top) atomicMax(reinterpret_cast<unsigned long long*>(&ws.ctrl->max_need), (unsigned long long)top);
        if (any_bad) atomicOr(&ws.ctrl->error, kCmpErrRange);
    }
}

__global__ void k_cmp_decide(CmpWs ws, uint64_t n, wq_slab_view dst, uint64_t* cursor, wq_slab_compact_counters* counters) {
    const CmpKE sum = ws.KE[n];
    const uint32_t over = cmp_decide(sum.e, ws.ctrl->max_need, dst);
    ws.ctrl->overflow = over;
    ws.ctrl->n_live = sum.k;
    ws.dE[sum.k] = sum.e;
    if (!over) *cursor = sum.e;
    if (counters) {
        wq_slab_compact_counters c;
        c.n_entries = n;
        c.n_live = sum.k;
        c.bytes_live = sum.e;
        c.entries_need = ws.ctrl->max_need;
        c.overflow = over;
        c.error = ws.ctrl->error;
        *counters = c;
    }
}

__global__ __launch_bounds__(kBlock) void k_cmp_entries(wq_slab_view src, wq_slab_view dst, CmpWs ws) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i = t / kCmpQuad;
    const uint32_t c = (uint32_t)(t % kCmpQuad);
    if (i >= dst.n_entries || ws.ctrl->overflow) return;
    const uint64_t term = i < src.n_entries ? ws.term[i] : 0ull;
    const bool kept = cmp_live(term);
    CmpChunk v{0u, 0u, 0u, 0u};
    CmpKE at{0ull, 0ull};
    if (kept) {
        v = reinterpret_cast<const CmpChunk*>(src.entries)[t];
        if (c == 3) {
            at = ws.KE[i];
            ws.dE[at.k] = at.e;
            ws.dS[at.k] = cmp_size(term) ? cmp_chunk_off(v) : 0ull;
        }
    }
    reinterpret_cast<CmpChunk*>(dst.entries)[t] = cmp_entry_chunk(c, v, kept, term, at.e);
}

// One wave per block; the blocks share the result's tiles in consecutive runs, so only a block's first
// tile searches all of dE. Everything that decides a branch around a barrier is the same in all 64 lanes
// (the tile, its first element, the window).
__global__ __launch_bounds__(kPackLanes) void k_cmp_copy(const uint8_t* __restrict__ in, uint64_t n_in_bytes, CmpWs ws,
                                                         uint8_t* __restrict__ out) {
    __shared__ uint64_t W[kPackWindow + 1];
    __shared__ uint64_t S[kPackWindow];
    if (ws.ctrl->overflow) return;
    const uint32_t T = (uint32_t)ws.ctrl->n_live;
    const uint64_t total = ws.dE[T];
    const uint64_t tiles = cmp_tiles(total);
    const uint64_t per = pack_tiles_per_block(total, gridDim.x);
    const uint32_t lane = threadIdx.x;
    uint32_t e0 = 0;
    for (uint64_t i = 0; i < per; ++i) {
        const uint64_t ti = blockIdx.x * per + i;
        if (ti >= tiles) break;
        const uint64_t c0 = ti * kPackTile, c1 = c0 + kPackTile < total ? c0 + kPackTile : total;
        const uint64_t d0 = c0 + (uint64_t)lane * kPackChunk;
        const uint64_t hi = d0 + kPackChunk < c1 ? d0 + kPackChunk : c1;
        e0 = i ? pack_elem_from(ws.dE, T, e0, c0) : pack_elem_of(ws.dE, T, c0);
        const uint64_t r0 = ws.dE[e0], r1 = ws.dE[e0 + 1];
        if (pack_tile_inside(r0, r1, 0, c0, c1)) {
            pack_store(out, d0, kPackChunk, pack_load16(in + ws.dS[e0] + (d0 - r0)));
            continue;
        }
        PackChunk v{0ull, 0ull};
        for (uint64_t wb = e0;; wb += kPackWindow) {
            __syncthreads();  // the window before this one has been read
            W[lane] = pack_win_entry(ws.dE, T, wb, lane);
            if (lane == 0) W[kPackWindow] = pack_win_entry(ws.dE, T, wb, kPackWindow);
            S[lane] = wb + lane < T ? ws.dS[wb + lane] : 0ull;
            __syncthreads();
            const uint64_t w0 = W[0], w1 = W[kPackWindow];
            const uint64_t a = d0 > w0 ? d0 : w0, b = hi < w1 ? hi : w1;
            if (a < b) pack_compose(W, S, in, n_in_bytes, 0, d0, a, b, &v);
            if (w1 >= c1) {
                e0 = (uint32_t)wb + pack_win_find(W, c1 - 1);  // the element of the tile's last byte
                break;
            }
        }
        if (d0 < hi) pack_store(out, d0, (uint32_t)(hi - d0), v);
    }
}

}  // namespace

void slab_compact_release(wq_router* h) {
    h->cmp_ws.release();
    h->cmp_ctrl.release();
}

// The call on device arrays (the handle's device is current; arguments validated, n_entries < 2^32 - 1).
int launch_slab_compact(wq_router* h, const wq_slab_view* src, const wq_slab_view* dst, uint64_t* d_dst_cursor,
                        wq_slab_compact_counters* d_counters) {
    hipStream_t s = h->stream;
    const size_t n = src->n_entries;
    // one buffer: KE (16-byte pairs), then term, dE, dS (8-byte words)
    WQ_ALLOC(h, h->cmp_ws, (n + 1) * 16 + n * 8 + (n + 1) * 8 + n * 8);
    WQ_ALLOC(h, h->cmp_ctrl, sizeof(CmpCtrl));
    WQ_HIP(h, hipMemsetAsync(h->cmp_ctrl.p, 0, sizeof(CmpCtrl), s));
    CmpKE* KE = h->cmp_ws.as<CmpKE>();
    uint64_t* w = reinterpret_cast<uint64_t*>(KE + n + 1);
    const CmpWs ws{w, KE, w + n, w + 2 * n + 1, h->cmp_ctrl.as<CmpCtrl>()};
    if (n) {
        const uint64_t per_block = (uint64_t)kBlock * kCmpRun;
        hipLaunchKernelGGL(k_cmp_size, dim3((unsigned)(((uint64_t)n * kCmpQuad + per_block - 1) / per_block)), dim3(kBlock), 0, s, *src, ws);
        WQ_HIP(h, hipGetLastError());
    }
    if (int rc = scan_terms(h, CmpTerm{ws.term, (uint64_t)n}, ws.KE, CmpKE{0ull, 0ull}, n + 1, CmpPlus())) return rc;
    hipLaunchKernelGGL(k_cmp_decide, dim3(1), dim3(1), 0, s, ws, (uint64_t)n, *dst, d_dst_cursor, d_counters);
    WQ_HIP(h, hipGetLastError());
    if (dst->n_entries) {
        hipLaunchKernelGGL(k_cmp_entries, dim3(grid_for((uint64_t)dst->n_entries * kCmpQuad)), dim3(kBlock), 0, s, *src, *dst, ws);
        WQ_HIP(h, hipGetLastError());
    }
    if (n && dst->n_payload_bytes) {
        const unsigned blocks = (unsigned)pack_blocks(dst->n_payload_bytes);
        hipLaunchKernelGGL(k_cmp_copy, dim3(blocks), dim3(kPackLanes), 0, s, (const uint8_t*)src->payload, src->n_payload_bytes, ws,
                           dst->payload);
        WQ_HIP(h, hipGetLastError());
    }
    return WQ_OK;
}

}  // namespace wq
