// wq_slab.hip — the record payload slab: a tick's created records copied from its frames into device memory.
//
// wq_records_dispatch_device leaves an op and an op_ref per accepted create; the host used to read both
// back and slice the frame bytes into one Python dict per record. Here the payloads go from the frames
// where the decoder read them into the caller's arena, and one 64-byte entry per handle says where they
// lie. An extension the reference does not have: its records live in PostgreSQL (database/client.rs).
// All arithmetic is slab_ops.hpp.
//
//   size     one lane per op: its two elements (data, flex) under the validity rules, their sizes and where
//            they start in the frame bytes; the largest create handle by an atomic max
//   scan     one u64 exclusive scan of the element sizes: E
//   decide   one lane: the cursor, the total and the two overflow bits; advances the cursor when the call
//            fits; the counters. The passes behind it return at once after an overflow: all or nothing
//   entries  one lane per op: the entry of a create at its handle
//   copy     over the arena bytes [cursor, cursor + total) in the send buffers' shape (wq_pack.hip): a wave
//            owns a 1 KiB-aligned tile of the arena and a lane one 16-byte chunk. A tile inside one payload
//            is 64 unaligned 16-byte loads and 64 aligned stores; otherwise the tile's elements go through
//            LDS 64 at a time and every lane composes its chunk from the one or more elements that touch it
//
// No lane, wave or block owns an op or a payload. Placement comes from the scan alone; the only atomics
// are a max, an add and ORs into the control block, so the slab is the same bytes every time.
#include "slab_ops.hpp"
#include "send_rows.hpp"

namespace wq {

namespace {

static_assert(sizeof(wq_slab_entry) == 64, "abi.SLAB_ENTRY_DTYPE mirrors this layout");
static_assert(sizeof(wq_slab_view) == 32, "abi.SlabView mirrors this layout");
static_assert(sizeof(wq_slab_counters) == 56, "abi.SLAB_COUNTERS_DTYPE mirrors this layout");
static_assert(kSlabOverArena == 1u && kSlabOverEntries == 2u, "the header's overflow bits");

struct SlabWs {
    uint32_t* size;  // [2 n_ops] element sizes
    uint64_t* src;   // [2 n_ops] where each element starts in the frame bytes
    uint64_t* E;     // [2 n_ops + 1]
    SlabCtrl* ctrl;
};

struct SlabTerm {
    const uint32_t* size;
    uint64_t T;
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t k) const { return slab_term(size, T, k); }
};

__global__ __launch_bounds__(kBlock) void k_slab_size(SlabIn in, SlabWs ws) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool create = false;
    if (q < in.n_ops) {
        const SlabParts p = slab_parts(in, q);
        create = p.create;
        ws.size[2 * q] = p.len[0];
        ws.size[2 * q + 1] = p.len[1];
        ws.src[2 * q] = p.src[0];
        ws.src[2 * q + 1] = p.src[1];
        if (p.err) atomicOr(&ws.ctrl->error, p.err);
        if (create)
            atomicMax(reinterpret_cast<unsigned long long*>(&ws.ctrl->max_need),
                      (unsigned long long)in.ops[q].handle + 1ull);
    }
    const uint64_t m = __ballot(create);
    if ((threadIdx.x & 63u) == 0 && m)
        atomicAdd(reinterpret_cast<unsigned long long*>(&ws.ctrl->n_creates), (unsigned long long)__popcll(m));
}

__global__ void k_slab_decide(SlabWs ws, uint64_t n_ops, wq_slab_view v, uint64_t* cursor, wq_slab_counters* counters) {
    const uint64_t base = *cursor, total = ws.E[2 * n_ops];
    const uint32_t over = slab_decide(base, total, ws.ctrl->max_need, v);
    ws.ctrl->base = base;
    ws.ctrl->overflow = over;
    if (!over) *cursor = base + total;
    if (counters) {
        wq_slab_counters c;
        c.n_ops = n_ops;
        c.n_creates = ws.ctrl->n_creates;
        c.bytes_stored = total;
        c.bytes_need = total > ~0ull - base ? ~0ull : base + total;  // saturates with an absurd cursor
        c.entries_need = ws.ctrl->max_need;
        c.cursor = over ? base : base + total;
        c.overflow = over;
        c.error = ws.ctrl->error;
        *counters = c;
    }
}

__global__ __launch_bounds__(kBlock) void k_slab_entries(SlabIn in, SlabWs ws, wq_slab_view v) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= in.n_ops || ws.ctrl->overflow) return;
    if (in.ops[q].kind != WQ_RECORD_CREATE) return;
    // the decision has seen every create's handle below n_entries
    v.entries[in.ops[q].handle] = slab_entry(in, q, ws.ctrl->base + ws.E[2 * q], ws.size[2 * q], ws.size[2 * q + 1]);
}

// One wave per block; the blocks share the call's tiles in consecutive runs, so only a block's first
// tile searches all of E. Everything that decides a branch around a barrier is the same in all 64
// lanes (the tile, its first element, the window).
__global__ __launch_bounds__(kPackLanes) void k_slab_copy(SlabIn in, SlabWs ws, uint8_t* __restrict__ out) {
    __shared__ uint64_t W[kPackWindow + 1];
    __shared__ uint64_t S[kPackWindow];
    if (ws.ctrl->overflow) return;
    const uint32_t T = (uint32_t)(2 * in.n_ops);
    const uint64_t base = ws.ctrl->base, total = ws.E[T], end = base + total;
    const uint64_t tiles = slab_tiles(base, total);
    const uint64_t per = slab_tiles_per_block(tiles, gridDim.x);
    const uint64_t n_frame_bytes = slab_frame_bytes(in);
    const uint32_t lane = threadIdx.x;
    uint32_t e0 = 0;
    for (uint64_t i = 0; i < per; ++i) {
        const uint64_t ti = blockIdx.x * per + i;
        if (ti >= tiles) break;
        const uint64_t a0 = slab_tile0(base) + ti * kPackTile;
        const uint64_t c0 = a0 > base ? a0 : base, c1 = a0 + kPackTile < end ? a0 + kPackTile : end;
        const uint64_t d0 = a0 + (uint64_t)lane * kPackChunk;
        const uint64_t lo = d0 > c0 ? d0 : c0, hi = d0 + kPackChunk < c1 ? d0 + kPackChunk : c1;
        e0 = i ? pack_elem_from(ws.E, T, e0, c0 - base) : pack_elem_of(ws.E, T, c0 - base);
        const uint64_t r0 = base + ws.E[e0], r1 = base + ws.E[e0 + 1];
        if (pack_tile_inside(r0, r1, 0, c0, c1)) {
            pack_store(out, d0, kPackChunk, pack_load16(in.frames + ws.src[e0] + (d0 - r0)));
            continue;
        }
        PackChunk v{0ull, 0ull};
        for (uint64_t wb = e0;; wb += kPackWindow) {
            __syncthreads();  // the window before this one has been read
            W[lane] = base + pack_win_entry(ws.E, T, wb, lane);
            if (lane == 0) W[kPackWindow] = base + pack_win_entry(ws.E, T, wb, kPackWindow);
            S[lane] = wb + lane < T ? ws.src[wb + lane] : 0ull;
            __syncthreads();
            const uint64_t w0 = W[0], w1 = W[kPackWindow];
            const uint64_t a = lo > w0 ? lo : w0, b = hi < w1 ? hi : w1;
            if (a < b) pack_compose(W, S, in.frames, n_frame_bytes, 0, d0, a, b, &v);
            if (w1 >= c1) {
                e0 = (uint32_t)wb + pack_win_find(W, c1 - 1);  // the element of the tile's last byte
                break;
            }
        }
        if (lo < hi) slab_store(out, d0, lo, hi, v);
    }
}

}  // namespace

void slab_release(wq_router* h) {
    h->slab_ws.release();
    h->slab_ctrl.release();
}

// The call on device arrays (the handle's device is current; arguments validated, n_ops < 2^31).
int launch_slab_store(wq_router* h, const wq_rec_op* d_ops, const wq_rec_op_ref* d_op_ref, size_t n_ops,
                      const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n_frames, const wq_slab_view* view,
                      uint64_t* d_cursor, wq_slab_counters* d_counters) {
    hipStream_t s = h->stream;
    const size_t T = 2 * n_ops;
    // one buffer: E, src (8-byte words), then the sizes
    WQ_ALLOC(h, h->slab_ws, (T + 1) * 8 + T * 8 + T * 4);
    WQ_ALLOC(h, h->slab_ctrl, sizeof(SlabCtrl));
    WQ_HIP(h, hipMemsetAsync(h->slab_ctrl.p, 0, sizeof(SlabCtrl), s));
    uint64_t* E = h->slab_ws.as<uint64_t>();
    const SlabWs ws{reinterpret_cast<uint32_t*>(E + 2 * T + 1), E + T + 1, E, h->slab_ctrl.as<SlabCtrl>()};
    const SlabIn in{d_ops, d_op_ref, d_frames, d_frame_offsets, (uint64_t)n_ops, (uint64_t)n_frames};
    if (n_ops) {
        hipLaunchKernelGGL(k_slab_size, dim3(grid_for(n_ops)), dim3(kBlock), 0, s, in, ws);
        WQ_HIP(h, hipGetLastError());
    }
    if (int rc = scan_terms(h, SlabTerm{ws.size, (uint64_t)T}, ws.E, T + 1)) return rc;
    hipLaunchKernelGGL(k_slab_decide, dim3(1), dim3(1), 0, s, ws, (uint64_t)n_ops, *view, d_cursor, d_counters);
    WQ_HIP(h, hipGetLastError());
    if (n_ops && view->n_entries) {
        hipLaunchKernelGGL(k_slab_entries, dim3(grid_for(n_ops)), dim3(kBlock), 0, s, in, ws, *view);
        WQ_HIP(h, hipGetLastError());
    }
    if (n_ops && view->n_payload_bytes) {
        const unsigned blocks = (unsigned)slab_blocks(view->n_payload_bytes);
        hipLaunchKernelGGL(k_slab_copy, dim3(blocks), dim3(kPackLanes), 0, s, in, ws, view->payload);
        WQ_HIP(h, hipGetLastError());
    }
    return WQ_OK;
}

}  // namespace wq
