// wq_reply.hip — the record reply builder: frames of messages that carry records, read from the payload slab.
//
// wq_records_read_device leaves a CSR of payload handles; the replies used to be gathered as Python dicts and
// serialized on the host. Here the frames are written on the device, ready for the byte budget and the pack,
// as wq_frames.hip writes flat ones. All arithmetic is reply_ops.hpp.
//
//   rows    the send side's ordinal space over the CSR (send_rows.hpp): pre
//   term    one lane per ordinal: its row (a search over pre), its entry under the validity rules, the
//           segmented scan's term
//   scan    the exclusive segmented scan of the terms: per ordinal the shapes its row has seen before it and
//           whether the last kept record left the fill at 2 mod 4
//   place   one lane per ordinal: the record's size from that state; a shape's first occurrence registers
//           itself in first[8 row + shape]
//   scans   the u64 prefix sums of the sizes (P) and of the kept flags (K)
//   size    one lane per message: the frame's size from its row's bytes and count; the 2^30 rule
//   scan    the u64 exclusive scan of the frame sizes into the caller's d_frame_offsets: E
//   copy    wq_frames.hip's copy with the reply's composer: per 16-byte chunk the message walk, the one or two
//           records whose bytes touch it (a search over P) and the offsets-vector slots inside it (a search
//           over K each). A tile inside one payload, a message's or a record's, is 64 loads and 64 stores.
//
// No lane, wave or block owns a row or a payload. Placement comes from the scans alone; `first` has one writer
// per entry; the only atomics are ORs into the error word.
#include "reply_ops.hpp"
#include "send_rows.hpp"

namespace wq {

namespace {

static_assert(sizeof(wq_frames_rec_src) == 96, "abi.FramesRecSrc mirrors this layout");
static_assert(kRpSkipEmpty == WQ_FRAMES_SKIP_EMPTY, "the header's flag");

struct RpScanTerm {
    const uint32_t* term;
    const uint32_t* T;
    __host__ __device__ __forceinline__ uint32_t operator()(uint64_t q) const { return q < *T ? term[q] : kRpHead; }
};
struct RpSizeTerm {
    const uint32_t* sz;
    const uint32_t* T;
    bool count;
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t q) const {
        return q < *T ? (count ? (uint64_t)(sz[q] != 0) : (uint64_t)sz[q]) : 0ull;
    }
};
struct RpFrameTerm {
    const uint32_t* size;
    uint64_t n;
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t q) const { return frame_term(size, n, q); }
};

__global__ __launch_bounds__(kBlock) void k_reply_term(ReplyCtx c, uint32_t* __restrict__ ctrl) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n = (uint32_t)c.s.n;
    if (q >= c.pre[n]) return;
    uint32_t err = 0;
    c.term[q] = reply_term(c, bud_row_of(c.pre, n, (uint32_t)q), (uint32_t)q, &err);
    if (err) atomicOr(&ctrl[1], err);
}

__global__ __launch_bounds__(kBlock) void k_reply_place(ReplyCtx c) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n = (uint32_t)c.s.n;
    if (q >= c.pre[n]) return;
    c.sz[q] = reply_place(c, bud_row_of(c.pre, n, (uint32_t)q), (uint32_t)q);
}

__global__ __launch_bounds__(kBlock) void k_reply_size(ReplyCtx c, uint32_t* __restrict__ size, uint32_t* __restrict__ out_size,
                                                       uint32_t* __restrict__ ctrl) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.s.n) return;
    uint32_t err = 0;
    const uint32_t s = reply_size(c, i, &err);
    size[i] = s;
    if (out_size) out_size[i] = s;
    if (err) atomicOr(&ctrl[1], err);
}

// wq_frames.hip's copy: one wave per block, consecutive runs of tiles, barrier branches wave-uniform.
__global__ __launch_bounds__(kPackLanes) void k_reply_copy(ReplyCtx c, const uint64_t* __restrict__ E,
                                                           uint8_t* __restrict__ out, uint64_t capacity) {
    __shared__ uint64_t W[kPackWindow + 1];
    const uint32_t T = (uint32_t)c.s.n;
    const uint64_t need = E[T];
    const uint64_t written = need < capacity ? need : capacity;
    const uint32_t lane = threadIdx.x;
    const uint64_t per = pack_tiles_per_block(written, gridDim.x);
    uint32_t e0 = 0;
    for (uint64_t i = 0; i < per; ++i) {
        const uint64_t c0 = (blockIdx.x * per + i) * kPackTile;
        if (c0 >= written) break;
        const uint64_t c1 = written - c0 > kPackTile ? c0 + kPackTile : written;
        const uint64_t d0 = c0 + (uint64_t)lane * kPackChunk;
        const uint64_t d1 = d0 >= c1 ? d0 : (c1 - d0 > kPackChunk ? d0 + kPackChunk : c1);
        e0 = i ? pack_elem_from(E, T, e0, c0) : pack_elem_of(E, T, c0);
        const uint64_t r0 = E[e0], r1 = E[e0 + 1];
        if (c1 - c0 == kPackTile && r1 - r0 >= kPackTile) {
            const uint8_t* from;
            if (reply_tile_inside(c, e0, r0, r1, c0, c1, &from)) {
                pack_store(out, d0, kPackChunk, pack_load16(from + (uint64_t)lane * kPackChunk));
                continue;
            }
        }
        PackChunk v{0ull, 0ull};
        for (uint64_t wb = e0;; wb += kPackWindow) {
            __syncthreads();  // the window before this one has been read
            W[lane] = pack_win_entry(E, T, wb, lane);
            if (lane == 0) W[kPackWindow] = pack_win_entry(E, T, wb, kPackWindow);
            __syncthreads();
            const uint64_t w0 = W[0], w1 = W[kPackWindow];
            const uint64_t lo = d0 > w0 ? d0 : w0, hi = d1 < w1 ? d1 : w1;
            if (lo < hi) reply_compose(W, wb, c, d0, lo, hi, &v);
            if (w1 >= c1) {
                e0 = (uint32_t)wb + pack_win_find(W, c1 - 1);
                break;
            }
        }
        if (d0 < d1) pack_store(out, d0, (uint32_t)(d1 - d0), v);
    }
}

__global__ void k_reply_counters(const uint64_t* __restrict__ E, uint64_t n, uint64_t capacity, const uint32_t* __restrict__ ctrl,
                                 wq_frames_counters* counters) {
    const uint64_t need = E[n];
    wq_frames_counters c;
    c.n_frames = n;
    c.n_complete = pack_elem_of(E, (uint32_t)n, capacity);
    c.bytes_need = need;
    c.bytes_written = need < capacity ? need : capacity;
    c.overflow = need > capacity ? 1u : 0u;
    c.error = ctrl[1];
    *counters = c;
}

size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

void reply_release(wq_router* h) { h->rp_ws.release(); }

// The call on device arrays (the handle's device is current; arguments validated, n_msgs and n_handles < 2^32 - 1).
int launch_frames_build_records(wq_router* h, const wq_frames_src* src, const wq_frames_rec_src* rec, size_t n_msgs,
                                uint8_t* d_frames, size_t capacity_bytes, uint64_t* d_frame_offsets, uint32_t* d_frame_size,
                                wq_frames_counters* d_counters) {
    hipStream_t s = h->stream;
    const size_t nh = rec->n_handles, rows = n_msgs + 1;
    if (int rc = rows_alloc(h, rows)) return rc;
    WQ_ALLOC(h, h->frm_size, n_msgs * 4);
    WQ_ALLOC(h, h->frm_ctrl, 64);
    // one buffer: P, K (u64), then X, term, sz, first (u32)
    const size_t o_p = 0, o_k = o_p + (nh + 1) * 8, o_x = o_k + (nh + 1) * 8, o_t = o_x + up8((nh + 1) * 4),
                 o_sz = o_t + up8((nh + 1) * 4), o_first = o_sz + up8((nh + 1) * 4), total = o_first + 32 * rows;
    WQ_ALLOC(h, h->rp_ws, total);
    WQ_HIP(h, hipMemsetAsync(h->frm_ctrl.p, 0, 64, s));
    uint8_t* p = h->rp_ws.as<uint8_t>();
    auto u8 = [](const void* q) { return static_cast<const uint8_t*>(q); };

    ReplyCtx c;
    FrameSrc& in = c.s;
    in.instruction = src->instruction;
    in.replication = src->replication;
    in.sender_uuid = src->sender_uuid;
    in.world = u8(src->world);
    in.pos = u8(src->pos);
    in.param = src->param;
    in.param_offsets = u8(src->param_offsets);
    in.flex = src->flex;
    in.flex_offsets = u8(src->flex_offsets);
    in.msg_flags = src->msg_flags;
    in.world_bytes = h->frm_n_worlds ? h->frm_world_bytes.as<uint8_t>() + kFrWorldSlack : nullptr;
    in.world_slack = kFrWorldSlack;
    in.world_off = h->frm_world_off.as<uint32_t>();
    in.n = n_msgs;
    in.n_param_bytes = src->param_offsets ? src->n_param_bytes : 0;
    in.n_flex_bytes = src->flex_offsets ? src->n_flex_bytes : 0;
    in.n_world_bytes = h->frm_world_total;
    in.n_worlds = h->frm_n_worlds;
    in.instruction_all = src->instruction_all;
    in.replication_all = src->replication_all;
    c.r = ReplySrc{rec->row_offsets, rec->handles, (uint32_t)nh, rec->flags, rec->slab.entries, rec->slab.n_entries,
                   rec->slab.payload, rec->slab.n_payload_bytes, rec->world_bytes, u8(rec->world_off), u8(rec->world_len),
                   rec->world_bytes ? rec->n_world_bytes : 0};
    const RowSpace r = rows_view(h, rec->row_offsets, (uint32_t)n_msgs, nh);
    c.pre = r.pre;
    c.P = reinterpret_cast<uint64_t*>(p + o_p);
    c.K = reinterpret_cast<uint64_t*>(p + o_k);
    c.X = reinterpret_cast<uint32_t*>(p + o_x);
    c.term = reinterpret_cast<uint32_t*>(p + o_t);
    c.sz = reinterpret_cast<uint32_t*>(p + o_sz);
    c.first = reinterpret_cast<uint32_t*>(p + o_first);

    uint32_t* size = h->frm_size.as<uint32_t>();
    uint32_t* ctrl = h->frm_ctrl.as<uint32_t>();
    const dim3 blk(kBlock);
    const dim3 grid_r(grid_for(rows));
    hipLaunchKernelGGL(k_rows_len, grid_r, blk, 0, s, r, ctrl + 1, kRpErrRows);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_sat(h, r.len, r.sum, rows)) return rc;
    hipLaunchKernelGGL(k_rows_pre, grid_r, blk, 0, s, r, ctrl + 1, kRpErrRows);
    WQ_HIP(h, hipGetLastError());
    const uint32_t* T = r.pre + n_msgs;
    if (nh) {
        hipLaunchKernelGGL(k_reply_term, dim3(grid_for(nh)), blk, 0, s, c, ctrl);
        WQ_HIP(h, hipGetLastError());
    }
    if (int rc = scan_terms(h, RpScanTerm{c.term, T}, c.X, 0u, nh + 1, RpCombine())) return rc;
    if (nh) {
        hipLaunchKernelGGL(k_reply_place, dim3(grid_for(nh)), blk, 0, s, c);
        WQ_HIP(h, hipGetLastError());
    }
    if (int rc = scan_terms(h, RpSizeTerm{c.sz, T, false}, c.P, nh + 1)) return rc;
    if (int rc = scan_terms(h, RpSizeTerm{c.sz, T, true}, c.K, nh + 1)) return rc;
    if (n_msgs) {
        hipLaunchKernelGGL(k_reply_size, dim3(grid_for(n_msgs)), blk, 0, s, c, size, d_frame_size, ctrl);
        WQ_HIP(h, hipGetLastError());
    }
    if (int rc = scan_terms(h, RpFrameTerm{size, n_msgs}, d_frame_offsets, n_msgs + 1)) return rc;
    if (n_msgs && capacity_bytes) {
        const unsigned blocks = (unsigned)pack_blocks(capacity_bytes);
        hipLaunchKernelGGL(k_reply_copy, dim3(blocks), dim3(kPackLanes), 0, s, c, d_frame_offsets, d_frames, (uint64_t)capacity_bytes);
        WQ_HIP(h, hipGetLastError());
    }
    if (d_counters) {
        hipLaunchKernelGGL(k_reply_counters, dim3(1), dim3(1), 0, s, d_frame_offsets, (uint64_t)n_msgs, (uint64_t)capacity_bytes,
                           ctrl, d_counters);
        WQ_HIP(h, hipGetLastError());
    }
    return WQ_OK;
}

}  // namespace wq
