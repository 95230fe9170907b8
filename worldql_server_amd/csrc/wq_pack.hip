// wq_pack.hip — send buffers: every peer's frames gathered into one contiguous byte run.
//
// The budgets leave, per peer, a list of message indices; the tick's frames sit in one byte array
// (wq_serialize_messages). Here every element of the peer-major CSR becomes a record, an optional
// u32 size and the frame, and the records are laid out in list order: peer p's run is
// out[PB[p] .. PB[p + 1]). An extension the reference does not have: its broadcast_to!
// (transport/peer_map.rs:22-40) clones the bytes and sends once per recipient on the host.
//
//   rows   one lane per peer: the clamped length; the saturating scan and the clamp to n_in give the
//          ordinal space (send_rows.hpp, as the budgets)
//   size   one lane per ordinal: its row (a search over the prefix), its message, its frame under the
//          validity rules (pack_ops.hpp): the frame's size and where it starts
//   scan   one u64 exclusive scan of the record sizes over the ordinals: E
//   PB     one lane per peer: E at the row's first ordinal; one lane per ordinal copies E to the
//          caller's d_out_elem_bytes
//   copy   over the output bytes [0, bytes_written): a wave owns a tile of 64 x 16 bytes and a lane
//          one 16-byte chunk. One search per tile finds the element that covers its first byte
//          (over all of E for a block's first tile, from the last tile's end for the next ones). A
//          tile inside one frame's payload is 64 unaligned 16-byte loads and 64 aligned stores.
//          Otherwise the tile's elements go through LDS 64 at a time (their E and source offsets),
//          every lane finds its chunk's first element there and composes the chunk from its one or
//          more elements: prefixes from sizes, payload parts from one masked 16-byte load each, byte
//          by byte only where those 16 bytes would leave the frame array. The output's last chunk
//          is stored with narrower stores.
//
// No lane, wave or block owns a row or a frame: a 1 MiB frame is a thousand tiles, a thousand empty
// frames are windows of one tile. Placement comes from the scans alone; the only atomics are ORs
// into the error word, so the output is the same bytes every time.
#include "pack_ops.hpp"
#include "send_rows.hpp"

namespace wq {

namespace {

static_assert(kPackFlagPrefix == WQ_PACK_LEN_PREFIX, "the header's flag");
static_assert(sizeof(wq_pack_counters) == 40, "wq_pack_counters is 40 bytes");

struct PackIn {
    const uint32_t* off;
    const uint32_t* msgs;
    const uint8_t* frames;
    const uint64_t* fo;
    uint64_t n_msgs, n_frame_bytes;
    uint32_t n_peers, n_in, pre;  // pre: bytes of the length prefix, 0 or 4
};

struct PackWs {
    uint32_t* len;   // [n_peers + 1] clamped lengths
    uint32_t* sum;   // [n_peers + 1] their saturating prefix
    uint32_t* pre;   // [n_peers + 1] the prefix clamped to n_in: the ordinal space
    uint32_t* size;  // [n_in] frame sizes
    uint64_t* src;   // [n_in] where each frame starts in the frame bytes
    uint64_t* E;     // [n_in + 1]
    uint32_t* ctrl;  // {unused, error}
};

struct PackTerm {
    const uint32_t* size;
    const uint32_t* T;
    uint32_t pre;
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t q) const {
        return pack_rec_term(size, *T, pre, q);
    }
};

__global__ __launch_bounds__(kBlock) void k_pack_size(PackIn in, PackWs ws) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= ws.pre[in.n_peers]) return;
    const uint32_t p = bud_row_of(ws.pre, in.n_peers, (uint32_t)q);
    const uint32_t j = rows_elem(in.off, ws.pre, in.n_in, p, (uint32_t)q);
    uint32_t err = 0;
    uint64_t src;
    ws.size[q] = pack_frame(in.fo, in.n_msgs, in.n_frame_bytes, in.msgs[j], &src, &err);
    ws.src[q] = src;
    if (err) atomicOr(&ws.ctrl[1], err);
}

__global__ __launch_bounds__(kBlock) void k_pack_peer_bytes(PackWs ws, uint32_t n_peers,
                                                             uint64_t* __restrict__ out_peer_bytes) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > n_peers) return;
    out_peer_bytes[p] = ws.E[ws.pre[p]];
}

__global__ __launch_bounds__(kBlock) void k_pack_elem_bytes(PackWs ws, uint32_t n_peers,
                                                             uint64_t* __restrict__ out_elem_bytes) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= ws.pre[n_peers]) return;
    out_elem_bytes[q] = ws.E[q];
}

// One wave per block; the blocks share the tiles below bytes_written in consecutive runs, so only a
// block's first tile searches all of E. Everything that decides a branch around a barrier is the
// same in all 64 lanes (the tile, its first element, the window).
__global__ __launch_bounds__(kPackLanes) void k_pack_copy(PackIn in, PackWs ws, uint8_t* __restrict__ out,
                                                          uint64_t capacity) {
    __shared__ uint64_t W[kPackWindow + 1];
    __shared__ uint64_t S[kPackWindow];
    const uint32_t T = ws.pre[in.n_peers];
    const uint64_t need = ws.E[T];
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
        // the block's first tile searches all of E; the next one starts from where this one ended
        e0 = i ? pack_elem_from(ws.E, T, e0, c0) : pack_elem_of(ws.E, T, c0);
        const uint64_t r0 = ws.E[e0], r1 = ws.E[e0 + 1];
        if (pack_tile_inside(r0, r1, in.pre, c0, c1)) {
            pack_store(out, d0, kPackChunk, pack_load16(in.frames + ws.src[e0] + (d0 - r0 - in.pre)));
            continue;
        }
        PackChunk v{0ull, 0ull};
        for (uint64_t wb = e0;; wb += kPackWindow) {
            __syncthreads();  // the window before this one has been read
            W[lane] = pack_win_entry(ws.E, T, wb, lane);
            if (lane == 0) W[kPackWindow] = pack_win_entry(ws.E, T, wb, kPackWindow);
            S[lane] = wb + lane < T ? ws.src[wb + lane] : 0ull;
            __syncthreads();
            const uint64_t w0 = W[0], w1 = W[kPackWindow];
            const uint64_t lo = d0 > w0 ? d0 : w0, hi = d1 < w1 ? d1 : w1;
            if (lo < hi) pack_compose(W, S, in.frames, in.n_frame_bytes, in.pre, d0, lo, hi, &v);
            if (w1 >= c1) {
                e0 = (uint32_t)wb + pack_win_find(W, c1 - 1);  // the element of the tile's last byte
                break;
            }
        }
        if (d0 < d1) pack_store(out, d0, (uint32_t)(d1 - d0), v);
    }
}

__global__ void k_pack_counters(PackWs ws, uint32_t n_peers, uint64_t capacity, wq_pack_counters* counters) {
    const uint32_t T = ws.pre[n_peers];
    const uint64_t need = ws.E[T];
    wq_pack_counters c;
    c.n_in = T;
    c.n_complete = pack_elem_of(ws.E, T, capacity);
    c.bytes_need = need;
    c.bytes_written = need < capacity ? need : capacity;
    c.overflow = need > capacity ? 1u : 0u;
    c.error = ws.ctrl[1];
    *counters = c;
}

}  // namespace

void pack_release(wq_router* h) {
    for (DevBuf* b : {&h->pack_size, &h->pack_src, &h->pack_scan, &h->pack_ctrl}) b->release();
}

// The call on device arrays (the handle's device is current; arguments validated, n_in <= 2^32 - 1).
// The ordinal space's three buffers are the budgets' (send_rows.hpp rows_alloc): the calls are ordered
// on the handle's stream and nothing in them outlives a call. Everything else is this path's own.
int launch_peer_pack(wq_router* h, const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers, size_t n_in,
                     const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n_msgs, size_t n_frame_bytes,
                     uint32_t flags, uint8_t* d_out, size_t capacity_bytes, uint64_t* d_out_peer_bytes,
                     uint64_t* d_out_elem_bytes, wq_pack_counters* d_counters) {
    hipStream_t s = h->stream;
    const size_t rows = (size_t)n_peers + 1;
    if (int rc = rows_alloc(h, rows)) return rc;
    WQ_ALLOC(h, h->pack_size, n_in * 4);
    WQ_ALLOC(h, h->pack_src, n_in * 8);
    WQ_ALLOC(h, h->pack_scan, (n_in + 1) * 8);
    WQ_ALLOC(h, h->pack_ctrl, 64);
    WQ_HIP(h, hipMemsetAsync(h->pack_ctrl.p, 0, 64, s));

    const PackIn in{d_peer_offsets, d_msgs,  d_frames,       d_frame_offsets,         (uint64_t)n_msgs, (uint64_t)n_frame_bytes,
                    n_peers,        (uint32_t)n_in, pack_prefix_bytes(flags)};
    const RowSpace r = rows_view(h, d_peer_offsets, n_peers, n_in);
    const PackWs ws{r.len, r.sum, r.pre, h->pack_size.as<uint32_t>(), h->pack_src.as<uint64_t>(),
                    h->pack_scan.as<uint64_t>(), h->pack_ctrl.as<uint32_t>()};

    const dim3 blk(kBlock);
    const dim3 grid_r(grid_for(rows));
    hipLaunchKernelGGL(k_rows_len, grid_r, blk, 0, s, r, ws.ctrl + 1, kBudErrRows);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_sat(h, ws.len, ws.sum, rows)) return rc;
    hipLaunchKernelGGL(k_rows_pre, grid_r, blk, 0, s, r, ws.ctrl + 1, kBudErrRows);
    WQ_HIP(h, hipGetLastError());
    if (n_in) {
        hipLaunchKernelGGL(k_pack_size, dim3(grid_for(n_in)), blk, 0, s, in, ws);
        WQ_HIP(h, hipGetLastError());
    }
    if (int rc = scan_terms(h, PackTerm{ws.size, ws.pre + n_peers, in.pre}, ws.E, n_in + 1)) return rc;
    hipLaunchKernelGGL(k_pack_peer_bytes, grid_r, blk, 0, s, ws, n_peers, d_out_peer_bytes);
    WQ_HIP(h, hipGetLastError());
    if (n_in && d_out_elem_bytes) {
        hipLaunchKernelGGL(k_pack_elem_bytes, dim3(grid_for(n_in)), blk, 0, s, ws, n_peers, d_out_elem_bytes);
        WQ_HIP(h, hipGetLastError());
    }
    if (n_in && capacity_bytes) {
        const unsigned blocks = (unsigned)pack_blocks(capacity_bytes);
        hipLaunchKernelGGL(k_pack_copy, dim3(blocks), dim3(kPackLanes), 0, s, in, ws, d_out, (uint64_t)capacity_bytes);
        WQ_HIP(h, hipGetLastError());
    }
    if (d_counters) {
        hipLaunchKernelGGL(k_pack_counters, dim3(1), dim3(1), 0, s, ws, n_peers, (uint64_t)capacity_bytes, d_counters);
        WQ_HIP(h, hipGetLastError());
    }
    return WQ_OK;
}

}  // namespace wq
