// wq_frames.hip — the frame builder: a tick's flat messages serialized on the device.
//
// wq_serialize_messages (wq_codec.cpp) builds a tick's FlatBuffer frames on the host from values that,
// for entity updates, the device already holds. Here the same bytes are written on the device, ready
// for wq_peer_budget_bytes_device and wq_peer_pack_device, for messages without records and entities.
// An extension the reference does not have: its Message::serialize (structures/message.rs:120-134)
// runs once per message on the host.
//
//   size   one lane per message: its fields under the validity rules and the builder's push sequence
//          replayed on counters (frame_ops.hpp): the frame's size
//   scan   one u64 exclusive scan of the sizes into the caller's d_frame_offsets: E
//   copy   over the output bytes [0, bytes_written) in the send buffers' shape (wq_pack.hip): a wave
//          owns a tile of 64 x 16 bytes and a lane one 16-byte chunk; one search per tile finds the
//          frame that covers its first byte. A tile inside one parameter or flex payload is 64
//          unaligned 16-byte loads and 64 aligned stores. Otherwise the tile's frame offsets go through
//          LDS 64 at a time, every lane finds its chunk's first frame there and replays the push
//          sequence of each frame that touches the chunk, keeping the pieces that fall into it:
//          values from the replay, payload, world and position bytes from one masked 16-byte load
//          each, the uuid's text from one load of its 16 bytes.
//
// No lane, wave or block owns a frame or a payload: a 1 MiB flex is a thousand tiles. Placement comes
// from the scan alone; the only atomics are ORs into the error word.
#include "decode_ops.hpp"
#include "frame_ops.hpp"
#include "send_rows.hpp"

namespace wq {

namespace {

static_assert(sizeof(wq_frames_counters) == 40, "wq_frames_counters is 40 bytes");
static_assert(sizeof(wq_frames_src) == 112, "abi.FramesSrc mirrors this layout");
static_assert(kDecWorldSlack == kFrWorldSlack, "the ingest decoder reads the same table");

struct FrameTerm {
    const uint32_t* size;
    uint64_t n;
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t q) const { return frame_term(size, n, q); }
};

__global__ __launch_bounds__(kBlock) void k_frames_size(FrameSrc src, uint32_t* __restrict__ size,
                                                        uint32_t* __restrict__ out_size, uint32_t* __restrict__ ctrl) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= src.n) return;
    const FrameMsg m = frame_msg(src, i);
    uint32_t err = m.err;
    const uint32_t s = frame_size(m, &err);
    size[i] = s;
    if (out_size) out_size[i] = s;
    if (err) atomicOr(&ctrl[1], err);
}

// One wave per block; the blocks share the tiles below bytes_written in consecutive runs, so only a
// block's first tile searches all of E. Everything that decides a branch around a barrier is the
// same in all 64 lanes (the tile, its first frame, the window).
__global__ __launch_bounds__(kPackLanes) void k_frames_copy(FrameSrc src, const uint64_t* __restrict__ E,
                                                            uint8_t* __restrict__ out, uint64_t capacity) {
    __shared__ uint64_t W[kPackWindow + 1];
    const uint32_t T = (uint32_t)src.n;
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
            if (frame_tile_inside(src, frame_msg(src, e0), r0, r1, c0, c1, &from)) {
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
            if (lo < hi) frame_compose(W, wb, src, d0, lo, hi, &v);
            if (w1 >= c1) {
                e0 = (uint32_t)wb + pack_win_find(W, c1 - 1);  // the frame of the tile's last byte
                break;
            }
        }
        if (d0 < d1) pack_store(out, d0, (uint32_t)(d1 - d0), v);
    }
}

__global__ void k_frames_counters(const uint64_t* __restrict__ E, uint64_t n, uint64_t capacity,
                                  const uint32_t* __restrict__ ctrl, wq_frames_counters* counters) {
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

// Rust std::str::from_utf8 acceptance, as wq_codec.cpp checks a message's strings.
bool utf8_ok(const uint8_t* s, size_t n) {
    size_t i = 0;
    while (i < n) {
        const uint8_t c = s[i];
        if (c < 0x80) {
            ++i;
            continue;
        }
        size_t k;
        uint8_t lo = 0x80, hi = 0xBF;
        if (c >= 0xC2 && c <= 0xDF) k = 1;
        else if (c == 0xE0) { k = 2; lo = 0xA0; }
        else if ((c >= 0xE1 && c <= 0xEC) || c == 0xEE || c == 0xEF) k = 2;
        else if (c == 0xED) { k = 2; hi = 0x9F; }
        else if (c == 0xF0) { k = 3; lo = 0x90; }
        else if (c >= 0xF1 && c <= 0xF3) k = 3;
        else if (c == 0xF4) { k = 3; hi = 0x8F; }
        else return false;
        if (i + k >= n) return false;
        if (s[i + 1] < lo || s[i + 1] > hi) return false;
        for (size_t j = 2; j <= k; ++j)
            if (s[i + j] < 0x80 || s[i + j] > 0xBF) return false;
        i += k + 1;
    }
    return true;
}

}  // namespace

void frames_release(wq_router* h) {
    for (DevBuf* b : {&h->frm_size, &h->frm_ctrl, &h->frm_world_bytes, &h->frm_world_off}) b->release();
    h->frm_n_worlds = 0;
    h->frm_world_total = 0;
}

// The table on the device (the handle's device is current; arguments validated). The copies are
// waited for, so the caller's arrays are free on return and every later build sees the new table;
// builds already on the stream finish first, they are ahead of the copies.
int frames_set_worlds(wq_router* h, const char* names, const uint32_t* name_offsets, uint32_t n_worlds) {
    if (n_worlds == 0) {
        h->frm_n_worlds = 0;
        h->frm_world_total = 0;
        return WQ_OK;
    }
    const uint32_t first = name_offsets[0], total = name_offsets[n_worlds] - first;
    std::vector<uint32_t> off((size_t)n_worlds + 1);
    for (size_t w = 0; w <= n_worlds; ++w) off[w] = name_offsets[w] - first;
    WQ_HIP(h, hipStreamSynchronize(h->stream));  // a growing buffer is freed: nothing may still read it
    WQ_ALLOC(h, h->frm_world_off, off.size() * 4);
    WQ_ALLOC(h, h->frm_world_bytes, (size_t)total + 2 * kFrWorldSlack);  // zero slack on both sides of the names
    h->frm_n_worlds = 0;  // an error below leaves no table rather than a torn one
    h->frm_world_total = 0;
    WQ_HIP(h, hipMemcpyAsync(h->frm_world_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, h->stream));
    WQ_HIP(h, hipMemsetAsync(h->frm_world_bytes.p, 0, (size_t)total + 2 * kFrWorldSlack, h->stream));
    if (total)
        WQ_HIP(h, hipMemcpyAsync(h->frm_world_bytes.as<uint8_t>() + kFrWorldSlack, names + first, total,
                                 hipMemcpyHostToDevice, h->stream));
    WQ_HIP(h, hipStreamSynchronize(h->stream));
    // the order wq_frames_decode_device looks a name up in, beside the table
    if (int rc = ingest_set_world_index(h, reinterpret_cast<const uint8_t*>(names) + first, off.data(), n_worlds)) return rc;
    h->frm_n_worlds = n_worlds;
    h->frm_world_total = total;
    return WQ_OK;
}

bool frames_worlds_valid(const char* names, const uint32_t* name_offsets, uint32_t n_worlds) {
    if (n_worlds == 0) return true;
    if (!name_offsets) return false;
    for (uint32_t w = 0; w < n_worlds; ++w)
        if (name_offsets[w] > name_offsets[w + 1]) return false;
    if (!names && name_offsets[n_worlds] != name_offsets[0]) return false;
    for (uint32_t w = 0; w < n_worlds; ++w)
        if (!utf8_ok(reinterpret_cast<const uint8_t*>(names) + name_offsets[w], name_offsets[w + 1] - name_offsets[w]))
            return false;
    return true;
}

// The call on device arrays (the handle's device is current; arguments validated, n_msgs < 2^32 - 1).
int launch_frames_build(wq_router* h, const wq_frames_src* src, size_t n_msgs, uint8_t* d_frames, size_t capacity_bytes,
                        uint64_t* d_frame_offsets, uint32_t* d_frame_size, wq_frames_counters* d_counters) {
    hipStream_t s = h->stream;
    WQ_ALLOC(h, h->frm_size, n_msgs * 4);
    WQ_ALLOC(h, h->frm_ctrl, 64);
    WQ_HIP(h, hipMemsetAsync(h->frm_ctrl.p, 0, 64, s));

    auto u8 = [](const void* p) { return static_cast<const uint8_t*>(p); };
    FrameSrc in;
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

    uint32_t* size = h->frm_size.as<uint32_t>();
    uint32_t* ctrl = h->frm_ctrl.as<uint32_t>();
    if (n_msgs) {
        hipLaunchKernelGGL(k_frames_size, dim3(grid_for(n_msgs)), dim3(kBlock), 0, s, in, size, d_frame_size, ctrl);
        WQ_HIP(h, hipGetLastError());
    }
    if (int rc = scan_terms(h, FrameTerm{size, n_msgs}, d_frame_offsets, n_msgs + 1)) return rc;
    if (n_msgs && capacity_bytes) {
        const unsigned blocks = (unsigned)pack_blocks(capacity_bytes);
        hipLaunchKernelGGL(k_frames_copy, dim3(blocks), dim3(kPackLanes), 0, s, in, d_frame_offsets, d_frames,
                           (uint64_t)capacity_bytes);
        WQ_HIP(h, hipGetLastError());
    }
    if (d_counters) {
        hipLaunchKernelGGL(k_frames_counters, dim3(1), dim3(1), 0, s, d_frame_offsets, (uint64_t)n_msgs,
                           (uint64_t)capacity_bytes, ctrl, d_counters);
        WQ_HIP(h, hipGetLastError());
    }
    return WQ_OK;
}

}  // namespace wq
