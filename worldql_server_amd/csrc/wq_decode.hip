// wq_decode.hip — the ingest decoder: a tick's received frames verified and decoded on the device.
//
// wq_decode_messages (wq_codec.cpp) does this on the host's cores, and the host then resolves one world
// name and one sender uuid per message and uploads four arrays. Here the raw frames are decoded where
// they land, with world ids and peer ids resolved, into the arrays wq_route_tick_device and
// wq_follow_peers_device take. An extension the reference does not have: its Message::deserialize
// (structures/message.rs:136-142) runs once per message on the host. All arithmetic is decode_ops.hpp.
//
//   walk     one lane per frame: the verifier over Message, Record and Entity, the decode rules, the
//            world and sender lookups, every output of the frame, and the frame's word (flags, status).
//            A string above kDecLane bytes goes to the work list and counts as valid for now; a lane
//            that finds the list full validates it itself.
//   strings  the listed strings: blocks (x) stride over the entries, kDecSlices blocks (y) share one
//            string tile by tile, a lane checks kDecChunk bytes. An invalid chunk ORs kDecTentBad into
//            the frame's word. The list's order depends on the walk's timing; the OR does not.
//   finish   one lane per frame: a frame with kDecTentBad is rewritten to the verifier's failure; the
//            six counts are summed per block in LDS and added with one u64 atomic per block and count.
//
// No lane spins or waits for another. A lane's reads of its frame are byte loads at whatever address
// the frame has: a 136-byte frame is about 25 dependent structure reads of 2 or 4 bytes and 60 string
// bytes, spread over two or three cache lines that neighbouring lanes' frames share.
#include "decode_ops.hpp"
#include "wq_internal.hpp"

namespace wq {

namespace {

static_assert(sizeof(wq_ingest_counters) == 64, "abi.INGEST_COUNTERS_DTYPE mirrors this layout");
static_assert(sizeof(wq_ingest_out) == 72, "abi.IngestOut mirrors this layout");
static_assert(sizeof(wq_decoded_msg) == 72, "wq_decoded_msg has no padding");
static_assert(sizeof(DecEntry) == 16, "the work list is 16 bytes an entry");

constexpr size_t kCtrlBytes = 128;  // wq_ingest_counters, then the list's count at byte 64

__global__ __launch_bounds__(kDecBlock) void k_decode_walk(const uint8_t* __restrict__ frames,
                                                           const uint64_t* __restrict__ fo, uint64_t n,
                                                           uint64_t n_frame_bytes, DecList list, DecTables t,
                                                           wq_ingest_out out, uint32_t* __restrict__ word,
                                                           wq_ingest_counters* ctrl,
                                                           const uint32_t* __restrict__ live_peers) {
    const uint64_t i = (uint64_t)blockIdx.x * kDecBlock + threadIdx.x;
    if (i >= n) return;
    if (live_peers) t.n_peers = *live_peers;  // a reserved sender table: its live count is the device's
    uint32_t err = 0;
    word[i] = dec_walk(frames, fo, i, n, n_frame_bytes, list, t, out, &err);
    if (err) atomicOr(&ctrl->error, err);
}

__global__ __launch_bounds__(kDecBlock) void k_decode_strings(const uint8_t* __restrict__ frames, DecList list,
                                                              uint32_t* __restrict__ word) {
    const uint32_t appended = *list.count;
    const uint32_t cnt = appended < list.cap ? appended : list.cap;
    for (uint32_t k = blockIdx.x; k < cnt; k += gridDim.x) {
        const DecEntry e = list.e[k];
        bool bad = false;
        for (uint64_t t0 = (uint64_t)blockIdx.y * kDecTile; t0 < e.len; t0 += (uint64_t)kDecSlices * kDecTile) {
            const uint64_t c0 = t0 + (uint64_t)threadIdx.x * kDecChunk;
            if (c0 < e.len && !dec_entry_chunk_ok(frames, e, c0)) bad = true;
        }
        if (bad) atomicOr(&word[e.frame], kDecTentBad);
    }
}

__global__ __launch_bounds__(kDecBlock) void k_decode_finish(uint64_t n, wq_ingest_out out,
                                                             const uint32_t* __restrict__ word,
                                                             wq_ingest_counters* ctrl) {
    __shared__ uint32_t sum[6];
    if (threadIdx.x < 6) sum[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * kDecBlock + threadIdx.x;
    if (i < n) {
        uint32_t c[6] = {0, 0, 0, 0, 0, 0};
        dec_count(dec_finish(word[i], i, out), c);
        for (int k = 0; k < 6; ++k)
            if (c[k]) atomicAdd(&sum[k], c[k]);
    }
    __syncthreads();
    if (threadIdx.x < 6 && sum[threadIdx.x]) {
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(&ctrl->n_ok) + threadIdx.x;
        atomicAdd(dst, (unsigned long long)sum[threadIdx.x]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->n_frames = n;
}

}  // namespace

void ingest_release(wq_router* h) {
    for (DevBuf* b : {&h->ing_word, &h->ing_list, &h->ing_ctrl, &h->ing_whash, &h->ing_wid, &h->ing_phi, &h->ing_plo,
                      &h->ing_pid})
        b->release();
    h->ing_n_peers = 0;
}

// The lookup order beside the world table (the handle's device is current, the stream idle, n_worlds > 0).
// Waited for: the vectors are free on return.
int ingest_set_world_index(wq_router* h, const uint8_t* names, const uint32_t* off, uint32_t n_worlds) {
    std::vector<uint64_t> hash;
    std::vector<uint32_t> id;
    dec_world_index(names, off, n_worlds, &hash, &id);
    WQ_ALLOC(h, h->ing_whash, (size_t)n_worlds * 8);
    WQ_ALLOC(h, h->ing_wid, (size_t)n_worlds * 4);
    WQ_HIP(h, hipMemcpyAsync(h->ing_whash.p, hash.data(), (size_t)n_worlds * 8, hipMemcpyHostToDevice, h->stream));
    WQ_HIP(h, hipMemcpyAsync(h->ing_wid.p, id.data(), (size_t)n_worlds * 4, hipMemcpyHostToDevice, h->stream));
    WQ_HIP(h, hipStreamSynchronize(h->stream));
    return WQ_OK;
}

// The sender table (the handle's device is current; arguments validated). Like the world table: waited
// for, ordered behind earlier decodes and before later ones, and an error leaves no table, not a torn one.
int ingest_set_peers(wq_router* h, const uint8_t* uuids, const uint32_t* ids, uint32_t n) {
    const bool reserved = h->ing_live.p != nullptr;  // wq_ingest_peers_reserve: the live count is a device word
    if (n == 0) {
        h->ing_n_peers = 0;
        if (reserved) {
            WQ_HIP(h, hipStreamSynchronize(h->stream));
            WQ_HIP(h, hipMemcpy(h->ing_live.p, &n, 4, hipMemcpyHostToDevice));
        }
        return WQ_OK;
    }
    std::vector<uint64_t> hi, lo;
    std::vector<uint32_t> id;
    if (!dec_peer_index(uuids, ids, n, &hi, &lo, &id))
        return set_error(h, WQ_E_INVALID, "ingest_set_peers: a uuid occurs twice");
    WQ_HIP(h, hipStreamSynchronize(h->stream));  // a growing buffer is freed: nothing may still read it
    const size_t room = reserved && h->ing_cap > n ? h->ing_cap : n;  // the reserved room is kept, or grown
    WQ_ALLOC(h, h->ing_phi, room * 8);
    WQ_ALLOC(h, h->ing_plo, room * 8);
    WQ_ALLOC(h, h->ing_pid, room * 4);
    h->ing_n_peers = 0;
    if (reserved) {
        const uint32_t none = 0;
        WQ_HIP(h, hipMemcpy(h->ing_live.p, &none, 4, hipMemcpyHostToDevice));
        h->ing_cap = (uint32_t)room;
    }
    WQ_HIP(h, hipMemcpyAsync(h->ing_phi.p, hi.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    WQ_HIP(h, hipMemcpyAsync(h->ing_plo.p, lo.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    WQ_HIP(h, hipMemcpyAsync(h->ing_pid.p, id.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    WQ_HIP(h, hipStreamSynchronize(h->stream));
    h->ing_n_peers = n;
    if (reserved) WQ_HIP(h, hipMemcpy(h->ing_live.p, &n, 4, hipMemcpyHostToDevice));
    return WQ_OK;
}

// The handle's two tables as the kernels take them (the record dispatch looks worlds up in the same one).
void ingest_tables(const wq_router* h, DecTables* t) {
    t->n_worlds = h->frm_n_worlds;
    t->world_bytes = h->frm_n_worlds ? h->frm_world_bytes.as<uint8_t>() + kDecWorldSlack : nullptr;
    t->world_off = h->frm_world_off.as<uint32_t>();
    t->world_hash = h->ing_whash.as<uint64_t>();
    t->world_id = h->ing_wid.as<uint32_t>();
    t->n_peers = h->ing_n_peers;
    t->peer_hi = h->ing_phi.as<uint64_t>();
    t->peer_lo = h->ing_plo.as<uint64_t>();
    t->peer_id = h->ing_pid.as<uint32_t>();
}

// The call on device arrays (the handle's device is current; arguments validated, n_frames < 2^32 - 1).
int launch_frames_decode(wq_router* h, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n_frames,
                         size_t n_frame_bytes, const wq_ingest_out* out, wq_ingest_counters* d_counters) {
    hipStream_t s = h->stream;
    const uint32_t cap = h->ing_list_cap < 0 ? kDecListDefault : (uint32_t)h->ing_list_cap;
    WQ_ALLOC(h, h->ing_word, n_frames * 4);
    WQ_ALLOC(h, h->ing_list, (size_t)cap * sizeof(DecEntry));
    WQ_ALLOC(h, h->ing_ctrl, kCtrlBytes);
    WQ_HIP(h, hipMemsetAsync(h->ing_ctrl.p, 0, kCtrlBytes, s));
    wq_ingest_counters* ctrl = h->ing_ctrl.as<wq_ingest_counters>();
    if (n_frames) {
        DecList list{h->ing_list.as<DecEntry>(), reinterpret_cast<uint32_t*>(h->ing_ctrl.as<uint8_t>() + 64), cap};
        DecTables t;
        ingest_tables(h, &t);
        uint32_t* word = h->ing_word.as<uint32_t>();
        const unsigned blocks = (unsigned)((n_frames + kDecBlock - 1) / kDecBlock);
        hipLaunchKernelGGL(k_decode_walk, dim3(blocks), dim3(kDecBlock), 0, s, d_frames, d_frame_offsets,
                           (uint64_t)n_frames, (uint64_t)n_frame_bytes, list, t, *out, word, ctrl,
                           h->ing_live.as<const uint32_t>());
        WQ_HIP(h, hipGetLastError());
        if (cap) {
            const unsigned bx = cap < kDecListBlocks ? cap : kDecListBlocks;
            hipLaunchKernelGGL(k_decode_strings, dim3(bx, kDecSlices), dim3(kDecBlock), 0, s, d_frames, list, word);
            WQ_HIP(h, hipGetLastError());
        }
        hipLaunchKernelGGL(k_decode_finish, dim3(blocks), dim3(kDecBlock), 0, s, (uint64_t)n_frames, *out, word, ctrl);
        WQ_HIP(h, hipGetLastError());
    }
    if (d_counters) WQ_HIP(h, hipMemcpyAsync(d_counters, ctrl, sizeof(wq_ingest_counters), hipMemcpyDeviceToDevice, s));
    return WQ_OK;
}

}  // namespace wq
