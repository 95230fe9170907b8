// wq_sends.hip — tick sends: one per-peer frame list from all of a tick's read runs
// (include/wq_router.h wq_tick_sends_device).
//
// A dispatched tick is routed run by run: every read run leaves a CSR region for its LocalMessage rows,
// one for its GlobalMessage rows, or both, and inside one run the two kinds interleave by frame. The
// transport wants, per peer, the received frames in arrival order — the reference's broadcast_to per
// message, restated as one list. Here, over the regions' elements laid end to end:
//   begin    the counters zeroed, n_regions and n_elems written
//   rows     one lane per row of the regions that have offsets: a row that ends before it starts or past
//            its region's capacity sets error bit 0
//   expand   one lane per element: its region (a search over the uploaded element prefix), its row (a
//            search over the region's offsets; none for unit rows), its frame and its peer, then the key
//            (peer or sentinel n_peers) << frame_bits | frame and the frame as value; a dropped element
//            gets the sentinel and frame 0, so all n_elems keys and values are written on every call.
//            The block's counts go to the counters with one integer atomic each (sends_ops.hpp)
//   sort     one stable radix sort of (key, frame) over pm_key_bits(n_peers) + frame_bits bits: u32 keys
//            when that is at most 32 bits, u64 keys otherwise; the values land in d_frames_out
//   offsets  one lane per peer: the lower bound of p << frame_bits in the sorted keys
// The regions are a host array: checked, copied with their prefixes into a pinned buffer of the handle's
// and uploaded from there; the next call waits for that copy's event before it refills the buffer.
#include "sends_ops.hpp"
#include "table_prims.hpp"

namespace wq {

namespace {

__global__ void k_snd_begin(uint64_t n_regions, uint64_t n_elems, wq_tick_sends_counters* ctrl) {
    if (threadIdx.x) return;
    wq_tick_sends_counters c{};
    c.n_regions = n_regions;
    c.n_elems = n_elems;
    *ctrl = c;
}

__global__ __launch_bounds__(kBlock) void k_snd_rows(SndView v, uint64_t n_rows, wq_tick_sends_counters* ctrl) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const int bad = i < n_rows && snd_row_bad(v, i);
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(&ctrl->error, 1u);
}

template <typename K>
__global__ __launch_bounds__(kBlock) void k_snd_expand(SndView v, uint32_t n_elems, K* __restrict__ key,
                                                       uint32_t* __restrict__ val, wq_tick_sends_counters* ctrl) {
    __shared__ uint32_t sum[4];
    if (threadIdx.x < 4) sum[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n_elems) {
        K k;
        uint32_t f;
        const int what = snd_elem<K>(v, (uint32_t)j, &k, &f);
        key[j] = k;
        val[j] = f;
        if (what) atomicAdd(&sum[what], 1u);
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < 4 && sum[threadIdx.x]) {
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(&ctrl->n_kept) + (threadIdx.x - 1);
        atomicAdd(dst, (unsigned long long)sum[threadIdx.x]);
    }
    if (threadIdx.x == 0) {
        const uint32_t covered = sum[kSndKept] + sum[kSndDropPeer] + sum[kSndDropFrame];
        if (covered) atomicAdd(reinterpret_cast<unsigned long long*>(&ctrl->n_covered), (unsigned long long)covered);
        if (sum[kSndDropFrame]) atomicOr(&ctrl->error, 2u);
    }
}

template <typename K>
__global__ void k_snd_offsets(const K* __restrict__ skey, uint32_t P, uint32_t n_peers, int frame_bits,
                              uint32_t* __restrict__ out) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > n_peers) return;
    out[p] = snd_lower_bound<K>(skey, P, (uint32_t)p, frame_bits);
}

template <typename K>
int expand_sort_offsets(wq_router* h, const SndView& v, uint32_t P, DevBuf& ka, DevBuf& kb, uint32_t* d_peer_offsets,
                        uint32_t* d_frames_out, wq_tick_sends_counters* ctrl) {
    hipStream_t s = h->stream;
    WQ_ALLOC(h, ka, (size_t)P * sizeof(K));
    WQ_ALLOC(h, kb, (size_t)P * sizeof(K));
    WQ_ALLOC(h, h->idx_a, (size_t)P * 4);
    K* key = ka.as<K>();
    K* skey = kb.as<K>();
    uint32_t* val = h->idx_a.as<uint32_t>();
    hipLaunchKernelGGL(k_snd_expand<K>, dim3(grid_for(P)), dim3(kBlock), 0, s, v, P, key, val, ctrl);
    WQ_HIP(h, hipGetLastError());
    int rc = sort_pairs<K>(h, key, skey, val, d_frames_out, P, pm_key_bits(v.n_peers) + v.frame_bits);
    if (rc) return rc;
    hipLaunchKernelGGL(k_snd_offsets<K>, dim3(grid_for((uint64_t)v.n_peers + 1)), dim3(kBlock), 0, s, skey, P,
                       v.n_peers, v.frame_bits, d_peer_offsets);
    WQ_HIP(h, hipGetLastError());
    return WQ_OK;
}

}  // namespace

void sends_release(wq_router* h) {
    if (h->snd_ev) (void)hipEventDestroy(h->snd_ev);
    if (h->snd_pinned) (void)hipHostFree(h->snd_pinned);
    h->snd_ev = nullptr;
    h->snd_pinned = nullptr;
    h->snd_pinned_bytes = 0;
    h->snd_pending = false;
    h->snd_tab.release();
    h->snd_ctrl.release();
}

// The call on device arrays (the handle's device is current; the pointers checked against their sizes).
int launch_tick_sends(wq_router* h, const wq_tick_sends_in* in, uint32_t* d_peer_offsets, uint32_t* d_frames_out,
                      size_t n_elems, wq_tick_sends_counters* d_counters) {
    if (const char* why = snd_check(in, n_elems)) return set_error(h, WQ_E_INVALID, why);
    hipStream_t s = h->stream;
    const uint32_t n = in->n_regions, P = (uint32_t)n_elems;
    // [row_pre u64 x (n + 1)][regions x n][elem_pre u32 x (n + 1)]
    const size_t at_reg = 8 * ((size_t)n + 1), at_elem = at_reg + sizeof(wq_send_region) * (size_t)n;
    const size_t bytes = at_elem + 4 * ((size_t)n + 1);
    // the previous call's upload reads the pinned buffer: wait for that copy alone, not for the stream
    if (h->snd_pending) {
        WQ_HIP(h, hipEventSynchronize(h->snd_ev));
        h->snd_pending = false;
    }
    if (bytes > h->snd_pinned_bytes) {
        if (h->snd_pinned) WQ_HIP(h, hipHostFree(h->snd_pinned));
        h->snd_pinned = nullptr;
        h->snd_pinned_bytes = 0;
        const size_t cap = bytes < 4096 ? 4096 : bytes + bytes / 4;
        if (hipHostMalloc(&h->snd_pinned, cap, hipHostMallocDefault) != hipSuccess) {
            h->snd_pinned = nullptr;
            return set_error(h, WQ_E_OOM, "tick_sends: hipHostMalloc of the region staging buffer");
        }
        h->snd_pinned_bytes = cap;
    }
    if (!h->snd_ev) WQ_HIP(h, hipEventCreateWithFlags(&h->snd_ev, hipEventDisableTiming));
    WQ_ALLOC(h, h->snd_tab, bytes);
    WQ_ALLOC(h, h->snd_ctrl, sizeof(wq_tick_sends_counters));
    uint8_t* stage = static_cast<uint8_t*>(h->snd_pinned);
    uint64_t* row_pre = reinterpret_cast<uint64_t*>(stage);
    if (n) std::memcpy(stage + at_reg, in->regions, sizeof(wq_send_region) * (size_t)n);
    snd_prefixes(in->regions, n, reinterpret_cast<uint32_t*>(stage + at_elem), row_pre);
    const uint64_t n_rows = row_pre[n];
    WQ_HIP(h, hipMemcpyAsync(h->snd_tab.p, stage, bytes, hipMemcpyHostToDevice, s));
    WQ_HIP(h, hipEventRecord(h->snd_ev, s));
    h->snd_pending = true;

    const uint8_t* tab = h->snd_tab.as<uint8_t>();
    SndView v;
    v.row_pre = reinterpret_cast<const uint64_t*>(tab);
    v.reg = reinterpret_cast<const wq_send_region*>(tab + at_reg);
    v.elem_pre = reinterpret_cast<const uint32_t*>(tab + at_elem);
    v.off = in->d_offsets;
    v.peers = in->d_peers;
    v.src[0] = in->d_src[0];
    v.src[1] = in->d_src[1];
    v.connected = in->d_connected;
    v.n_regions = n;
    v.n_peers = in->n_peers;
    v.n_frames = in->n_frames;
    v.frame_bits = snd_frame_bits(in->n_frames);
    wq_tick_sends_counters* ctrl = h->snd_ctrl.as<wq_tick_sends_counters>();
    hipLaunchKernelGGL(k_snd_begin, dim3(1), dim3(64), 0, s, (uint64_t)n, (uint64_t)n_elems, ctrl);
    WQ_HIP(h, hipGetLastError());
    if (n_rows) {
        hipLaunchKernelGGL(k_snd_rows, dim3(grid_for(n_rows)), dim3(kBlock), 0, s, v, n_rows, ctrl);
        WQ_HIP(h, hipGetLastError());
    }
    int rc = WQ_OK;
    if (P == 0) {
        hipLaunchKernelGGL(k_snd_offsets<uint32_t>, dim3(grid_for((uint64_t)in->n_peers + 1)), dim3(kBlock), 0, s,
                           static_cast<const uint32_t*>(nullptr), 0u, in->n_peers, 0, d_peer_offsets);
        WQ_HIP(h, hipGetLastError());
    } else if (pm_key_bits(in->n_peers) + v.frame_bits <= 32) {
        rc = expand_sort_offsets<uint32_t>(h, v, P, h->key32_a, h->key32_b, d_peer_offsets, d_frames_out, ctrl);
    } else {
        rc = expand_sort_offsets<uint64_t>(h, v, P, h->key64_a, h->key64_b, d_peer_offsets, d_frames_out, ctrl);
    }
    if (rc) return rc;
    if (d_counters) WQ_HIP(h, hipMemcpyAsync(d_counters, ctrl, sizeof(*ctrl), hipMemcpyDeviceToDevice, s));
    return WQ_OK;
}

}  // namespace wq
