// wq_leave.hip — ingest leaves: stale and disconnected senders leave on the device (include/wq_router.h,
// "ingest leaves"). One call judges every live entry of the handle's sender table against the heartbeat
// stamps and the transport's disconnect list, lists the leavers with their uuid text, writes the bitmap
// wq_remove_peers_device takes and the caller's new free list, resets the stamps and compacts the table.
// All arithmetic is leave_ops.hpp. The table's live count and the leavers' count are only known on the
// device: every table pass has one lane per reserved entry and reads its bounds there.
//
//   listed   the scratch bitmap of the listed ids (zeroed, then integer ORs)
//   flags    one lane per reserved entry: the reason bits; a wave's ballot of the leavers is its granule's word
//   scan     the exclusive prefix of the words' popcounts: every granule's base, and the count k
//   decide   one lane: k against the two limits, the counters, the go-ahead
//   apply    a leaver writes its rows at its rank, its bit, its id in the free list and its stamp; a kept
//            entry moves down by the leavers below it into the second buffer and starts its clock
//   back     the kept entries return to the table; one lane writes the live count
//   free     the caller's free list behind the leavers' ids
//
// No lane owns a peer, placement comes from the scan alone, and the only atomics are integer ORs into the
// two bitmaps and integer adds / ORs into the counters.
#include <algorithm>

#include "leave_ops.hpp"
#include "send_rows.hpp"

namespace wq {

namespace {

static_assert(sizeof(wq_leave_in) == 56, "abi.LeaveIn mirrors this layout");
static_assert(sizeof(wq_leave_out) == 64, "abi.LeaveOut mirrors this layout");
static_assert(sizeof(wq_leave_counters) == 80, "abi.LEAVE_COUNTERS_DTYPE mirrors this layout");
static_assert(kJnGranule == 64, "a granule is one wave64 ballot");

// The popcount of granule g's word, 0 behind the nG granules: the terms of the rank scan.
struct LvWordTerm {
    const uint64_t* words;
    uint64_t nG;
    __host__ __device__ __forceinline__ uint32_t operator()(uint64_t g) const {
        return g < nG ? dsp_popc(words[g]) : 0u;
    }
};

__device__ __forceinline__ void lv_add(uint64_t* p, uint64_t v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

__global__ __launch_bounds__(kBlock) void k_leave_listed(wq_leave_in in, uint32_t* __restrict__ listed) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= in.n_leave) return;
    const uint32_t id = in.leave_ids[i];
    if (id < in.n_ids) atomicOr(&listed[id >> 5], 1u << (id & 31u));
}

__global__ __launch_bounds__(kBlock) void k_leave_flags(wq_leave_in in, JnTable t, const uint32_t* __restrict__ listed,
                                                        uint8_t* __restrict__ reason, uint64_t* __restrict__ words,
                                                        LvCtrl* ctrl) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t r = 0, err = 0;
    if (e < t.cap) {
        if (e < *t.live) r = lv_reason(in, listed, t.id[e], &err);
        reason[e] = (uint8_t)r;
    }
    const uint64_t word = __ballot(r != 0), wl = __ballot((r & kLvListed) != 0), ws = __ballot((r & kLvStale) != 0),
                   we = __ballot(err != 0);
    if ((threadIdx.x & 63u) == 0 && e < t.cap) {
        words[e / kJnGranule] = word;
        lv_add(&ctrl->c.n_listed_found, dsp_popc(wl));
        lv_add(&ctrl->c.n_stale, dsp_popc(ws));
        if (we) atomicOr(reinterpret_cast<unsigned long long*>(&ctrl->c.error), (unsigned long long)kLvErrIdRange);
    }
}

__global__ void k_leave_decide(wq_leave_in in, wq_leave_out out, JnTable t, const uint32_t* __restrict__ base, uint32_t nG,
                               LvCtrl* ctrl) {
    if (blockIdx.x || threadIdx.x) return;
    lv_decide(ctrl, in, out, base[nG], *t.live);
}

__global__ void k_leave_no_table(wq_leave_in in, LvCtrl* ctrl) {
    if (blockIdx.x || threadIdx.x) return;
    lv_no_table(ctrl, in);
}

__global__ __launch_bounds__(kBlock) void k_leave_apply(wq_leave_in in, wq_leave_out out, JnTable t,
                                                        const uint8_t* __restrict__ reason,
                                                        const uint64_t* __restrict__ words, const uint32_t* __restrict__ base,
                                                        uint64_t* __restrict__ ohi, uint64_t* __restrict__ olo,
                                                        uint32_t* __restrict__ oid, LvCtrl* ctrl) {
    if (!ctrl->ok) return;
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t k = ctrl->k;
    bool stamped = false;
    if (e < ctrl->live) {
        const uint32_t g = (uint32_t)(e / kJnGranule), lane = (uint32_t)(e % kJnGranule);
        const uint64_t word = words[g];
        const uint32_t below = base[g] + dsp_popc(word & dsp_below(lane));
        if ((word >> lane) & 1ull) {
            const uint32_t id = t.id[e];
            lv_emit(in, out, t, (uint32_t)e, below, reason[e], k);
            if (out.gone_bits) atomicOr(&out.gone_bits[id >> 5], 1u << (id & 31u));
        } else {
            stamped = lv_keep(in, t, (uint32_t)e, below, k != 0, ohi, olo, oid);
        }
    }
    const uint64_t m = __ballot(stamped);
    if ((threadIdx.x & 63u) == 0) lv_add(&ctrl->c.n_stamped, dsp_popc(m));
}

__global__ __launch_bounds__(kBlock) void k_leave_back(JnTable t, const uint64_t* __restrict__ ohi,
                                                       const uint64_t* __restrict__ olo, const uint32_t* __restrict__ oid,
                                                       const LvCtrl* ctrl) {
    if (!ctrl->ok || !ctrl->k) return;
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t kept = ctrl->live - ctrl->k;
    if (e < kept) t.hi[e] = ohi[e], t.lo[e] = olo[e], t.id[e] = oid[e];
    if (e == 0) *t.live = kept;  // no lane of this pass reads the word
}

__global__ __launch_bounds__(kBlock) void k_leave_free(wq_leave_in in, wq_leave_out out, const LvCtrl* ctrl) {
    if (!ctrl->ok) return;
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < in.n_free) lv_free_tail(in, out, ctrl->k, (uint32_t)j);
}

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

void leave_release(wq_router* h) {
    for (DevBuf* b : {&h->leave_ws, &h->leave_ctrl}) b->release();
}

// The call on device arrays (the handle's device is current; arguments validated).
int launch_ingest_leave(wq_router* h, const wq_leave_in* in, const wq_leave_out* out, wq_leave_counters* d_counters) {
    hipStream_t st = h->stream;
    WQ_ALLOC(h, h->leave_ctrl, sizeof(LvCtrl));
    LvCtrl* ctrl = h->leave_ctrl.as<LvCtrl>();
    WQ_HIP(h, hipMemsetAsync(ctrl, 0, sizeof(LvCtrl), st));
    const size_t n_words = ((size_t)in->n_ids + 31) / 32;
    if (out->gone_bits && n_words) WQ_HIP(h, hipMemsetAsync(out->gone_bits, 0, n_words * 4, st));
    auto counters_out = [&]() -> int {
        if (d_counters)
            WQ_HIP(h, hipMemcpyAsync(d_counters, ctrl, sizeof(wq_leave_counters), hipMemcpyDeviceToDevice, st));
        return WQ_OK;
    };
    if (!h->ing_live.p) {
        hipLaunchKernelGGL(k_leave_no_table, dim3(1), dim3(1), 0, st, *in, ctrl);
        WQ_HIP(h, hipGetLastError());
        return counters_out();
    }
    const JnTable t{h->ing_phi.as<uint64_t>(), h->ing_plo.as<uint64_t>(), h->ing_pid.as<uint32_t>(), h->ing_live.as<uint32_t>(),
                    h->ing_cap};
    const size_t cap = t.cap, nG = (cap + kJnGranule - 1) / kJnGranule;
    // one buffer, every array at 8-byte alignment; the table's second buffer is the join's
    const size_t o_words = 0, o_base = o_words + nG * 8, o_listed = o_base + align8((nG + 1) * 4),
                 o_reason = o_listed + align8(n_words * 4), total = o_reason + align8(cap);
    WQ_ALLOC(h, h->leave_ws, total + 8);
    WQ_ALLOC(h, h->join_tab, cap * 20 + 8);
    uint8_t* p = h->leave_ws.as<uint8_t>();
    uint64_t* words = reinterpret_cast<uint64_t*>(p + o_words);
    uint32_t* base = reinterpret_cast<uint32_t*>(p + o_base);
    uint32_t* listed = reinterpret_cast<uint32_t*>(p + o_listed);
    uint8_t* reason = p + o_reason;
    uint64_t *ohi = h->join_tab.as<uint64_t>(), *olo = ohi + cap;
    uint32_t* oid = reinterpret_cast<uint32_t*>(olo + cap);
    if (in->n_leave) {
        if (n_words) WQ_HIP(h, hipMemsetAsync(listed, 0, n_words * 4, st));
        hipLaunchKernelGGL(k_leave_listed, dim3(grid_for(in->n_leave)), dim3(kBlock), 0, st, *in, listed);
        WQ_HIP(h, hipGetLastError());
    }
    const unsigned grid = std::max(1u, grid_for(cap));
    if (cap) {
        hipLaunchKernelGGL(k_leave_flags, dim3(grid), dim3(kBlock), 0, st, *in, t, in->n_leave ? listed : nullptr, reason, words,
                           ctrl);
        WQ_HIP(h, hipGetLastError());
    }
    if (int rc = scan_terms(h, LvWordTerm{words, nG}, base, 0u, nG + 1, rocprim::plus<uint32_t>())) return rc;
    hipLaunchKernelGGL(k_leave_decide, dim3(1), dim3(1), 0, st, *in, *out, t, base, (uint32_t)nG, ctrl);
    WQ_HIP(h, hipGetLastError());
    if (cap) {
        hipLaunchKernelGGL(k_leave_apply, dim3(grid), dim3(kBlock), 0, st, *in, *out, t, reason, words, base, ohi, olo, oid, ctrl);
        WQ_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_leave_back, dim3(grid), dim3(kBlock), 0, st, t, ohi, olo, oid, ctrl);
        WQ_HIP(h, hipGetLastError());
    }
    if (out->free_out && in->n_free) {
        hipLaunchKernelGGL(k_leave_free, dim3(grid_for(in->n_free)), dim3(kBlock), 0, st, *in, *out, ctrl);
        WQ_HIP(h, hipGetLastError());
    }
    return counters_out();
}

}  // namespace wq
