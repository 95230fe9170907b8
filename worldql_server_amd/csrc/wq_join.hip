// wq_join.hip — ingest joins: new senders get their peer ids on the device (include/wq_router.h, "ingest
// joins"). Between the decode and the dispatch one call finds the subscribes of unknown senders, gives
// their distinct uuids ids by the caller's allocator state, patches sender / flags in place and merges the
// uuids into the handle's sender table; the leave side removes ids from that table. All arithmetic is
// join_ops.hpp. The joins' and the table's sizes are only known on the device: the passes over the frames
// have n_frames lanes, the table passes stride over the reserved room and read their bounds there.
//
//   flags    one lane per frame: candidate / unknown bits (a candidate searches the table once: its uuid
//            must be new); a wave's ballot is its granule's word
//   scan     the exclusive prefix of the words' popcounts: every granule's base, and the count c
//   compact  the candidates' key halves and frame index at their rank; the slots behind c padded
//   sort     two stable 64-bit radix passes (low half, then high half) carrying the rank; gathers between
//   heads    a sorted position opens a group of equal keys: its flag goes to its rank in frame order
//   scan     the heads in frame order: the join rank; its total is k
//   decide   one lane: k against the three limits, the counters, the go-ahead
//   scan     the heads in sorted order: a new key's rank among the new keys
//   copy     the live table to the handle's second buffer (returns at once without joins)
//   apply    one lane per frame: as a sorted position, a head writes its j_* row and its table entry; as a
//            frame, an unknown one looks its uuid up among the sorted candidates and takes the id
//   merge    the old entries move up by the new keys below them (strided; returns at once without joins)
//   finish   one lane: the live count
//
// No lane owns a uuid's frames: a uuid in every frame of the tick is one group of the sort, and every one
// of its frames finds the group's head by its own binary search.
#include <algorithm>
#include <utility>
#include <vector>

#include "join_ops.hpp"
#include "send_rows.hpp"

namespace wq {

namespace {

static_assert(sizeof(wq_join_in) == 64, "abi.JoinIn mirrors this layout");
static_assert(sizeof(wq_join_out) == 32, "abi.JoinOut mirrors this layout");
static_assert(sizeof(wq_join_counters) == 80, "abi.JOIN_COUNTERS_DTYPE mirrors this layout");
static_assert(kJnGranule == 64, "a granule is one wave64 ballot");

constexpr unsigned kJnTableBlocks = 2048;  // the strided table passes: 8 blocks of 256 per CU

// The popcount of granule g's word, 0 behind the nG granules: the terms of the rank scan.
struct JnWordTerm {
    const uint64_t* words;
    uint64_t nG;
    __host__ __device__ __forceinline__ uint32_t operator()(uint64_t g) const {
        return g < nG ? dsp_popc(words[g]) : 0u;
    }
};
// A flag per slot, 0 behind the n slots.
struct JnFlagTerm {
    const uint32_t* flag;
    uint64_t n;
    __host__ __device__ __forceinline__ uint32_t operator()(uint64_t r) const { return r < n ? flag[r] : 0u; }
};
// Whether sorted position s is a head, 0 behind the candidates (their count is read on the device).
struct JnHeadTerm {
    JnSorted s;
    const JnCtrl* ctrl;
    uint64_t n;
    __host__ __device__ __forceinline__ uint32_t operator()(uint64_t pos) const {
        return pos < n && jn_head(s, (uint32_t)pos, ctrl->n_cand) ? 1u : 0u;
    }
};

template <class F>
int scan_u32_terms(wq_router* h, const F& f, uint32_t* out, size_t n) {
    return scan_terms(h, f, out, 0u, n, rocprim::plus<uint32_t>());
}

__global__ __launch_bounds__(kBlock) void k_join_flags(wq_join_in in, uint32_t n, uint64_t* __restrict__ words,
                                                       uint8_t* __restrict__ bits, JnTable t, JnCtrl* ctrl) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t f = 0, err = 0;
    if (i < n) {
        f = jn_check_new(t, in.sender_uuid, (uint32_t)i,
                         jn_flags(in.instruction[i], in.flags[i], in.world[i], in.sender[i], &err), &err);
        bits[i] = (uint8_t)f;
    }
    const uint64_t word = __ballot((f & kJnCand) != 0), e = __ballot(err != 0);
    if ((threadIdx.x & 63u) == 0 && i < n) {
        words[i / kJnGranule] = word;
        if (e) atomicOr(reinterpret_cast<unsigned long long*>(&ctrl->c.error), (unsigned long long)kJnErrDisagree);
    }
}

__global__ __launch_bounds__(kBlock) void k_join_compact(wq_join_in in, uint32_t n, const uint64_t* __restrict__ words,
                                                         const uint32_t* __restrict__ base, uint32_t nG,
                                                         const uint8_t* __restrict__ bits, JnCand w) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = (uint32_t)(i / kJnGranule);
    jn_compact(w, in.sender_uuid, (uint32_t)i, (bits[i] & kJnCand) != 0, words[g], base[g], base[nG]);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_join_gather(const T* __restrict__ src, const uint32_t* __restrict__ idx,
                                                        T* __restrict__ dst, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

__global__ __launch_bounds__(kBlock) void k_join_sorted(JnCand w, const uint32_t* __restrict__ perm, uint64_t* __restrict__ slo,
                                                        uint32_t* __restrict__ sframe, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = perm[i];
    slo[i] = w.lo[r];
    sframe[i] = w.frame[r];
}

// hflag[perm[s]] = head(s): perm is a permutation of [0, n), so every slot is written once.
__global__ __launch_bounds__(kBlock) void k_join_heads(JnSorted s, uint32_t n, const uint32_t* __restrict__ base, uint32_t nG,
                                                       uint32_t* __restrict__ hflag) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    hflag[s.perm[i]] = jn_head(s, (uint32_t)i, base[nG]) ? 1u : 0u;
}

__global__ void k_join_decide(wq_join_in in, wq_join_out out, uint64_t n, const uint32_t* __restrict__ base, uint32_t nG,
                              const uint32_t* __restrict__ rank, JnTable t, JnCtrl* ctrl) {
    if (blockIdx.x || threadIdx.x) return;
    jn_decide(ctrl, in, out, n, n ? base[nG] : 0u, n ? rank[n] : 0u, *t.live, t.cap);
}

__global__ void k_join_no_table(uint64_t n, uint32_t id_next, JnCtrl* ctrl) {
    if (blockIdx.x || threadIdx.x) return;
    jn_no_table(ctrl, n, id_next);
}

// The live table's copy (strided over the live entries).
__global__ __launch_bounds__(kBlock) void k_join_copy(JnTable t, uint64_t* __restrict__ ohi, uint64_t* __restrict__ olo,
                                                      uint32_t* __restrict__ oid, const JnCtrl* ctrl) {
    if (!ctrl->ok || !ctrl->k) return;
    const uint32_t live = ctrl->live;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < live; e += (uint64_t)gridDim.x * kBlock)
        ohi[e] = t.hi[e], olo[e] = t.lo[e], oid[e] = t.id[e];
}

__global__ __launch_bounds__(kBlock) void k_join_apply(wq_join_in in, wq_join_out out, uint32_t n, JnSorted s,
                                                       const uint32_t* __restrict__ rank,
                                                       const uint32_t* __restrict__ heads_before,
                                                       const uint8_t* __restrict__ bits, JnTable t,
                                                       const uint64_t* __restrict__ ohi, const uint64_t* __restrict__ olo,
                                                       JnCtrl* ctrl) {
    if (!ctrl->ok || !ctrl->k) return;
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t c = ctrl->n_cand;
    bool patched = false;
    if (i < n) {
        if (jn_head(s, (uint32_t)i, c)) {  // as a sorted position
            const uint32_t r = rank[s.perm[i]];
            jn_emit(in, out, s, (uint32_t)i, r, ctrl);
            jn_merge_new(t, ohi, olo, ctrl->live, s, heads_before, (uint32_t)i, jn_join_id(in, r));
        }
        if (bits[i] & kJnUnknown) patched = jn_patch(in, s, rank, c, (uint32_t)i);  // as a frame
    }
    const uint64_t m = __ballot(patched);
    if ((threadIdx.x & 63u) == 0 && m)
        atomicAdd(reinterpret_cast<unsigned long long*>(&ctrl->c.n_patched), (unsigned long long)dsp_popc(m));
}

__global__ __launch_bounds__(kBlock) void k_join_merge(JnTable t, const uint64_t* __restrict__ ohi,
                                                       const uint64_t* __restrict__ olo, const uint32_t* __restrict__ oid,
                                                       JnSorted s, const uint32_t* __restrict__ heads_before,
                                                       const JnCtrl* ctrl) {
    if (!ctrl->ok || !ctrl->k) return;
    const uint32_t live = ctrl->live, c = ctrl->n_cand;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < live; e += (uint64_t)gridDim.x * kBlock)
        jn_merge_old(t, ohi, olo, oid, (uint32_t)e, s, heads_before, c);
}

__global__ void k_join_finish(JnTable t, const JnCtrl* ctrl) {
    if (blockIdx.x || threadIdx.x) return;
    if (ctrl->ok && ctrl->k) *t.live = ctrl->live + ctrl->k;
}

// ---- the leave side ----
__global__ __launch_bounds__(kBlock) void k_drop_flags(JnTable t, const uint32_t* __restrict__ sorted, uint32_t n,
                                                       uint64_t* __restrict__ words) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool keep = e < t.cap && jn_drop_keep(t.id, sorted, n, *t.live, (uint32_t)e);
    const uint64_t word = __ballot(keep);
    if ((threadIdx.x & 63u) == 0 && e < t.cap) words[e / kJnGranule] = word;
}

// The kept entries at their rank in the second buffer (nothing moves when nothing was removed).
__global__ __launch_bounds__(kBlock) void k_drop_scatter(JnTable t, const uint64_t* __restrict__ words,
                                                         const uint32_t* __restrict__ base, uint32_t nG,
                                                         uint64_t* __restrict__ ohi, uint64_t* __restrict__ olo,
                                                         uint32_t* __restrict__ oid) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= t.cap || base[nG] == *t.live) return;
    const uint32_t g = (uint32_t)(e / kJnGranule);
    const uint64_t word = words[g];
    if (!((word >> (e % kJnGranule)) & 1)) return;
    const uint32_t d = base[g] + dsp_popc(word & dsp_below((uint32_t)(e % kJnGranule)));
    ohi[d] = t.hi[e], olo[d] = t.lo[e], oid[d] = t.id[e];
}

__global__ __launch_bounds__(kBlock) void k_drop_back(JnTable t, const uint32_t* __restrict__ base, uint32_t nG,
                                                      const uint64_t* __restrict__ ohi, const uint64_t* __restrict__ olo,
                                                      const uint32_t* __restrict__ oid) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= base[nG] || base[nG] == *t.live) return;
    t.hi[e] = ohi[e], t.lo[e] = olo[e], t.id[e] = oid[e];
}

__global__ void k_drop_finish(JnTable t, uint64_t n, const uint32_t* __restrict__ base, uint32_t nG, JnCtrl* ctrl) {
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t live = *t.live, kept = base ? base[nG] : live;
    jn_drop_finish(ctrl, n, live, kept);
    *t.live = kept;
}

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

JnTable join_table(wq_router* h) {
    return JnTable{h->ing_phi.as<uint64_t>(), h->ing_plo.as<uint64_t>(), h->ing_pid.as<uint32_t>(), h->ing_live.as<uint32_t>(),
                   h->ing_cap};
}

// The table's second buffer: three arrays of cap entries.
int join_second(wq_router* h, uint64_t** ohi, uint64_t** olo, uint32_t** oid) {
    const size_t cap = h->ing_cap;
    WQ_ALLOC(h, h->join_tab, cap * 20 + 8);
    *ohi = h->join_tab.as<uint64_t>();
    *olo = *ohi + cap;
    *oid = reinterpret_cast<uint32_t*>(*olo + cap);
    return WQ_OK;
}

int join_counters_out(wq_router* h, wq_join_counters* d_counters) {
    if (d_counters)
        WQ_HIP(h, hipMemcpyAsync(d_counters, h->join_ctrl.p, sizeof(wq_join_counters), hipMemcpyDeviceToDevice, h->stream));
    return WQ_OK;
}

}  // namespace

void join_release(wq_router* h) {
    for (DevBuf* b : {&h->ing_live, &h->join_ws, &h->join_tab, &h->join_ctrl}) b->release();
    h->ing_cap = 0;
}

// The handle's device is current; capacity < 2^32 - 1. Waited for: the old buffers are free on return.
int ingest_peers_reserve(wq_router* h, size_t capacity) {
    hipStream_t s = h->stream;
    WQ_HIP(h, hipStreamSynchronize(s));
    uint32_t live = h->ing_n_peers;
    if (h->ing_live.p) WQ_HIP(h, hipMemcpy(&live, h->ing_live.p, 4, hipMemcpyDeviceToHost));
    size_t cap = capacity;
    if (cap < h->ing_cap) cap = h->ing_cap;
    if (cap < live) cap = live;
    DevBuf hi, lo, id;
    if (h->ing_phi.bytes < cap * 8 || h->ing_plo.bytes < cap * 8 || h->ing_pid.bytes < cap * 4) {
        WQ_ALLOC(h, hi, cap * 8);
        WQ_ALLOC(h, lo, cap * 8);
        WQ_ALLOC(h, id, cap * 4);
        if (live) {
            WQ_HIP(h, hipMemcpyAsync(hi.p, h->ing_phi.p, (size_t)live * 8, hipMemcpyDeviceToDevice, s));
            WQ_HIP(h, hipMemcpyAsync(lo.p, h->ing_plo.p, (size_t)live * 8, hipMemcpyDeviceToDevice, s));
            WQ_HIP(h, hipMemcpyAsync(id.p, h->ing_pid.p, (size_t)live * 4, hipMemcpyDeviceToDevice, s));
            WQ_HIP(h, hipStreamSynchronize(s));
        }
        std::swap(h->ing_phi, hi), std::swap(h->ing_plo, lo), std::swap(h->ing_pid, id);
        hi.release(), lo.release(), id.release();
    }
    WQ_ALLOC(h, h->ing_live, 4);
    WQ_HIP(h, hipMemcpy(h->ing_live.p, &live, 4, hipMemcpyHostToDevice));
    h->ing_cap = (uint32_t)cap;
    return WQ_OK;
}

int ingest_peers_read(wq_router* h, uint8_t* uuids, uint32_t* ids, size_t capacity, size_t* n) {
    WQ_HIP(h, hipStreamSynchronize(h->stream));
    uint32_t live = h->ing_n_peers;
    if (h->ing_live.p) WQ_HIP(h, hipMemcpy(&live, h->ing_live.p, 4, hipMemcpyDeviceToHost));
    *n = live;
    if (!uuids && !ids) return WQ_OK;
    if (capacity < live) return set_error(h, WQ_E_INVALID, "ingest_peers_read: capacity is below the live count");
    if (!live) return WQ_OK;
    if (uuids) {
        std::vector<uint64_t> hi(live), lo(live);
        WQ_HIP(h, hipMemcpy(hi.data(), h->ing_phi.p, (size_t)live * 8, hipMemcpyDeviceToHost));
        WQ_HIP(h, hipMemcpy(lo.data(), h->ing_plo.p, (size_t)live * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < live; ++i)
            for (int b = 0; b < 8; ++b) {
                uuids[16 * i + b] = (uint8_t)(hi[i] >> (56 - 8 * b));
                uuids[16 * i + 8 + b] = (uint8_t)(lo[i] >> (56 - 8 * b));
            }
    }
    if (ids) WQ_HIP(h, hipMemcpy(ids, h->ing_pid.p, (size_t)live * 4, hipMemcpyDeviceToHost));
    return WQ_OK;
}

// The call on device arrays (the handle's device is current; arguments validated, n_frames < 2^32 - 1).
int launch_ingest_join(wq_router* h, const wq_join_in* in, size_t n_frames, const wq_join_out* out,
                       wq_join_counters* d_counters) {
    hipStream_t st = h->stream;
    const uint32_t n = (uint32_t)n_frames;
    WQ_ALLOC(h, h->join_ctrl, sizeof(JnCtrl));
    JnCtrl* ctrl = h->join_ctrl.as<JnCtrl>();
    WQ_HIP(h, hipMemsetAsync(ctrl, 0, sizeof(JnCtrl), st));
    if (!h->ing_live.p) {
        hipLaunchKernelGGL(k_join_no_table, dim3(1), dim3(1), 0, st, (uint64_t)n, in->id_next, ctrl);
        WQ_HIP(h, hipGetLastError());
        return join_counters_out(h, d_counters);
    }
    const JnTable t = join_table(h);
    const size_t N = n, nG = (N + kJnGranule - 1) / kJnGranule;
    // one buffer, every array at 8-byte alignment
    const size_t o_chi = 0, o_clo = o_chi + N * 8, o_tmp = o_clo + N * 8, o_chi1 = o_tmp + N * 8, o_shi = o_chi1 + N * 8,
                 o_words = o_shi + N * 8, o_cfr = o_words + nG * 8, o_iota = o_cfr + align8(N * 4),
                 o_perm1 = o_iota + align8(N * 4), o_perm2 = o_perm1 + align8(N * 4), o_sfr = o_perm2 + align8(N * 4),
                 o_rank = o_sfr + align8(N * 4), o_hb = o_rank + align8((N + 1) * 4), o_base = o_hb + align8((N + 1) * 4),
                 o_bits = o_base + align8((nG + 1) * 4), total = o_bits + align8(N);
    WQ_ALLOC(h, h->join_ws, total);
    uint8_t* p = h->join_ws.as<uint8_t>();
    auto u64p = [&](size_t o) { return reinterpret_cast<uint64_t*>(p + o); };
    auto u32p = [&](size_t o) { return reinterpret_cast<uint32_t*>(p + o); };
    uint64_t *chi = u64p(o_chi), *clo = u64p(o_clo), *tmp = u64p(o_tmp), *chi1 = u64p(o_chi1), *shi = u64p(o_shi),
             *words = u64p(o_words);
    uint32_t *cfr = u32p(o_cfr), *iota = u32p(o_iota), *perm1 = u32p(o_perm1), *perm2 = u32p(o_perm2), *sfr = u32p(o_sfr),
             *rank = u32p(o_rank), *hb = u32p(o_hb), *base = u32p(o_base);
    uint8_t* bits = p + o_bits;
    uint64_t *ohi, *olo;
    uint32_t* oid;
    if (int rc = join_second(h, &ohi, &olo, &oid)) return rc;
    const JnCand w{chi, clo, cfr, iota};
    const JnSorted s{shi, tmp, sfr, perm2};  // tmp: the low halves' sorted copy, then the sorted low halves
    const unsigned grid = grid_for(N);
    if (n) {
        hipLaunchKernelGGL(k_join_flags, dim3(grid), dim3(kBlock), 0, st, *in, n, words, bits, t, ctrl);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_u32_terms(h, JnWordTerm{words, nG}, base, nG + 1)) return rc;
        hipLaunchKernelGGL(k_join_compact, dim3(grid), dim3(kBlock), 0, st, *in, n, words, base, (uint32_t)nG, bits, w);
        WQ_HIP(h, hipGetLastError());
        if (int rc = sort_pairs<uint64_t, uint32_t>(h, clo, tmp, iota, perm1, N, 64)) return rc;
        hipLaunchKernelGGL(k_join_gather<uint64_t>, dim3(grid), dim3(kBlock), 0, st, chi, perm1, chi1, n);
        WQ_HIP(h, hipGetLastError());
        if (int rc = sort_pairs<uint64_t, uint32_t>(h, chi1, shi, perm1, perm2, N, 64)) return rc;
        hipLaunchKernelGGL(k_join_sorted, dim3(grid), dim3(kBlock), 0, st, w, perm2, tmp, sfr, n);
        WQ_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_join_heads, dim3(grid), dim3(kBlock), 0, st, s, n, base, (uint32_t)nG, iota);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_u32_terms(h, JnFlagTerm{iota, N}, rank, N + 1)) return rc;
    }
    hipLaunchKernelGGL(k_join_decide, dim3(1), dim3(1), 0, st, *in, *out, (uint64_t)N, base, (uint32_t)nG, rank, t, ctrl);
    WQ_HIP(h, hipGetLastError());
    if (n) {
        if (int rc = scan_u32_terms(h, JnHeadTerm{s, ctrl, N}, hb, N + 1)) return rc;
        const unsigned tgrid = std::max(1u, std::min<unsigned>(kJnTableBlocks, grid_for(t.cap)));
        hipLaunchKernelGGL(k_join_copy, dim3(tgrid), dim3(kBlock), 0, st, t, ohi, olo, oid, ctrl);
        WQ_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_join_apply, dim3(grid), dim3(kBlock), 0, st, *in, *out, n, s, rank, hb, bits, t, ohi, olo, ctrl);
        WQ_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_join_merge, dim3(tgrid), dim3(kBlock), 0, st, t, ohi, olo, oid, s, hb, ctrl);
        WQ_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_join_finish, dim3(1), dim3(1), 0, st, t, ctrl);
        WQ_HIP(h, hipGetLastError());
    }
    return join_counters_out(h, d_counters);
}

// The call on a device id list (the handle's device is current; arguments validated, n < 2^32 - 1).
int launch_ingest_drop(wq_router* h, const uint32_t* d_ids, size_t n, wq_join_counters* d_counters) {
    hipStream_t st = h->stream;
    WQ_ALLOC(h, h->join_ctrl, sizeof(JnCtrl));
    JnCtrl* ctrl = h->join_ctrl.as<JnCtrl>();
    WQ_HIP(h, hipMemsetAsync(ctrl, 0, sizeof(JnCtrl), st));
    if (!h->ing_live.p) {
        hipLaunchKernelGGL(k_join_no_table, dim3(1), dim3(1), 0, st, (uint64_t)n, 0u, ctrl);
        WQ_HIP(h, hipGetLastError());
        return join_counters_out(h, d_counters);
    }
    const JnTable t = join_table(h);
    const size_t cap = t.cap, nG = (cap + kJnGranule - 1) / kJnGranule;
    const size_t o_words = 0, o_sorted = o_words + nG * 8, o_base = o_sorted + align8(n * 4),
                 total = o_base + align8((nG + 1) * 4);
    uint32_t* base = nullptr;
    if (n && cap) {
        WQ_ALLOC(h, h->join_ws, total);
        uint8_t* p = h->join_ws.as<uint8_t>();
        uint64_t* words = reinterpret_cast<uint64_t*>(p + o_words);
        uint32_t* sorted = reinterpret_cast<uint32_t*>(p + o_sorted);
        base = reinterpret_cast<uint32_t*>(p + o_base);
        uint64_t *ohi, *olo;
        uint32_t* oid;
        if (int rc = join_second(h, &ohi, &olo, &oid)) return rc;
        size_t bytes = 0;
        WQ_HIP(h, rocprim::radix_sort_keys(nullptr, bytes, d_ids, sorted, n, 0, 32, st));
        WQ_ALLOC(h, h->sort_tmp, bytes);
        WQ_HIP(h, rocprim::radix_sort_keys(h->sort_tmp.p, bytes, d_ids, sorted, n, 0, 32, st));
        const unsigned grid = grid_for(cap);
        hipLaunchKernelGGL(k_drop_flags, dim3(grid), dim3(kBlock), 0, st, t, sorted, (uint32_t)n, words);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_u32_terms(h, JnWordTerm{words, nG}, base, nG + 1)) return rc;
        hipLaunchKernelGGL(k_drop_scatter, dim3(grid), dim3(kBlock), 0, st, t, words, base, (uint32_t)nG, ohi, olo, oid);
        WQ_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_drop_back, dim3(grid), dim3(kBlock), 0, st, t, base, (uint32_t)nG, ohi, olo, oid);
        WQ_HIP(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_drop_finish, dim3(1), dim3(1), 0, st, t, (uint64_t)n, base, (uint32_t)nG, ctrl);
    WQ_HIP(h, hipGetLastError());
    return join_counters_out(h, d_counters);
}

}  // namespace wq
