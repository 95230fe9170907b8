// wq_csr_diff.hip — interest changes: who entered and who left each row between two ticks.
//
// Two CSRs over the same rows (the old tick and the new one, peers ascending and distinct within a
// row, as wq_route_tick* writes them) give two more: entered = new \ old and left = old \ new, row by
// row. An extension the reference does not have (it routes and forgets: local_message.rs:52-86).
//
//   rows    one lane per row: the clamped lengths of both sides (csr_diff_ops.hpp diff_row_bounds)
//   scan    their exclusive prefix: each side's ordinal space, monotone whatever the offsets hold
//   flag    element-parallel: a wave per granule of 64 ordinals; every lane finds its row (a search
//           narrowed to the rows the granule touches), searches its element in the other side's
//           row and the wave's ballot is the granule's flag word, its popcount the granule's count
//   scan    exclusive prefix of the granule counts
//   emit    a wave per granule with a flag bit set stores its kept elements as one contiguous run
//           at the granule's prefix; one lane per row derives the row's output offset from the same
//           prefix and the flag word (diff_kept_before); the lane of row n_rows writes the counters
//
// No lane, wave or block owns a row: a row of any length is spread over ceil(len / 64) granules, and
// the granules over a grid sized from the capacities (the totals are read on the device). Placement
// comes from the two prefix sums alone, so the output is the same bytes every time.
#include "csr_diff_ops.hpp"
#include "table_prims.hpp"

namespace wq {

namespace {

constexpr int kDiffWaves = kBlock / 64;
constexpr unsigned kDiffMaxBlocks = 4096;  // 16 blocks of 256 per CU: the persistent grids' size

__global__ __launch_bounds__(kBlock) void k_diff_rows(DiffSide nw, DiffSide od, uint32_t M, DiffPair* len,
                                                      uint32_t* err_cur, uint32_t* err_nxt) {
    const uint32_t m = blockIdx.x * kBlock + threadIdx.x;
    if (m == 0) *err_nxt = 0;  // the next call's slot (this call's was zeroed by the previous one)
    if (m > M) return;
    if (m == M) {
        len[m] = DiffPair{0, 0};
        return;
    }
    uint32_t a, b, c, d;
    const bool ok_n = diff_row_bounds(nw.off, m, nw.cap, a, b);
    const bool ok_o = diff_row_bounds(od.off, m, od.cap, c, d);
    len[m] = DiffPair{b - a, d - c};
    if (!(ok_n && ok_o)) atomicOr(err_cur, kDiffErrRows);
}

// The rows [rlo, rhi] that the granule starting at ordinal q0 touches (T: the side's total, q0 < T):
// lane 0 searches the first ordinal's row and lane 63 the last one's, among all M rows (the other
// lanes repeat lane 0's search: the same addresses, one request). A 64-way search by the whole wave
// (64 spaced probes and a ballot per step, 8 dependent steps instead of 24 at 10M rows) was
// measured and is twice as slow on C3: its 64 distinct lines per step cost more than the latency
// they save.
__device__ __forceinline__ void granule_rows(const uint32_t* __restrict__ pre, int side, uint32_t M, uint32_t T,
                                             uint32_t q0, uint32_t lane, uint32_t& rlo, uint32_t& rhi) {
    const uint32_t last = T - q0 > kDiffGranule ? q0 + kDiffGranule - 1 : T - 1;
    const uint32_t r = diff_row_of(pre, side, 0, M - 1, lane == 63 ? last : q0);
    rlo = __shfl(r, 0);
    rhi = __shfl(r, 63);
}

__device__ __forceinline__ void flag_side(const DiffSide& src, const DiffSide& oth, const uint32_t* __restrict__ pre,
                                          int side, uint32_t M, uint32_t T, uint32_t nG, uint64_t* flags,
                                          uint32_t* cnt, uint32_t wave, uint32_t n_waves, uint32_t lane) {
    for (uint32_t g = wave; g < nG; g += n_waves) {
        const uint64_t q0 = (uint64_t)g * kDiffGranule;
        uint64_t word = 0;
        if (q0 < T) {  // wave-uniform
            uint32_t rlo, rhi;
            granule_rows(pre, side, M, T, (uint32_t)q0, lane, rlo, rhi);
            const uint32_t q = (uint32_t)q0 + lane;
            const bool keep = q < T && diff_keeps(src, oth, pre, side, rlo, rhi, q);
            word = __ballot(keep);
            if (lane == 0) flags[g] = word;
        }
        if (lane == 0) cnt[2ull * g + side] = (uint32_t)__popcll(word);
    }
}

__global__ __launch_bounds__(kBlock) void k_diff_flag(DiffSide nw, DiffSide od, const uint32_t* __restrict__ pre,
                                                      uint32_t M, uint32_t lim_n, uint32_t lim_o, uint32_t nG,
                                                      uint64_t* flags_e, uint64_t* flags_l, uint32_t* cnt) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * kDiffWaves + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * kDiffWaves;
    const uint32_t tn = pre[2ull * M] < lim_n ? pre[2ull * M] : lim_n;
    const uint32_t to = pre[2ull * M + 1] < lim_o ? pre[2ull * M + 1] : lim_o;  // lim_o == 0: left side off
    flag_side(nw, od, pre, 0, M, tn, nG, flags_e, cnt, wave, n_waves, lane);
    flag_side(od, nw, pre, 1, M, to, nG, flags_l, cnt, wave, n_waves, lane);
}

__device__ __forceinline__ void emit_side(const DiffSide& src, const uint32_t* __restrict__ pre, int side, uint32_t M,
                                          uint32_t T, const uint64_t* __restrict__ flags,
                                          const uint32_t* __restrict__ base, uint32_t* out, uint32_t out_cap,
                                          uint32_t wave, uint32_t n_waves, uint32_t lane) {
    const uint32_t nGs = T / kDiffGranule + (T % kDiffGranule ? 1u : 0u);
    for (uint32_t g = wave; g < nGs; g += n_waves) {
        const uint64_t word = flags[g];
        if (!word) continue;  // wave-uniform
        const uint32_t q0 = g * kDiffGranule;
        uint32_t rlo, rhi;
        granule_rows(pre, side, M, T, q0, lane, rlo, rhi);
        if ((word >> lane) & 1ull) {
            uint32_t m;
            bool ok;
            const uint32_t j = diff_source(src, pre, side, rlo, rhi, q0 + lane, &m, &ok);
            // the kept lanes' positions are consecutive: one contiguous run per wave
            const uint32_t pos = base[2ull * g + side] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
            if (ok && pos < out_cap) out[pos] = src.peers[j];
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_diff_emit(DiffSide nw, DiffSide od, const uint32_t* __restrict__ pre,
                                                      uint32_t M, uint32_t lim_n, uint32_t lim_o,
                                                      const uint64_t* __restrict__ flags_e,
                                                      const uint64_t* __restrict__ flags_l,
                                                      const uint32_t* __restrict__ base, uint32_t* ent_off,
                                                      uint32_t* ent_peers, uint32_t ent_cap, uint32_t* left_off,
                                                      uint32_t* left_peers, uint32_t left_cap,
                                                      const uint32_t* __restrict__ err_cur, wq_diff_counters* counters,
                                                      wq_diff_counters* counters2) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * kDiffWaves + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * kDiffWaves;
    const uint32_t tn = pre[2ull * M] < lim_n ? pre[2ull * M] : lim_n;
    const uint32_t to = pre[2ull * M + 1] < lim_o ? pre[2ull * M + 1] : lim_o;
    emit_side(nw, pre, 0, M, tn, flags_e, base, ent_peers, ent_cap, wave, n_waves, lane);
    if (left_off) emit_side(od, pre, 1, M, to, flags_l, base, left_peers, left_cap, wave, n_waves, lane);
    // the rows' output offsets, [M + 1] from 0: the kept elements before each row's first ordinal
    const uint64_t n_threads = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i <= M; i += n_threads) {
        const uint32_t pn = pre[2 * i] < tn ? pre[2 * i] : tn;
        const uint32_t e = diff_kept_before(base, flags_e, 0, pn);
        ent_off[i] = e;
        uint32_t l = 0;
        if (left_off) {
            const uint32_t po = pre[2 * i + 1] < to ? pre[2 * i + 1] : to;
            l = diff_kept_before(base, flags_l, 1, po);
            left_off[i] = l;
        }
        if (i == M) {
            wq_diff_counters c;
            c.n_entered = e;
            c.n_left = l;
            c.overflow = (e > ent_cap ? 1u : 0u) | (l > left_cap ? 2u : 0u);
            c.error = *err_cur;
            if (counters) *counters = c;
            if (counters2) *counters2 = c;
        }
    }
}

int scan_pairs(wq_router* h, const DiffPair* in, DiffPair* out, size_t n) {
    size_t bytes = 0;
    WQ_HIP(h, rocprim::exclusive_scan(nullptr, bytes, in, out, DiffPair{0, 0}, n, DiffSatAdd(), h->stream));
    WQ_ALLOC(h, h->sort_tmp, bytes);
    WQ_HIP(h, rocprim::exclusive_scan(h->sort_tmp.p, bytes, in, out, DiffPair{0, 0}, n, DiffSatAdd(), h->stream));
    return WQ_OK;
}

}  // namespace

void csr_diff_release(wq_router* h) {
    for (DevBuf* b : {&h->diff_len, &h->diff_pre, &h->diff_cnt, &h->diff_base, &h->diff_flags, &h->diff_err})
        b->release();
}

// The call on device arrays (the handle's device is current; arguments validated, capacities
// <= 2^32 - 1). own: a second copy of the counters in the handle's scratch (the host form reads it).
int launch_csr_diff(wq_router* h, size_t n_rows, const uint32_t* d_old_offsets, const uint32_t* d_old_peers,
                    size_t old_capacity, const uint32_t* d_new_offsets, const uint32_t* d_new_peers,
                    size_t new_capacity, uint32_t* d_ent_offsets, uint32_t* d_ent_peers, size_t ent_capacity,
                    uint32_t* d_left_offsets, uint32_t* d_left_peers, size_t left_capacity,
                    wq_diff_counters* d_counters, bool own) {
    hipStream_t s = h->stream;
    const uint32_t M = (uint32_t)n_rows;
    const uint32_t lim_n = diff_limit(new_capacity);
    const uint32_t lim_o = d_left_offsets ? diff_limit(old_capacity) : 0u;
    const uint32_t gn = lim_n / kDiffGranule, go = lim_o / kDiffGranule;
    const uint32_t nG = std::max(gn, go) + 1;  // + 1: the exclusive prefix's last entry is the total
    WQ_ALLOC(h, h->diff_len, ((size_t)M + 1) * sizeof(DiffPair));
    WQ_ALLOC(h, h->diff_pre, ((size_t)M + 1) * sizeof(DiffPair));
    WQ_ALLOC(h, h->diff_cnt, (size_t)nG * sizeof(DiffPair));
    WQ_ALLOC(h, h->diff_base, (size_t)nG * sizeof(DiffPair));
    WQ_ALLOC(h, h->diff_flags, ((size_t)gn + go + 1) * 8);
    if (!h->diff_err.p) {  // once per handle: two error slots (each call zeroes the next call's), the own counters
        WQ_ALLOC(h, h->diff_err, 64);
        WQ_HIP(h, hipMemsetAsync(h->diff_err.p, 0, 64, s));
    }
    uint32_t* err = h->diff_err.as<uint32_t>();
    uint32_t* err_cur = err + (h->diff_calls & 1u);
    uint32_t* err_nxt = err + ((h->diff_calls + 1) & 1u);
    h->diff_calls++;
    wq_diff_counters* mine = own ? reinterpret_cast<wq_diff_counters*>(err + 4) : nullptr;

    const DiffSide nw{d_new_offsets, d_new_peers, (uint32_t)new_capacity};
    const DiffSide od{d_old_offsets, d_old_peers, (uint32_t)old_capacity};
    DiffPair* len = h->diff_len.as<DiffPair>();
    DiffPair* pre = h->diff_pre.as<DiffPair>();
    DiffPair* cnt = h->diff_cnt.as<DiffPair>();
    DiffPair* base = h->diff_base.as<DiffPair>();
    uint64_t* flags_e = h->diff_flags.as<uint64_t>();
    uint64_t* flags_l = flags_e + gn;

    hipLaunchKernelGGL(k_diff_rows, dim3(grid_for((uint64_t)M + 1)), dim3(kBlock), 0, s, nw, od, M, len, err_cur,
                       err_nxt);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_pairs(h, len, pre, (size_t)M + 1)) return rc;
    const unsigned grid_g = std::min<unsigned>(kDiffMaxBlocks, (nG + kDiffWaves - 1) / kDiffWaves);
    hipLaunchKernelGGL(k_diff_flag, dim3(grid_g), dim3(kBlock), 0, s, nw, od, reinterpret_cast<const uint32_t*>(pre), M,
                       lim_n, lim_o, nG, flags_e, flags_l, reinterpret_cast<uint32_t*>(cnt));
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_pairs(h, cnt, base, nG)) return rc;
    const unsigned grid_e = std::min<unsigned>(kDiffMaxBlocks, std::max(grid_g, grid_for((uint64_t)M + 1)));
    hipLaunchKernelGGL(k_diff_emit, dim3(grid_e), dim3(kBlock), 0, s, nw, od, reinterpret_cast<const uint32_t*>(pre), M,
                       lim_n, lim_o, flags_e, flags_l, reinterpret_cast<const uint32_t*>(base), d_ent_offsets,
                       d_ent_peers, (uint32_t)ent_capacity, d_left_offsets, d_left_peers, (uint32_t)left_capacity,
                       err_cur, d_counters, mine);
    WQ_HIP(h, hipGetLastError());
    return WQ_OK;
}

}  // namespace wq
