// wq_rotate.hip — the fair share: rotate what the budgets cut so every entity arrives.
//
// Both budgets keep the nearest messages of every peer's list. Here a second, small share of the
// connection's budget goes to the cut elements that follow the peer's cursor, a message index, in
// cyclic order of message index; the output is the kept and the chosen elements in the full row's
// order, and the cursor moves to the last chosen one (include/wq_router.h, wq_peer_rotate_device).
// The state is one u32 per peer.
//
//   rows    one lane per peer: the clamped lengths of the full and the kept row; two saturating scans
//           give both ordinal spaces (send_rows.hpp); a second lane per peer: P, the upper bound of
//           the cursor in the full row (a binary search)
//   cut     a wave per granule of 64 ordinals: the element's row (a search over the prefix), its
//           occurrence index, its value's lower and upper bound in the kept row, the ballot of "cut";
//           a u32 scan of the granules' counts and, with sizes, a u64 scan of cut flag * size
//   rowq    one lane per peer: the scans at s, P and e folded into RotRow (rotate_ops.hpp)
//   keep    a wave per granule: not cut, or chosen by rank and running bytes; the ballot; scan
//   offsets one lane per peer: the kept bits before s, the chosen count, rows_rotated / rows_behind;
//           with sizes a u64 scan of keep flag * size gives d_out_bytes and bytes_out
//   emit    every kept ordinal stores its message at the granule's prefix plus the kept bits below it;
//           the chosen element of the largest rank stores its message into the cursor
//
// No lane, wave or block walks a row. Placement comes from prefix sums alone; the atomics are integer
// adds and ORs into counters, so the output is the same bytes every time. The adds of a block or wave
// go to one of kRotParts slots by its index and the counters kernel sums the slots: tens of thousands
// of adds to one address cost more than the rest of the call. The cursors are read in
// `rows` and written by `emit`, the call's last kernel.
#include "rotate_ops.hpp"
#include "send_rows.hpp"

namespace wq {

namespace {

static_assert(kRotTile == kBlock && kRotGranule == 64, "a block sums one tile, a wave ballots one granule");

struct RotIn {
    const uint32_t* off;
    const uint32_t* msgs;
    const uint32_t* koff;
    const uint32_t* kmsgs;
    const uint32_t* msize;  // nullptr: count share only
    const uint32_t* extra;
    const uint64_t* extra_bytes;
    uint32_t n_peers, n_in, n_kin, n_msgs, r;
    uint64_t v;
};

struct RotWs {
    uint32_t* len;    // [n_peers + 1] clamped lengths of the full rows, then the rows' chosen counts
    uint32_t* sum;    // [n_peers + 1] their saturating prefix
    uint32_t* pre;    // [n_peers + 1] the prefix clamped to n_in: the ordinal space
    uint32_t* klen;   // the same three for the kept CSR
    uint32_t* ksum;
    uint32_t* kpre;
    RotRow* rrow;     // [n_peers]
    uint32_t* row;    // [n_in]
    uint32_t* size;   // [n_in], with sizes
    uint64_t* scan;   // [n_in + 1], with sizes: cut flag * size, then keep flag * size
    uint64_t* words;  // [2 * nG] cut flags, keep flags
    uint32_t* cnt;    // [2 * nG]
    uint32_t* base;   // [2 * nG]
    uint32_t* ctrl;   // {-, error}
    RotPart* part;    // [kRotParts] partial sums of bytes_chosen, rows_rotated, rows_behind; zero at the start
};

// The ordinal spaces of the full and of the kept CSR.
__device__ __forceinline__ RowSpace rot_full(const RotIn& in, const RotWs& ws) {
    return RowSpace{in.off, in.n_peers, in.n_in, ws.len, ws.sum, ws.pre};
}
__device__ __forceinline__ RowSpace rot_kept(const RotIn& in, const RotWs& ws) {
    return RowSpace{in.koff, in.n_peers, in.n_kin, ws.klen, ws.ksum, ws.kpre};
}

__global__ __launch_bounds__(kBlock) void k_rot_len(RotIn in, RotWs ws) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > in.n_peers) return;
    rows_len_step(rot_full(in, ws), p, &ws.ctrl[1], kRotErrRows);
    rows_len_step(rot_kept(in, ws), p, &ws.ctrl[1], kRotErrRows);
}

__global__ __launch_bounds__(kBlock) void k_rot_pre(RotIn in, RotWs ws, const uint32_t* __restrict__ cursor) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > in.n_peers) return;
    uint32_t len, klen;
    const uint32_t a = rows_pre_step(rot_full(in, ws), p, &ws.ctrl[1], kRotErrRows, &len);
    rows_pre_step(rot_kept(in, ws), p, &ws.ctrl[1], kRotErrRows, &klen);
    if (p == in.n_peers) return;
    ws.rrow[p].P = a + rot_upper(in.msgs + bud_row_start(in.off, (uint32_t)p, in.n_in), len, cursor[p]);
}

__global__ __launch_bounds__(kBlock) void k_rot_cut(RotIn in, RotWs ws, uint32_t nG) {
    const uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t g = (uint32_t)(x >> 6);
    if (g >= nG) return;  // wave-uniform
    bool cut = false;
    if (x < ws.pre[in.n_peers]) {
        const uint32_t p = bud_row_of(ws.pre, in.n_peers, (uint32_t)x);
        const uint32_t i = (uint32_t)x - ws.pre[p];
        const uint32_t* row = in.msgs + bud_row_start(in.off, p, in.n_in);
        const uint32_t m = row[i];
        const uint32_t* krow = in.kmsgs + bud_row_start(in.koff, p, in.n_kin);
        cut = rot_is_cut(krow, ws.kpre[p + 1] - ws.kpre[p], m, rot_occurrence(row, i));
        ws.row[x] = p;
        if (in.msize) {
            ws.size[x] = bud_size(in.msize, in.n_msgs, m);
            if (m >= in.n_msgs) atomicOr(&ws.ctrl[1], kRotErrMsg);
        }
    }
    store_flags(ws.words, ws.cnt, g, cut);
}

__global__ __launch_bounds__(kBlock) void k_rot_rowq(RotIn in, RotWs ws) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= in.n_peers) return;
    const uint32_t s = ws.pre[p], e = ws.pre[p + 1], P = ws.rrow[p].P;
    const uint32_t Cs = bud_before(ws.base, ws.words, s), CP = bud_before(ws.base, ws.words, P),
                   Ce = bud_before(ws.base, ws.words, e);
    ws.rrow[p] = in.msize ? rot_row(P, Cs, CP, Ce, ws.scan[s], ws.scan[P], ws.scan[e])
                          : rot_row(P, Cs, CP, Ce, 0, 0, 0);
}

__global__ __launch_bounds__(kBlock) void k_rot_keep(RotIn in, RotWs ws, uint32_t nG) {
    __shared__ unsigned long long wave_bytes[kBlock / 64];
    const uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t g = (uint32_t)(x >> 6);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool f = false;
    unsigned long long mine = 0;
    if (g < nG && x < ws.pre[in.n_peers]) {
        f = true;
        if (flag_at(ws.words, x)) {
            const uint32_t p = ws.row[x];
            const RotRow r = ws.rrow[p];
            const uint32_t rank = rot_rank(r, (uint32_t)x, bud_before(ws.base, ws.words, (uint32_t)x));
            const uint32_t sz = in.msize ? ws.size[x] : 0u;
            const uint64_t bytes = in.msize ? rot_bytes(r, (uint32_t)x, ws.scan[x], sz) : 0ull;
            f = rot_chosen(rank, bytes, rot_share(in.extra, in.r, p), in.msize != nullptr,
                           rot_share_bytes(in.extra_bytes, in.v, p));
            if (f) mine = sz;
        }
    }
    if (g < nG) store_flags(ws.words, ws.cnt, (uint64_t)nG + g, f);  // wave-uniform
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_down(mine, d);
    if (lane == 0) wave_bytes[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = 0;
        for (uint32_t w = 0; w < kBlock / 64; ++w) tot += wave_bytes[w];
        if (tot) atomicAdd(&ws.part[blockIdx.x & (kRotParts - 1u)].bytes_chosen, tot);
    }
}

// ws.scan: the scan of the kept sizes when out_bytes is given.
__global__ __launch_bounds__(kBlock) void k_rot_offsets(RotIn in, RotWs ws, uint32_t nG, uint32_t* __restrict__ out_off,
                                                         uint64_t* __restrict__ out_bytes) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool rotated = false, behind = false;
    if (p <= in.n_peers) {
        const uint32_t s = ws.pre[p];
        const uint32_t o = bud_before(ws.base + nG, ws.words + nG, s);
        out_off[p] = o;
        if (p < in.n_peers) {
            const uint32_t e = ws.pre[p + 1];
            const uint32_t n_cut = ws.rrow[p].n_cut;
            const uint32_t n = rot_n_chosen(bud_before(ws.base + nG, ws.words + nG, e) - o, e - s, n_cut);
            ws.len[p] = n;
            rotated = n > 0;
            behind = n < n_cut;
            if (out_bytes) out_bytes[p] = ws.scan[e] - ws.scan[s];
        }
    }
    const uint32_t n_rot = (uint32_t)__popcll(__ballot(rotated)), n_beh = (uint32_t)__popcll(__ballot(behind));
    if ((threadIdx.x & 63u) == 0) {
        RotPart* part = ws.part + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kRotParts - 1u));
        if (n_rot) atomicAdd(&part->rows_rotated, n_rot);
        if (n_beh) atomicAdd(&part->rows_behind, n_beh);
    }
}

// One wave: lane l sums the slots l, l + 64, ...; kept_scan: the scan of the kept sizes, NULL without sizes.
__global__ __launch_bounds__(64) void k_rot_counters(RotWs ws, uint32_t n_peers, const uint32_t* __restrict__ out_off,
                                                     const uint64_t* __restrict__ kept_scan,
                                                     wq_rotate_counters* counters) {
    unsigned long long bytes = 0;
    uint32_t n_rot = 0, n_beh = 0;
    for (uint32_t i = threadIdx.x; i < kRotParts; i += 64) {
        bytes += ws.part[i].bytes_chosen;
        n_rot += ws.part[i].rows_rotated;
        n_beh += ws.part[i].rows_behind;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        bytes += __shfl_down(bytes, d);
        n_rot += __shfl_down(n_rot, d);
        n_beh += __shfl_down(n_beh, d);
    }
    if (threadIdx.x != 0) return;
    const uint32_t T = ws.pre[n_peers];
    wq_rotate_counters c;
    c.n_in = T;
    c.n_kept_in = T - bud_before(ws.base, ws.words, T);
    c.n_out = out_off[n_peers];
    c.n_chosen = c.n_out - c.n_kept_in;
    c.bytes_chosen = bytes;
    c.bytes_out = kept_scan ? kept_scan[T] : 0ull;
    c.rows_rotated = n_rot;
    c.rows_behind = n_beh;
    c.error = ws.ctrl[1] | rot_kept_error(c.n_kept_in, ws.kpre[n_peers]);
    c.pad_ = 0;
    *counters = c;
}

__global__ __launch_bounds__(kBlock) void k_rot_emit(RotIn in, RotWs ws, uint32_t nG, uint32_t* __restrict__ out,
                                                      uint32_t* __restrict__ cursor) {
    const uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (x >= ws.pre[in.n_peers]) return;
    const uint64_t* keep = ws.words + nG;
    if (!flag_at(keep, x)) return;
    const uint32_t p = ws.row[x];
    const uint32_t m = in.msgs[rows_elem(in.off, ws.pre, in.n_in, p, (uint32_t)x)];
    const uint32_t pos = bud_before(ws.base + nG, keep, (uint32_t)x);
    if (pos < in.n_in) out[pos] = m;
    if (flag_at(ws.words, x)) {  // chosen: the one of the largest rank moves the cursor
        const uint32_t rank = rot_rank(ws.rrow[p], (uint32_t)x, bud_before(ws.base, ws.words, (uint32_t)x));
        if (rank + 1 == ws.len[p]) cursor[p] = m;
    }
}

}  // namespace

void rotate_release(wq_router* h) {
    for (DevBuf* b : {&h->rot_len, &h->rot_sum, &h->rot_pre, &h->rot_rows, &h->rot_part}) b->release();
}

// The call on device arrays (the handle's device is current; arguments validated). The full CSR's
// ordinal space (send_rows.hpp rows_alloc), the per-ordinal row and size, the u64 scan, the flag
// words and ctrl are the budgets' buffers: the calls are ordered on the handle's stream and nothing
// in them outlives a call. The kept CSR's ordinal space, RotRow and the counters' slots are this
// path's own.
int launch_peer_rotate(wq_router* h, const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers,
                       size_t n_in, const uint32_t* d_kept_offsets, const uint32_t* d_kept_msgs, size_t n_kept_in,
                       const uint32_t* d_msg_size, size_t n_msgs, uint32_t r, const uint32_t* d_extra, uint64_t v,
                       const uint64_t* d_extra_bytes, uint32_t* d_cursor, uint32_t* d_out_offsets,
                       uint32_t* d_out_msgs, uint64_t* d_out_bytes, wq_rotate_counters* d_counters) {
    hipStream_t s = h->stream;
    const size_t rows = (size_t)n_peers + 1;
    const uint32_t nG = (uint32_t)(n_in / 64 + 1);
    if (int rc = rows_alloc(h, rows)) return rc;
    WQ_ALLOC(h, h->rot_len, rows * 4);
    WQ_ALLOC(h, h->rot_sum, rows * 4);
    WQ_ALLOC(h, h->rot_pre, rows * 4);
    WQ_ALLOC(h, h->rot_rows, rows * sizeof(RotRow));
    WQ_ALLOC(h, h->bud_row, n_in * 4);
    WQ_ALLOC(h, h->bud_words, (size_t)nG * 16);
    WQ_ALLOC(h, h->bud_cnt, (size_t)nG * 8);
    WQ_ALLOC(h, h->bud_base, (size_t)nG * 8);
    WQ_ALLOC(h, h->bud_ctrl, 64);
    if (d_msg_size) {
        WQ_ALLOC(h, h->byt_size, n_in * 4);
        WQ_ALLOC(h, h->byt_scan, (n_in + 1) * 8);
    }
    WQ_ALLOC(h, h->rot_part, kRotParts * sizeof(RotPart));
    WQ_HIP(h, hipMemsetAsync(h->bud_ctrl.p, 0, 64, s));
    WQ_HIP(h, hipMemsetAsync(h->rot_part.p, 0, kRotParts * sizeof(RotPart), s));

    const RotIn in{d_peer_offsets, d_msgs, d_kept_offsets, d_kept_msgs, d_msg_size, d_extra, d_extra_bytes, n_peers,
                   (uint32_t)n_in, (uint32_t)n_kept_in, (uint32_t)std::min<size_t>(n_msgs, 0xFFFFFFFFull), r, v};
    const RotWs ws{h->bud_len.as<uint32_t>(), h->bud_sum.as<uint32_t>(), h->bud_pre.as<uint32_t>(),
                   h->rot_len.as<uint32_t>(), h->rot_sum.as<uint32_t>(), h->rot_pre.as<uint32_t>(),
                   h->rot_rows.as<RotRow>(), h->bud_row.as<uint32_t>(), h->byt_size.as<uint32_t>(),
                   h->byt_scan.as<uint64_t>(), h->bud_words.as<uint64_t>(), h->bud_cnt.as<uint32_t>(),
                   h->bud_base.as<uint32_t>(), h->bud_ctrl.as<uint32_t>(), h->rot_part.as<RotPart>()};

    const dim3 blk(kBlock);
    const dim3 grid_r(grid_for(rows));
    const dim3 grid_g(grid_for((uint64_t)nG * 64));
    const uint32_t* d_T = ws.pre + n_peers;
    hipLaunchKernelGGL(k_rot_len, grid_r, blk, 0, s, in, ws);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_sat(h, ws.len, ws.sum, rows)) return rc;
    if (int rc = scan_sat(h, ws.klen, ws.ksum, rows)) return rc;
    hipLaunchKernelGGL(k_rot_pre, grid_r, blk, 0, s, in, ws, (const uint32_t*)d_cursor);
    WQ_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(k_rot_cut, grid_g, blk, 0, s, in, ws, nG);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_u32(h, ws.cnt, ws.base, nG, false)) return rc;
    if (d_msg_size)
        if (int rc = scan_terms(h, SizeTerm{ws.size, ws.words, d_T}, ws.scan, n_in + 1)) return rc;
    if (n_peers) {
        hipLaunchKernelGGL(k_rot_rowq, dim3(grid_for(n_peers)), blk, 0, s, in, ws);
        WQ_HIP(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_rot_keep, grid_g, blk, 0, s, in, ws, nG);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_u32(h, ws.cnt + nG, ws.base + nG, nG, false)) return rc;
    const uint64_t* kept_scan = nullptr;
    if (d_msg_size && (d_out_bytes || d_counters)) {
        if (int rc = scan_terms(h, SizeTerm{ws.size, ws.words + nG, d_T}, ws.scan, n_in + 1)) return rc;
        kept_scan = ws.scan;
    }
    hipLaunchKernelGGL(k_rot_offsets, grid_r, blk, 0, s, in, ws, nG, d_out_offsets, d_out_bytes);
    WQ_HIP(h, hipGetLastError());
    if (d_counters) {
        hipLaunchKernelGGL(k_rot_counters, dim3(1), dim3(64), 0, s, ws, n_peers, d_out_offsets, kept_scan, d_counters);
        WQ_HIP(h, hipGetLastError());
    }
    if (n_in) {
        hipLaunchKernelGGL(k_rot_emit, dim3(grid_for(n_in)), blk, 0, s, in, ws, nG, d_out_msgs, d_cursor);
        WQ_HIP(h, hipGetLastError());
    }
    return WQ_OK;
}

}  // namespace wq
