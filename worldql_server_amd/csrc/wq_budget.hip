// wq_budget.hip — per-observer send budgets: of every peer's send list the B nearest messages.
//
// wq_peer_major_device gives every peer the messages it could be sent; a connection has a budget.
// Here each row of that CSR keeps its min(B, len) elements nearest to the peer — the radius filter's
// f64 squared distance, ties by position in the row — in input order. An extension the reference
// does not have (it routes and forgets: local_message.rs:52-86, peer_map.rs:151-163).
//
//   rows    one lane per peer: the clamped length; a saturating scan gives the ordinal space
//           (send_rows.hpp); a second lane per peer: class, kept count, the select's slot of a long
//           cut row; the scan of the kept counts is the output's offsets
//   keys    one lane per ordinal: its row (a search over the prefix), its key (two position gathers),
//           its row's class
//   select  kBudPasses times: one lane per ordinal of a long cut row adds its digit into the row's
//           histogram (a block whose 256 ordinals lie in one row adds into LDS first and flushes the
//           bins it touched), then one block per slot picks the digit that holds the row's B-th key
//   ties    a wave per granule of 64 ordinals: the ballot of "key == the row's threshold key"; scan
//   keep    a wave per granule: the keep flags of every class — all, none, rank by counting in a short
//           row, below the threshold or one of its first ties in a long one; scan
//   emit    every kept ordinal stores its message at the granule's prefix plus the kept bits below it
//
// No lane, wave or block owns a row: a long row is spread over ceil(len / 256) blocks in every pass
// and its select step is one block of 256 lanes per pass; a short row costs each of its elements at
// most kBudShort key reads. Placement comes from counts and prefix sums alone; the atomics are
// integer adds into histograms and counters, so the output is the same bytes every time.
//
// The byte budgets (wq_peer_budget_bytes_device: the nearest messages that fit in W bytes) share the
// rows, keys, flag words and emit, and the select: its kernels are written once and take what a key
// weighs, and everything that follows from it, from a policy (SelCount, SelBytes).
#include "budget_ops.hpp"
#include "send_rows.hpp"

namespace wq {

namespace {

static_assert(kBudTile == kBlock && kBudBins == kBlock, "a histogram tile is one block of lanes, one lane per bin");

// What both budgets read and work on; CntIn / CntWs and BytIn / BytWs add each one's own.
struct BudIn {
    const uint32_t* off;
    const uint32_t* msgs;
    const double* mpos;
    const double* ppos;
    uint32_t n_peers, n_in, n_msgs, n_ppos;
};

struct BudWs {
    uint32_t* len;    // [n_peers + 1] clamped lengths, then the kept counts (bytes: the rows' classes)
    uint32_t* sum;    // [n_peers + 1] their saturating prefix
    uint32_t* pre;    // [n_peers + 1] the prefix clamped to n_in: the ordinal space
    uint64_t* key;    // [n_in]
    uint32_t* row;    // [n_in]
    uint8_t* cls;     // [n_in]
    uint64_t* words;  // [2 * nG] tie flags, keep flags
    uint32_t* cnt;    // [2 * nG]
    uint32_t* base;   // [2 * nG]
    uint32_t* ctrl;   // {rows_cut, error}; bytes: behind them, as a u64, bytes_in
};

struct CntIn : BudIn {
    const uint32_t* budget;
    uint32_t k;
};

struct CntWs : BudWs {
    BudSel* sel;     // [n_in / kBudShort + 1]
    uint32_t* hist;  // kBudBins per slot; all zero between calls
};

struct BytIn : BudIn {
    const uint32_t* msize;
    const uint64_t* wbudget;
    uint64_t w;
};

struct BytWs : BudWs {
    uint32_t* size;            // [n_in]
    uint64_t* scan;            // [n_in + 1]
    BudSelW* sel;              // [n_in / kBudShort + 1]
    unsigned long long* hist;  // kBudBins per slot; all zero between calls
};

__host__ __device__ __forceinline__ RowSpace bud_rows(const BudIn& in, const BudWs& ws) {
    return RowSpace{in.off, in.n_peers, in.n_in, ws.len, ws.sum, ws.pre};
}

// ---- the select's policies: what an element weighs, and what follows from it ----

// The count budget: every key weighs 1, a row keeps its `need` smallest.
struct SelCount {
    using In = CntIn;
    using Ws = CntWs;
    using Sel = BudSel;
    using Bin = uint32_t;
    static __device__ __forceinline__ Bin weight(const Ws&, uint64_t) { return 1u; }
    static __device__ __forceinline__ uint32_t& left(Sel& s) { return s.need; }
    static __device__ __forceinline__ bool picks(Bin below, Bin count, Bin need) {
        return bud_picks(below, count, need);
    }
    static __device__ __forceinline__ bool short_keeps(const In& in, const Ws& ws, uint32_t p, uint32_t q) {
        return bud_short_keeps(ws.key, ws.pre[p], ws.pre[p + 1] - ws.pre[p], q, bud_budget(in.budget, in.k, p));
    }
    // q0: the row's first ordinal; the tie flags and their prefix are in place
    static __device__ __forceinline__ bool long_keeps(const Ws& ws, const Sel& s, uint32_t q0, uint32_t q,
                                                      uint64_t key) {
        uint32_t tie_rank = 0;
        if (key == s.prefix) tie_rank = bud_before(ws.base, ws.words, q) - bud_before(ws.base, ws.words, q0);
        return bud_keeps(key, tie_rank, s.prefix, s.need);
    }
};

// The byte budgets: a key weighs its element's size (a zero weight adds nothing), a row keeps its
// smallest while they fit in `remaining` bytes.
struct SelBytes {
    using In = BytIn;
    using Ws = BytWs;
    using Sel = BudSelW;
    using Bin = unsigned long long;
    static __device__ __forceinline__ Bin weight(const Ws& ws, uint64_t q) { return ws.size[q]; }
    static __device__ __forceinline__ uint64_t& left(Sel& s) { return s.remaining; }
    static __device__ __forceinline__ bool picks(Bin below, Bin bytes, Bin remaining) {
        return bud_picks_bytes(below, bytes, remaining);
    }
    static __device__ __forceinline__ bool short_keeps(const In& in, const Ws& ws, uint32_t p, uint32_t q) {
        return bud_short_keeps_bytes(ws.key, ws.size, ws.pre[p], ws.pre[p + 1] - ws.pre[p], q,
                                     bud_wbudget(in.wbudget, in.w, p));
    }
    // q0: the row's first ordinal; ws.scan is the scan of the ties' sizes
    static __device__ __forceinline__ bool long_keeps(const Ws& ws, const Sel& s, uint32_t q0, uint32_t q,
                                                      uint64_t key) {
        uint64_t tie_bytes = 0;
        if (key == s.prefix) tie_bytes = ws.scan[q] - ws.scan[q0] + ws.size[q];
        return bud_keeps_bytes(key, tie_bytes, s.prefix, s.remaining);
    }
};

// ---- the kernels both budgets launch ----

// One pass of the select's histograms. A tile of kBudTile ordinals inside one long cut row sums its
// weights in LDS; the bins go to the row's histogram when the block moves to another row or ends.
// Tiles that hold a row boundary add to the rows' histograms directly, one global atomic per matching
// key: a row of a few hundred elements then sends that many atomics, and in the top passes, where a
// row's keys share their digit, to one address (rows of 257 to a few thousand elements mostly take
// this path; it is where the C3 shape's time goes).
template <class P>
__global__ __launch_bounds__(kBlock) void k_sel_hist(typename P::Ws ws, uint32_t n_peers, int shift) {
    using Bin = typename P::Bin;
    __shared__ Bin bins[kBudBins];
    const uint32_t T = ws.pre[n_peers];
    const uint32_t t = threadIdx.x;
    bins[t] = 0;
    __syncthreads();
    uint32_t cur_slot = 0xFFFFFFFFu;
    uint64_t cur_prefix = 0;
    for (uint32_t i = 0; i < kBudTiles; ++i) {
        const uint64_t q0 = ((uint64_t)blockIdx.x * kBudTiles + i) * kBudTile;
        if (q0 >= T) break;  // block-uniform
        const uint32_t last = T - q0 > kBudTile ? (uint32_t)q0 + kBudTile - 1 : T - 1;
        const uint32_t r0 = ws.row[q0], r1 = ws.row[last];
        const uint64_t q = q0 + t;
        if (r0 == r1) {  // block-uniform: one row, one class
            if (ws.cls[q0] != kBudLongCut) continue;
            const uint32_t slot = ws.pre[r0] >> kBudShortLog2;
            if (slot != cur_slot) {
                if (cur_slot != 0xFFFFFFFFu) {
                    __syncthreads();
                    if (bins[t]) atomicAdd(&ws.hist[(uint64_t)cur_slot * kBudBins + t], bins[t]);
                    bins[t] = 0;
                    __syncthreads();
                }
                cur_slot = slot;
                cur_prefix = ws.sel[slot].prefix;
            }
            if (q < T) {
                const uint64_t key = ws.key[q];
                const Bin w = P::weight(ws, q);
                if (w && bud_matches(key, cur_prefix, shift)) atomicAdd(&bins[bud_digit(key, shift)], w);
            }
        } else if (q < T && ws.cls[q] == kBudLongCut) {
            const uint32_t slot = ws.pre[ws.row[q]] >> kBudShortLog2;
            const uint64_t key = ws.key[q];
            const Bin w = P::weight(ws, q);
            if (w && bud_matches(key, ws.sel[slot].prefix, shift))
                atomicAdd(&ws.hist[(uint64_t)slot * kBudBins + bud_digit(key, shift)], w);
        }
    }
    if (cur_slot != 0xFFFFFFFFu) {
        __syncthreads();
        if (bins[t]) atomicAdd(&ws.hist[(uint64_t)cur_slot * kBudBins + t], bins[t]);
    }
}

// One block per slot: lane t owns bin t; the block's prefix sum finds the bin the policy picks: the
// one that holds the need-th smallest matching key, or in which the running byte total first exceeds
// what is left. The bins are read and zeroed, so the histograms are zero after every pass.
template <class P>
__global__ __launch_bounds__(kBudBins) void k_sel_pick(typename P::Ws ws, int shift) {
    using Bin = typename P::Bin;
    __shared__ Bin wave_tot[kBudBins / 64];
    typename P::Sel* s = ws.sel + blockIdx.x;
    if (!s->active) return;  // block-uniform
    const Bin left = P::left(*s);
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    Bin* bin = ws.hist + (uint64_t)blockIdx.x * kBudBins + t;
    const Bin c = *bin;
    *bin = 0;
    Bin incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const Bin o = __shfl_up(incl, d);
        if (lane >= (uint32_t)d) incl += o;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();  // also: every lane has read what is left
    Bin below = incl - c;
    for (uint32_t w = 0; w < wave; ++w) below += wave_tot[w];
    if (P::picks(below, c, left)) {
        s->prefix |= (uint64_t)t << shift;
        P::left(*s) = left - below;
    }
}

// flags 0: ties (long cut rows, key == the row's threshold key); flags 1: keep.
template <class P, int kKeep>
__global__ __launch_bounds__(kBlock) void k_sel_flag(typename P::In in, typename P::Ws ws, uint32_t nG) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t g = (uint32_t)(q >> 6);
    if (g >= nG) return;  // wave-uniform
    const uint32_t T = ws.pre[in.n_peers];
    bool f = false;
    if (q < T) {
        const uint8_t c = ws.cls[q];
        if (!kKeep) {
            if (c == kBudLongCut) f = ws.key[q] == ws.sel[ws.pre[ws.row[q]] >> kBudShortLog2].prefix;
        } else if (c == kBudAll) {
            f = true;
        } else if (c == kBudShortCut) {
            f = P::short_keeps(in, ws, ws.row[q], (uint32_t)q);
        } else if (c == kBudLongCut) {
            const uint32_t q0 = ws.pre[ws.row[q]];
            const typename P::Sel s = ws.sel[q0 >> kBudShortLog2];
            f = P::long_keeps(ws, s, q0, (uint32_t)q, ws.key[q]);
        }
    }
    store_flags(ws.words, ws.cnt, (uint64_t)kKeep * nG + g, f);
}

__global__ __launch_bounds__(kBlock) void k_bud_emit(BudIn in, BudWs ws, uint32_t nG, uint32_t* __restrict__ out) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= ws.pre[in.n_peers]) return;
    const uint64_t* words = ws.words + nG;
    if (!flag_at(words, q)) return;
    const uint32_t j = rows_elem(in.off, ws.pre, in.n_in, ws.row[q], (uint32_t)q);
    const uint32_t pos = bud_before(ws.base + nG, words, (uint32_t)q);
    if (pos < in.n_in) out[pos] = in.msgs[j];
}

// ---- the count budget's own ----

__global__ __launch_bounds__(kBlock) void k_bud_rows(CntIn in, CntWs ws) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > in.n_peers) return;
    uint32_t len;
    const uint32_t a = rows_pre_step(bud_rows(in, ws), p, &ws.ctrl[1], kBudErrRows, &len);
    if (p == in.n_peers) {
        ws.len[p] = 0;
        return;
    }
    const uint32_t B = bud_budget(in.budget, in.k, (uint32_t)p);
    const uint8_t c = bud_class(len, B);
    if (c != kBudAll) atomicAdd(&ws.ctrl[0], 1u);
    if (c == kBudLongCut) ws.sel[a >> kBudShortLog2] = BudSel{0ull, B, 1u};
    ws.len[p] = len < B ? len : B;
}

__global__ __launch_bounds__(kBlock) void k_bud_keys(CntIn in, CntWs ws) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= ws.pre[in.n_peers]) return;
    const uint32_t p = bud_row_of(ws.pre, in.n_peers, (uint32_t)q);
    const uint32_t j = rows_elem(in.off, ws.pre, in.n_in, p, (uint32_t)q);
    bool bad;
    ws.key[q] = bud_key(in.mpos, in.n_msgs, in.ppos, in.n_ppos, p, in.msgs[j], &bad);
    ws.row[q] = p;
    ws.cls[q] = bud_class(ws.pre[p + 1] - ws.pre[p], bud_budget(in.budget, in.k, p));
    if (bad) atomicOr(&ws.ctrl[1], kBudErrMsg);
}

__global__ void k_bud_counters(BudWs ws, uint32_t n_peers, const uint32_t* __restrict__ out_off,
                               wq_budget_counters* counters) {
    wq_budget_counters c;
    c.n_in = ws.pre[n_peers];
    c.n_kept = out_off[n_peers];
    c.rows_cut = ws.ctrl[0];
    c.error = ws.ctrl[1];
    *counters = c;
}

// ---- the byte budgets' own: of every peer's send list the nearest messages that fit in W bytes ----
//
// The select is weighted: its histograms sum the sizes of the matching keys (u64 bins) and a pick
// takes the bin in which the running byte total first exceeds what is left of W. The output's offsets
// are not known before the elements are, so they come from the keep words.
//
//   rows    k_rows_len, the saturating scan and k_rows_pre: the ordinal space
//   keys    one lane per ordinal: its row, key and size; a u64 scan of the sizes (S)
//   class   one lane per peer: the row's total S[pre[p + 1]] - S[pre[p]] against W_p gives its class
//           and seeds a long cut row's slot; one lane per ordinal copies its row's class
//   select  as above with sizes, kBudPasses times
//   ties    the ballot of "key == the row's threshold key"; a u64 scan of the ties' sizes
//   keep    the keep flags of every class; scan of the granules' counts
//   offsets one lane per peer: the kept bits before pre[p]
//   emit    k_bud_emit; a u64 scan of the kept sizes gives d_out_bytes and bytes_kept
//
// The three u64 scans share one buffer: S is dead once the classes are known, the ties' scan once
// the keep words are.

// ctrl: {rows_cut, error} and, as a u64 behind them, bytes_in.
__device__ __forceinline__ uint64_t* byt_bytes_in(uint32_t* ctrl) { return reinterpret_cast<uint64_t*>(ctrl + 2); }

__global__ __launch_bounds__(kBlock) void k_byt_keys(BytIn in, BytWs ws) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= ws.pre[in.n_peers]) return;
    const uint32_t p = bud_row_of(ws.pre, in.n_peers, (uint32_t)q);
    const uint32_t m = in.msgs[rows_elem(in.off, ws.pre, in.n_in, p, (uint32_t)q)];
    bool bad;
    ws.key[q] = bud_key(in.mpos, in.n_msgs, in.ppos, in.n_ppos, p, m, &bad);
    ws.row[q] = p;
    ws.size[q] = bud_size(in.msize, in.n_msgs, m);
    if (bad) atomicOr(&ws.ctrl[1], kBudErrMsg);
}

__global__ __launch_bounds__(kBlock) void k_byt_class(BytIn in, BytWs ws) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > in.n_peers) return;
    const uint32_t a = ws.pre[p];
    if (p == in.n_peers) {
        *byt_bytes_in(ws.ctrl) = ws.scan[a];
        return;
    }
    const uint32_t b = ws.pre[p + 1];
    const uint64_t W = bud_wbudget(in.wbudget, in.w, (uint32_t)p);
    const uint8_t c = bud_class_bytes(b - a, ws.scan[b] - ws.scan[a], W);
    if (c != kBudAll) atomicAdd(&ws.ctrl[0], 1u);
    if (c == kBudLongCut) ws.sel[a >> kBudShortLog2] = BudSelW{0ull, W, 1u, 0u};
    ws.len[p] = c;
}

__global__ __launch_bounds__(kBlock) void k_byt_cls(BudWs ws, uint32_t n_peers) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= ws.pre[n_peers]) return;
    ws.cls[q] = (uint8_t)ws.len[ws.row[q]];
}

__global__ __launch_bounds__(kBlock) void k_byt_offsets(BudWs ws, uint32_t n_peers, uint32_t nG,
                                                         uint32_t* __restrict__ out_off) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > n_peers) return;
    out_off[p] = bud_before(ws.base + nG, ws.words + nG, ws.pre[p]);
}

// ws.scan: the scan of the kept sizes.
__global__ __launch_bounds__(kBlock) void k_byt_out_bytes(BytWs ws, uint32_t n_peers, uint64_t* __restrict__ out_bytes) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_peers) return;
    out_bytes[p] = ws.scan[ws.pre[p + 1]] - ws.scan[ws.pre[p]];
}

// kept_scan: the scan of the kept sizes, NULL when the call has no element.
__global__ void k_byt_counters(BudWs ws, uint32_t n_peers, const uint32_t* __restrict__ out_off,
                               const uint64_t* __restrict__ kept_scan, wq_budget_bytes_counters* counters) {
    wq_budget_bytes_counters c;
    c.n_in = ws.pre[n_peers];
    c.n_kept = out_off[n_peers];
    c.bytes_in = *byt_bytes_in(ws.ctrl);
    c.bytes_kept = kept_scan ? kept_scan[ws.pre[n_peers]] : 0ull;
    c.rows_cut = ws.ctrl[0];
    c.error = ws.ctrl[1];
    *counters = c;
}

// ---- host side ----

// The buffers both budgets run on, and the two views of them. The per-peer and per-ordinal arrays,
// the flag words and ctrl are one set: the calls are ordered on the handle's stream and nothing in
// them outlives a call. Each budget's select state and histograms, which must be zero between
// calls, are its own.
int bud_setup(wq_router* h, const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers, size_t n_in,
              const double* d_msg_pos, size_t n_msgs, const double* d_peer_pos, size_t n_peer_pos, BudIn* in,
              BudWs* ws) {
    const size_t nG = n_in / 64 + 1;
    if (int rc = rows_alloc(h, (size_t)n_peers + 1)) return rc;
    WQ_ALLOC(h, h->bud_key, n_in * 8);
    WQ_ALLOC(h, h->bud_row, n_in * 4);
    WQ_ALLOC(h, h->bud_cls, n_in);
    WQ_ALLOC(h, h->bud_words, nG * 16);
    WQ_ALLOC(h, h->bud_cnt, nG * 8);
    WQ_ALLOC(h, h->bud_base, nG * 8);
    WQ_ALLOC(h, h->bud_ctrl, 64);
    const RowSpace r = rows_view(h, d_peer_offsets, n_peers, n_in);
    *in = BudIn{d_peer_offsets, d_msgs, d_msg_pos, d_peer_pos, n_peers, r.n_in,
                (uint32_t)std::min<size_t>(n_msgs, 0xFFFFFFFFull),
                (uint32_t)std::min<size_t>(n_peer_pos, 0xFFFFFFFFull)};
    *ws = BudWs{r.len, r.sum, r.pre, h->bud_key.as<uint64_t>(), h->bud_row.as<uint32_t>(), h->bud_cls.as<uint8_t>(),
                h->bud_words.as<uint64_t>(), h->bud_cnt.as<uint32_t>(), h->bud_base.as<uint32_t>(),
                h->bud_ctrl.as<uint32_t>()};
    return WQ_OK;
}

// The select's kBudPasses pairs of a histogram pass and its pick, the top digit first.
template <class P>
int launch_select(wq_router* h, ZeroedBuf& hist, const typename P::Ws& ws, uint32_t n_peers, size_t n_in,
                  size_t n_slots) {
    hipStream_t s = h->stream;
    const dim3 grid_h(grid_for((n_in + kBudTiles - 1) / kBudTiles));
    const dim3 grid_p((unsigned)n_slots);
    hist.begin();  // until every pass has its pick
    for (int pass = 0; pass < kBudPasses; ++pass) {
        hipLaunchKernelGGL(k_sel_hist<P>, grid_h, dim3(kBlock), 0, s, ws, n_peers, bud_shift(pass));
        WQ_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_sel_pick<P>, grid_p, dim3(kBudBins), 0, s, ws, bud_shift(pass));
        WQ_HIP(h, hipGetLastError());
    }
    hist.end();
    return WQ_OK;
}

}  // namespace

void budget_release(wq_router* h) {
    for (DevBuf* b : {&h->bud_len, &h->bud_sum, &h->bud_pre, &h->bud_key, &h->bud_row, &h->bud_cls, &h->bud_sel,
                      &h->bud_words, &h->bud_cnt, &h->bud_base, &h->bud_ctrl, &h->byt_size, &h->byt_scan, &h->byt_sel})
        b->release();
    h->bud_hist.release();
    h->byt_hist.release();
}

// The call on device arrays (the handle's device is current; arguments validated, n_in <= 2^32 - 1,
// d_peer_pos / n_peer_pos already resolved to the handle's positions when the caller gave none).
int launch_peer_budget(wq_router* h, const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers,
                       size_t n_in, const double* d_msg_pos, size_t n_msgs, const double* d_peer_pos,
                       size_t n_peer_pos, uint32_t k, const uint32_t* d_budget, uint32_t* d_out_offsets,
                       uint32_t* d_out_msgs, wq_budget_counters* d_counters) {
    hipStream_t s = h->stream;
    const size_t rows = (size_t)n_peers + 1;
    const size_t n_slots = n_in / kBudShort + 1;
    const uint32_t nG = (uint32_t)(n_in / 64 + 1);
    CntIn in;
    CntWs ws;
    if (int rc = bud_setup(h, d_peer_offsets, d_msgs, n_peers, n_in, d_msg_pos, n_msgs, d_peer_pos, n_peer_pos, &in,
                           &ws))
        return rc;
    WQ_ALLOC(h, h->bud_sel, n_slots * sizeof(BudSel));
    if (int rc = h->bud_hist.prepare(h, n_slots * kBudBins * 4, s)) return rc;
    WQ_HIP(h, hipMemsetAsync(h->bud_ctrl.p, 0, 64, s));
    WQ_HIP(h, hipMemsetAsync(h->bud_sel.p, 0, n_slots * sizeof(BudSel), s));
    in.budget = d_budget;
    in.k = k;
    ws.sel = h->bud_sel.as<BudSel>();
    ws.hist = h->bud_hist.b.as<uint32_t>();

    const dim3 blk(kBlock);
    const dim3 grid_r(grid_for(rows));
    hipLaunchKernelGGL(k_rows_len, grid_r, blk, 0, s, bud_rows(in, ws), ws.ctrl + 1, kBudErrRows);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_sat(h, ws.len, ws.sum, rows)) return rc;
    hipLaunchKernelGGL(k_bud_rows, grid_r, blk, 0, s, in, ws);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_u32(h, ws.len, d_out_offsets, rows, false)) return rc;
    if (n_in) {
        const dim3 grid_e(grid_for(n_in));
        const dim3 grid_g(grid_for((uint64_t)nG * 64));
        hipLaunchKernelGGL(k_bud_keys, grid_e, blk, 0, s, in, ws);
        WQ_HIP(h, hipGetLastError());
        if (int rc = launch_select<SelCount>(h, h->bud_hist, ws, n_peers, n_in, n_slots)) return rc;
        hipLaunchKernelGGL((k_sel_flag<SelCount, 0>), grid_g, blk, 0, s, in, ws, nG);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_u32(h, ws.cnt, ws.base, nG, false)) return rc;
        hipLaunchKernelGGL((k_sel_flag<SelCount, 1>), grid_g, blk, 0, s, in, ws, nG);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_u32(h, ws.cnt + nG, ws.base + nG, nG, false)) return rc;
        hipLaunchKernelGGL(k_bud_emit, grid_e, blk, 0, s, in, ws, nG, d_out_msgs);
        WQ_HIP(h, hipGetLastError());
    }
    if (d_counters) {
        hipLaunchKernelGGL(k_bud_counters, dim3(1), dim3(1), 0, s, ws, n_peers, d_out_offsets, d_counters);
        WQ_HIP(h, hipGetLastError());
    }
    return WQ_OK;
}

// The byte budgets on device arrays (as launch_peer_budget: arguments validated, positions resolved).
int launch_peer_budget_bytes(wq_router* h, const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers,
                             size_t n_in, const double* d_msg_pos, const uint32_t* d_msg_size, size_t n_msgs,
                             const double* d_peer_pos, size_t n_peer_pos, uint64_t w, const uint64_t* d_budget_bytes,
                             uint32_t* d_out_offsets, uint32_t* d_out_msgs, uint64_t* d_out_bytes,
                             wq_budget_bytes_counters* d_counters) {
    hipStream_t s = h->stream;
    const size_t rows = (size_t)n_peers + 1;
    const size_t n_slots = n_in / kBudShort + 1;
    const uint32_t nG = (uint32_t)(n_in / 64 + 1);
    BytIn in;
    BytWs ws;
    if (int rc = bud_setup(h, d_peer_offsets, d_msgs, n_peers, n_in, d_msg_pos, n_msgs, d_peer_pos, n_peer_pos, &in,
                           &ws))
        return rc;
    WQ_ALLOC(h, h->byt_size, n_in * 4);
    WQ_ALLOC(h, h->byt_scan, (n_in + 1) * 8);
    WQ_ALLOC(h, h->byt_sel, n_slots * sizeof(BudSelW));
    if (int rc = h->byt_hist.prepare(h, n_slots * kBudBins * 8, s)) return rc;
    WQ_HIP(h, hipMemsetAsync(h->bud_ctrl.p, 0, 64, s));
    WQ_HIP(h, hipMemsetAsync(h->byt_sel.p, 0, n_slots * sizeof(BudSelW), s));
    in.msize = d_msg_size;
    in.wbudget = d_budget_bytes;
    in.w = w;
    ws.size = h->byt_size.as<uint32_t>();
    ws.scan = h->byt_scan.as<uint64_t>();
    ws.sel = h->byt_sel.as<BudSelW>();
    ws.hist = h->byt_hist.b.as<unsigned long long>();

    const dim3 blk(kBlock);
    const dim3 grid_r(grid_for(rows));
    hipLaunchKernelGGL(k_rows_len, grid_r, blk, 0, s, bud_rows(in, ws), ws.ctrl + 1, kBudErrRows);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_sat(h, ws.len, ws.sum, rows)) return rc;
    hipLaunchKernelGGL(k_rows_pre, grid_r, blk, 0, s, bud_rows(in, ws), ws.ctrl + 1, kBudErrRows);
    WQ_HIP(h, hipGetLastError());
    const uint32_t* d_T = ws.pre + n_peers;
    const uint64_t* kept_scan = nullptr;
    if (n_in) {
        const dim3 grid_e(grid_for(n_in));
        const dim3 grid_g(grid_for((uint64_t)nG * 64));
        hipLaunchKernelGGL(k_byt_keys, grid_e, blk, 0, s, in, ws);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_terms(h, SizeTerm{ws.size, nullptr, d_T}, ws.scan, n_in + 1)) return rc;
        hipLaunchKernelGGL(k_byt_class, grid_r, blk, 0, s, in, ws);
        WQ_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_byt_cls, grid_e, blk, 0, s, ws, n_peers);
        WQ_HIP(h, hipGetLastError());
        if (int rc = launch_select<SelBytes>(h, h->byt_hist, ws, n_peers, n_in, n_slots)) return rc;
        hipLaunchKernelGGL((k_sel_flag<SelBytes, 0>), grid_g, blk, 0, s, in, ws, nG);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_terms(h, SizeTerm{ws.size, ws.words, d_T}, ws.scan, n_in + 1)) return rc;
        hipLaunchKernelGGL((k_sel_flag<SelBytes, 1>), grid_g, blk, 0, s, in, ws, nG);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_u32(h, ws.cnt + nG, ws.base + nG, nG, false)) return rc;
        hipLaunchKernelGGL(k_byt_offsets, grid_r, blk, 0, s, ws, n_peers, nG, d_out_offsets);
        WQ_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_bud_emit, grid_e, blk, 0, s, in, ws, nG, d_out_msgs);
        WQ_HIP(h, hipGetLastError());
        if (d_out_bytes || d_counters) {
            if (int rc = scan_terms(h, SizeTerm{ws.size, ws.words + nG, d_T}, ws.scan, n_in + 1)) return rc;
            kept_scan = ws.scan;
        }
        if (d_out_bytes && n_peers) {
            hipLaunchKernelGGL(k_byt_out_bytes, dim3(grid_for(n_peers)), blk, 0, s, ws, n_peers, d_out_bytes);
            WQ_HIP(h, hipGetLastError());
        }
    } else {
        WQ_HIP(h, hipMemsetAsync(d_out_offsets, 0, rows * 4, s));
        if (d_out_bytes && n_peers) WQ_HIP(h, hipMemsetAsync(d_out_bytes, 0, (size_t)n_peers * 8, s));
    }
    if (d_counters) {
        hipLaunchKernelGGL(k_byt_counters, dim3(1), dim3(1), 0, s, ws, n_peers, d_out_offsets, kept_scan,
                           d_counters);
        WQ_HIP(h, hipGetLastError());
    }
    return WQ_OK;
}

}  // namespace wq
