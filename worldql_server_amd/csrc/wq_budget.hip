// wq_budget.hip — per-observer send budgets: of every peer's send list the B nearest messages.
//
// wq_peer_major_device gives every peer the messages it could be sent; a connection has a budget.
// Here each row of that CSR keeps its min(B, len) elements nearest to the peer — the radius filter's
// f64 squared distance, ties by position in the row — in input order. An extension the reference
// does not have (it routes and forgets: local_message.rs:52-86, peer_map.rs:151-163).
//
//   rows    one lane per peer: the clamped length; a saturating scan gives the ordinal space
//           (budget_ops.hpp); a second lane per peer: class, kept count, the select's slot of a long
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
// The byte budgets (wq_peer_budget_bytes_device: the nearest messages that fit in W bytes) follow the
// count budget below and share its rows, keys, flag words and emit.
#include "budget_ops.hpp"
#include "table_prims.hpp"

namespace wq {

namespace {

static_assert(kBudTile == kBlock && kBudBins == kBlock, "a histogram tile is one block of lanes, one lane per bin");

struct BudIn {
    const uint32_t* off;
    const uint32_t* msgs;
    const double* mpos;
    const double* ppos;
    const uint32_t* budget;
    uint32_t n_peers, n_in, n_msgs, n_ppos, k;
};

struct BudWs {
    uint32_t* len;    // [n_peers + 1] clamped lengths, then the kept counts
    uint32_t* sum;    // [n_peers + 1] their saturating prefix
    uint32_t* pre;    // [n_peers + 1] the prefix clamped to n_in: the ordinal space
    uint64_t* key;    // [n_in]
    uint32_t* row;    // [n_in]
    uint8_t* cls;     // [n_in]
    BudSel* sel;      // [n_in / kBudShort + 1]
    uint32_t* hist;   // kBudBins per slot; all zero between calls
    uint64_t* words;  // [2 * nG] tie flags, keep flags
    uint32_t* cnt;    // [2 * nG]
    uint32_t* base;   // [2 * nG]
    uint32_t* ctrl;   // {rows_cut, error}
};

__global__ __launch_bounds__(kBlock) void k_bud_len(BudIn in, BudWs ws) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > in.n_peers) return;
    bool ok = true;
    ws.len[p] = p < in.n_peers ? bud_len(in.off, (uint32_t)p, in.n_in, &ok) : 0u;
    if (!ok) atomicOr(&ws.ctrl[1], kBudErrRows);
}

__global__ __launch_bounds__(kBlock) void k_bud_rows(BudIn in, BudWs ws) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > in.n_peers) return;
    const uint32_t a = ws.sum[p] < in.n_in ? ws.sum[p] : in.n_in;
    ws.pre[p] = a;
    if (p == in.n_peers) {
        ws.len[p] = 0;
        return;
    }
    const uint32_t b = ws.sum[p + 1] < in.n_in ? ws.sum[p + 1] : in.n_in;
    const uint32_t len = b - a;
    if (len != ws.len[p]) atomicOr(&ws.ctrl[1], kBudErrRows);  // overlapping rows: cut at n_in ordinals
    const uint32_t B = bud_budget(in.budget, in.k, (uint32_t)p);
    const uint8_t c = bud_class(len, B);
    if (c != kBudAll) atomicAdd(&ws.ctrl[0], 1u);
    if (c == kBudLongCut) ws.sel[a >> kBudShortLog2] = BudSel{0ull, B, 1u};
    ws.len[p] = len < B ? len : B;
}

__global__ __launch_bounds__(kBlock) void k_bud_keys(BudIn in, BudWs ws) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= ws.pre[in.n_peers]) return;
    const uint32_t p = bud_row_of(ws.pre, in.n_peers, (uint32_t)q);
    const uint32_t j = bud_row_start(in.off, p, in.n_in) + ((uint32_t)q - ws.pre[p]);
    bool bad;
    ws.key[q] = bud_key(in.mpos, in.n_msgs, in.ppos, in.n_ppos, p, in.msgs[j], &bad);
    ws.row[q] = p;
    ws.cls[q] = bud_class(ws.pre[p + 1] - ws.pre[p], bud_budget(in.budget, in.k, p));
    if (bad) atomicOr(&ws.ctrl[1], kBudErrMsg);
}

// One pass of the select's histograms. A tile of kBudTile ordinals inside one long cut row counts in
// LDS; the bins go to the row's histogram when the block moves to another row or ends. Tiles that
// hold a row boundary add to the rows' histograms directly, one global atomic per matching key: a
// row of a few hundred elements then sends that many atomics, and in the top passes, where a row's
// keys share their digit, to one address (rows of 257 to a few thousand elements mostly take this
// path; it is where the C3 shape's time goes).
__global__ __launch_bounds__(kBlock) void k_bud_hist(BudWs ws, uint32_t n_peers, int shift) {
    __shared__ uint32_t bins[kBudBins];
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
                if (bud_matches(key, cur_prefix, shift)) atomicAdd(&bins[bud_digit(key, shift)], 1u);
            }
        } else if (q < T && ws.cls[q] == kBudLongCut) {
            const uint32_t slot = ws.pre[ws.row[q]] >> kBudShortLog2;
            const uint64_t key = ws.key[q];
            if (bud_matches(key, ws.sel[slot].prefix, shift))
                atomicAdd(&ws.hist[(uint64_t)slot * kBudBins + bud_digit(key, shift)], 1u);
        }
    }
    if (cur_slot != 0xFFFFFFFFu) {
        __syncthreads();
        if (bins[t]) atomicAdd(&ws.hist[(uint64_t)cur_slot * kBudBins + t], bins[t]);
    }
}

// One block per slot: lane t owns bin t; the block's prefix sum finds the bin that holds the need-th
// smallest matching key. The bins are read and zeroed, so the histograms are zero after every pass.
__global__ __launch_bounds__(kBudBins) void k_bud_pick(BudWs ws, int shift) {
    __shared__ uint32_t wave_tot[kBudBins / 64];
    BudSel* s = ws.sel + blockIdx.x;
    if (!s->active) return;  // block-uniform
    const uint32_t need = s->need;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t* bin = ws.hist + (uint64_t)blockIdx.x * kBudBins + t;
    const uint32_t c = *bin;
    *bin = 0;
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= (uint32_t)d) incl += o;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();  // also: every lane has read s->need
    uint32_t below = incl - c;
    for (uint32_t w = 0; w < wave; ++w) below += wave_tot[w];
    if (bud_picks(below, c, need)) {
        s->prefix |= (uint64_t)t << shift;
        s->need = need - below;
    }
}

// flags 0: ties (long cut rows, key == the row's threshold key); flags 1: keep.
template <int kKeep>
__global__ __launch_bounds__(kBlock) void k_bud_flag(BudIn in, BudWs ws, uint32_t nG) {
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
            const uint32_t p = ws.row[q];
            f = bud_short_keeps(ws.key, ws.pre[p], ws.pre[p + 1] - ws.pre[p], (uint32_t)q,
                                bud_budget(in.budget, in.k, p));
        } else if (c == kBudLongCut) {
            const uint32_t q0 = ws.pre[ws.row[q]];
            const BudSel s = ws.sel[q0 >> kBudShortLog2];
            const uint64_t key = ws.key[q];
            uint32_t tie_rank = 0;
            if (key == s.prefix) tie_rank = bud_before(ws.base, ws.words, (uint32_t)q) - bud_before(ws.base, ws.words, q0);
            f = bud_keeps(key, tie_rank, s.prefix, s.need);
        }
    }
    const uint64_t word = __ballot(f);
    if ((threadIdx.x & 63u) == 0) {
        ws.words[(uint64_t)kKeep * nG + g] = word;
        ws.cnt[(uint64_t)kKeep * nG + g] = (uint32_t)__popcll(word);
    }
}

__global__ __launch_bounds__(kBlock) void k_bud_emit(BudIn in, BudWs ws, uint32_t nG, uint32_t* __restrict__ out) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= ws.pre[in.n_peers]) return;
    const uint64_t* words = ws.words + nG;
    if (!((words[q >> 6] >> (q & 63u)) & 1ull)) return;
    const uint32_t p = ws.row[q];
    const uint32_t j = bud_row_start(in.off, p, in.n_in) + ((uint32_t)q - ws.pre[p]);
    const uint32_t pos = bud_before(ws.base + nG, words, (uint32_t)q);
    if (pos < in.n_in) out[pos] = in.msgs[j];
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

int scan_sat(wq_router* h, const uint32_t* in, uint32_t* out, size_t n) {
    size_t bytes = 0;
    WQ_HIP(h, rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, n, BudSatAdd(), h->stream));
    WQ_ALLOC(h, h->sort_tmp, bytes);
    WQ_HIP(h, rocprim::exclusive_scan(h->sort_tmp.p, bytes, in, out, 0u, n, BudSatAdd(), h->stream));
    return WQ_OK;
}

// ---- byte budgets: of every peer's send list the nearest messages that fit in W bytes ----
//
// The same ordinal space, keys, flag words and emit; the select is weighted: its histograms sum the
// sizes of the matching keys (u64 bins) and a pick takes the bin in which the running byte total
// first exceeds what is left of W. The output's offsets are not known before the elements are, so
// they come from the keep words.
//
//   rows    k_bud_len and the saturating scan as above; k_byt_pre: the ordinal space
//   keys    one lane per ordinal: its row, key and size; a u64 scan of the sizes (S)
//   class   one lane per peer: the row's total S[pre[p + 1]] - S[pre[p]] against W_p gives its class
//           and seeds a long cut row's slot; one lane per ordinal copies its row's class
//   select  as above with sizes: k_byt_hist / k_byt_pick, kBudPasses times
//   ties    the ballot of "key == the row's threshold key"; a u64 scan of the ties' sizes
//   keep    the keep flags of every class; scan of the granules' counts
//   offsets one lane per peer: the kept bits before pre[p]
//   emit    k_bud_emit; a u64 scan of the kept sizes gives d_out_bytes and bytes_kept
//
// The three u64 scans share one buffer: S is dead once the classes are known, the ties' scan once
// the keep words are.

struct BytIn {
    BudIn b;  // budget and k unused
    const uint32_t* msize;
    const uint64_t* wbudget;
    uint64_t w;
};

struct BytWs {
    BudWs b;         // len: the rows' classes after k_byt_class; sel and hist unused
    uint32_t* size;  // [n_in]
    uint64_t* scan;  // [n_in + 1]
    BudSelW* sel;    // [n_in / kBudShort + 1]
    uint64_t* hist;  // kBudBins per slot; all zero between calls
};

// ctrl: {rows_cut, error} and, as a u64 behind them, bytes_in.
__device__ __forceinline__ uint64_t* byt_bytes_in(uint32_t* ctrl) { return reinterpret_cast<uint64_t*>(ctrl + 2); }

struct BytTerm {
    const uint32_t* size;
    const uint64_t* words;  // nullable
    const uint32_t* T;
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t q) const {
        return bud_byte_term(size, words, *T, q);
    }
};

__global__ __launch_bounds__(kBlock) void k_byt_pre(BudIn in, BudWs ws) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > in.n_peers) return;
    const uint32_t a = ws.sum[p] < in.n_in ? ws.sum[p] : in.n_in;
    ws.pre[p] = a;
    if (p == in.n_peers) return;
    const uint32_t b = ws.sum[p + 1] < in.n_in ? ws.sum[p + 1] : in.n_in;
    if (b - a != ws.len[p]) atomicOr(&ws.ctrl[1], kBudErrRows);  // overlapping rows: cut at n_in ordinals
}

__global__ __launch_bounds__(kBlock) void k_byt_keys(BytIn in, BytWs ws) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= ws.b.pre[in.b.n_peers]) return;
    const uint32_t p = bud_row_of(ws.b.pre, in.b.n_peers, (uint32_t)q);
    const uint32_t j = bud_row_start(in.b.off, p, in.b.n_in) + ((uint32_t)q - ws.b.pre[p]);
    const uint32_t m = in.b.msgs[j];
    bool bad;
    ws.b.key[q] = bud_key(in.b.mpos, in.b.n_msgs, in.b.ppos, in.b.n_ppos, p, m, &bad);
    ws.b.row[q] = p;
    ws.size[q] = bud_size(in.msize, in.b.n_msgs, m);
    if (bad) atomicOr(&ws.b.ctrl[1], kBudErrMsg);
}

__global__ __launch_bounds__(kBlock) void k_byt_class(BytIn in, BytWs ws) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > in.b.n_peers) return;
    const uint32_t a = ws.b.pre[p];
    if (p == in.b.n_peers) {
        *byt_bytes_in(ws.b.ctrl) = ws.scan[a];
        return;
    }
    const uint32_t b = ws.b.pre[p + 1];
    const uint64_t W = bud_wbudget(in.wbudget, in.w, (uint32_t)p);
    const uint8_t c = bud_class_bytes(b - a, ws.scan[b] - ws.scan[a], W);
    if (c != kBudAll) atomicAdd(&ws.b.ctrl[0], 1u);
    if (c == kBudLongCut) ws.sel[a >> kBudShortLog2] = BudSelW{0ull, W, 1u, 0u};
    ws.b.len[p] = c;
}

__global__ __launch_bounds__(kBlock) void k_byt_cls(BytWs ws, uint32_t n_peers) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= ws.b.pre[n_peers]) return;
    ws.b.cls[q] = (uint8_t)ws.b.len[ws.b.row[q]];
}

// k_bud_hist with sizes: a tile inside one long cut row sums in LDS and flushes the bins it touched,
// a tile with a row boundary adds to the rows' histograms directly. Zero-size elements add nothing.
__global__ __launch_bounds__(kBlock) void k_byt_hist(BytWs ws, uint32_t n_peers, int shift) {
    __shared__ unsigned long long bins[kBudBins];
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(ws.hist);
    const uint32_t T = ws.b.pre[n_peers];
    const uint32_t t = threadIdx.x;
    bins[t] = 0;
    __syncthreads();
    uint32_t cur_slot = 0xFFFFFFFFu;
    uint64_t cur_prefix = 0;
    for (uint32_t i = 0; i < kBudTiles; ++i) {
        const uint64_t q0 = ((uint64_t)blockIdx.x * kBudTiles + i) * kBudTile;
        if (q0 >= T) break;  // block-uniform
        const uint32_t last = T - q0 > kBudTile ? (uint32_t)q0 + kBudTile - 1 : T - 1;
        const uint32_t r0 = ws.b.row[q0], r1 = ws.b.row[last];
        const uint64_t q = q0 + t;
        if (r0 == r1) {  // block-uniform: one row, one class
            if (ws.b.cls[q0] != kBudLongCut) continue;
            const uint32_t slot = ws.b.pre[r0] >> kBudShortLog2;
            if (slot != cur_slot) {
                if (cur_slot != 0xFFFFFFFFu) {
                    __syncthreads();
                    if (bins[t]) atomicAdd(&hist[(uint64_t)cur_slot * kBudBins + t], bins[t]);
                    bins[t] = 0;
                    __syncthreads();
                }
                cur_slot = slot;
                cur_prefix = ws.sel[slot].prefix;
            }
            if (q < T) {
                const uint64_t key = ws.b.key[q];
                const uint32_t sz = ws.size[q];
                if (sz && bud_matches(key, cur_prefix, shift))
                    atomicAdd(&bins[bud_digit(key, shift)], (unsigned long long)sz);
            }
        } else if (q < T && ws.b.cls[q] == kBudLongCut) {
            const uint32_t slot = ws.b.pre[ws.b.row[q]] >> kBudShortLog2;
            const uint64_t key = ws.b.key[q];
            const uint32_t sz = ws.size[q];
            if (sz && bud_matches(key, ws.sel[slot].prefix, shift))
                atomicAdd(&hist[(uint64_t)slot * kBudBins + bud_digit(key, shift)], (unsigned long long)sz);
        }
    }
    if (cur_slot != 0xFFFFFFFFu) {
        __syncthreads();
        if (bins[t]) atomicAdd(&hist[(uint64_t)cur_slot * kBudBins + t], bins[t]);
    }
}

// One block per slot: lane t owns bin t; the block's prefix sum finds the bin in which the running
// byte total first exceeds what is left. The bins are read and zeroed.
__global__ __launch_bounds__(kBudBins) void k_byt_pick(BytWs ws, int shift) {
    __shared__ uint64_t wave_tot[kBudBins / 64];
    BudSelW* s = ws.sel + blockIdx.x;
    if (!s->active) return;  // block-uniform
    const uint64_t remaining = s->remaining;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint64_t* bin = ws.hist + (uint64_t)blockIdx.x * kBudBins + t;
    const uint64_t c = *bin;
    *bin = 0;
    uint64_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((unsigned long long)incl, d);
        if (lane >= (uint32_t)d) incl += o;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();  // also: every lane has read s->remaining
    uint64_t below = incl - c;
    for (uint32_t w = 0; w < wave; ++w) below += wave_tot[w];
    if (bud_picks_bytes(below, c, remaining)) {
        s->prefix |= (uint64_t)t << shift;
        s->remaining = remaining - below;
    }
}

// flags 0: ties (long cut rows, key == the row's threshold key); flags 1: keep. The keep pass reads
// ws.scan as the scan of the ties' sizes.
template <int kKeep>
__global__ __launch_bounds__(kBlock) void k_byt_flag(BytIn in, BytWs ws, uint32_t nG) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t g = (uint32_t)(q >> 6);
    if (g >= nG) return;  // wave-uniform
    const uint32_t T = ws.b.pre[in.b.n_peers];
    bool f = false;
    if (q < T) {
        const uint8_t c = ws.b.cls[q];
        if (!kKeep) {
            if (c == kBudLongCut) f = ws.b.key[q] == ws.sel[ws.b.pre[ws.b.row[q]] >> kBudShortLog2].prefix;
        } else if (c == kBudAll) {
            f = true;
        } else if (c == kBudShortCut) {
            const uint32_t p = ws.b.row[q];
            f = bud_short_keeps_bytes(ws.b.key, ws.size, ws.b.pre[p], ws.b.pre[p + 1] - ws.b.pre[p], (uint32_t)q,
                                      bud_wbudget(in.wbudget, in.w, p));
        } else if (c == kBudLongCut) {
            const uint32_t q0 = ws.b.pre[ws.b.row[q]];
            const BudSelW s = ws.sel[q0 >> kBudShortLog2];
            const uint64_t key = ws.b.key[q];
            uint64_t tie_bytes = 0;
            if (key == s.prefix) tie_bytes = ws.scan[q] - ws.scan[q0] + ws.size[q];
            f = bud_keeps_bytes(key, tie_bytes, s.prefix, s.remaining);
        }
    }
    const uint64_t word = __ballot(f);
    if ((threadIdx.x & 63u) == 0) {
        ws.b.words[(uint64_t)kKeep * nG + g] = word;
        ws.b.cnt[(uint64_t)kKeep * nG + g] = (uint32_t)__popcll(word);
    }
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
    out_bytes[p] = ws.scan[ws.b.pre[p + 1]] - ws.scan[ws.b.pre[p]];
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

// Exclusive u64 scan of the n terms f(0 .. n).
int scan_bytes(wq_router* h, const BytTerm& f, uint64_t* out, size_t n) {
    auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), f);
    size_t bytes = 0;
    WQ_HIP(h, rocprim::exclusive_scan(nullptr, bytes, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), h->stream));
    WQ_ALLOC(h, h->sort_tmp, bytes);
    WQ_HIP(h, rocprim::exclusive_scan(h->sort_tmp.p, bytes, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(),
                                      h->stream));
    return WQ_OK;
}

}  // namespace

void budget_release(wq_router* h) {
    h->bud_hist_clean = 0;
    h->byt_hist_clean = 0;
    for (DevBuf* b : {&h->bud_len, &h->bud_sum, &h->bud_pre, &h->bud_key, &h->bud_row, &h->bud_cls, &h->bud_sel,
                      &h->bud_hist, &h->bud_words, &h->bud_cnt, &h->bud_base, &h->bud_ctrl, &h->byt_size, &h->byt_scan,
                      &h->byt_sel, &h->byt_hist})
        b->release();
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
    WQ_ALLOC(h, h->bud_len, rows * 4);
    WQ_ALLOC(h, h->bud_sum, rows * 4);
    WQ_ALLOC(h, h->bud_pre, rows * 4);
    WQ_ALLOC(h, h->bud_key, n_in * 8);
    WQ_ALLOC(h, h->bud_row, n_in * 4);
    WQ_ALLOC(h, h->bud_cls, n_in);
    WQ_ALLOC(h, h->bud_sel, n_slots * sizeof(BudSel));
    WQ_ALLOC(h, h->bud_words, (size_t)nG * 16);
    WQ_ALLOC(h, h->bud_cnt, (size_t)nG * 8);
    WQ_ALLOC(h, h->bud_base, (size_t)nG * 8);
    WQ_ALLOC(h, h->bud_ctrl, 64);
    // The select needs every bin zero when a call starts. Every pick pass zeroes the bins it read, so
    // a call that launched all its passes leaves them zero: bud_hist_clean is the number of bytes
    // known to be zero. It is 0 for a new allocation (decided from the capacity, not the address:
    // a freed block's address can come back) and while a call's passes are being launched, so a
    // call that failed between a histogram pass and its pick makes the next one clear the buffer.
    const size_t hist_cap = h->bud_hist.bytes;
    WQ_ALLOC(h, h->bud_hist, n_slots * kBudBins * 4);
    if (h->bud_hist.bytes != hist_cap) h->bud_hist_clean = 0;
    if (h->bud_hist_clean < h->bud_hist.bytes) {
        WQ_HIP(h, hipMemsetAsync(h->bud_hist.p, 0, h->bud_hist.bytes, s));
        h->bud_hist_clean = h->bud_hist.bytes;
    }
    WQ_HIP(h, hipMemsetAsync(h->bud_ctrl.p, 0, 64, s));
    WQ_HIP(h, hipMemsetAsync(h->bud_sel.p, 0, n_slots * sizeof(BudSel), s));

    const BudIn in{d_peer_offsets, d_msgs,      d_msg_pos,         d_peer_pos,           d_budget,
                   n_peers,        (uint32_t)n_in, (uint32_t)std::min<size_t>(n_msgs, 0xFFFFFFFFull),
                   (uint32_t)std::min<size_t>(n_peer_pos, 0xFFFFFFFFull), k};
    const BudWs ws{h->bud_len.as<uint32_t>(), h->bud_sum.as<uint32_t>(),  h->bud_pre.as<uint32_t>(),
                   h->bud_key.as<uint64_t>(), h->bud_row.as<uint32_t>(),  h->bud_cls.as<uint8_t>(),
                   h->bud_sel.as<BudSel>(),   h->bud_hist.as<uint32_t>(), h->bud_words.as<uint64_t>(),
                   h->bud_cnt.as<uint32_t>(), h->bud_base.as<uint32_t>(), h->bud_ctrl.as<uint32_t>()};

    const dim3 blk(kBlock);
    const dim3 grid_r(grid_for(rows));
    hipLaunchKernelGGL(k_bud_len, grid_r, blk, 0, s, in, ws);
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
        h->bud_hist_clean = 0;  // until every pass has its pick
        for (int pass = 0; pass < kBudPasses; ++pass) {
            hipLaunchKernelGGL(k_bud_hist, dim3(grid_for((n_in + kBudTiles - 1) / kBudTiles)), blk, 0, s, ws, n_peers,
                               bud_shift(pass));
            WQ_HIP(h, hipGetLastError());
            hipLaunchKernelGGL(k_bud_pick, dim3((unsigned)n_slots), dim3(kBudBins), 0, s, ws, bud_shift(pass));
            WQ_HIP(h, hipGetLastError());
        }
        h->bud_hist_clean = h->bud_hist.bytes;
        hipLaunchKernelGGL(k_bud_flag<0>, grid_g, blk, 0, s, in, ws, nG);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_u32(h, ws.cnt, ws.base, nG, false)) return rc;
        hipLaunchKernelGGL(k_bud_flag<1>, grid_g, blk, 0, s, in, ws, nG);
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
// The per-peer and per-ordinal arrays, the flag words and ctrl are the count budget's buffers: the
// calls are ordered on the handle's stream and nothing in them outlives a call. The select's state
// and histograms, which must be zero between calls, are this path's own.
int launch_peer_budget_bytes(wq_router* h, const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers,
                             size_t n_in, const double* d_msg_pos, const uint32_t* d_msg_size, size_t n_msgs,
                             const double* d_peer_pos, size_t n_peer_pos, uint64_t w, const uint64_t* d_budget_bytes,
                             uint32_t* d_out_offsets, uint32_t* d_out_msgs, uint64_t* d_out_bytes,
                             wq_budget_bytes_counters* d_counters) {
    hipStream_t s = h->stream;
    const size_t rows = (size_t)n_peers + 1;
    const size_t n_slots = n_in / kBudShort + 1;
    const uint32_t nG = (uint32_t)(n_in / 64 + 1);
    WQ_ALLOC(h, h->bud_len, rows * 4);
    WQ_ALLOC(h, h->bud_sum, rows * 4);
    WQ_ALLOC(h, h->bud_pre, rows * 4);
    WQ_ALLOC(h, h->bud_key, n_in * 8);
    WQ_ALLOC(h, h->bud_row, n_in * 4);
    WQ_ALLOC(h, h->bud_cls, n_in);
    WQ_ALLOC(h, h->bud_words, (size_t)nG * 16);
    WQ_ALLOC(h, h->bud_cnt, (size_t)nG * 8);
    WQ_ALLOC(h, h->bud_base, (size_t)nG * 8);
    WQ_ALLOC(h, h->bud_ctrl, 64);
    WQ_ALLOC(h, h->byt_size, n_in * 4);
    WQ_ALLOC(h, h->byt_scan, (n_in + 1) * 8);
    WQ_ALLOC(h, h->byt_sel, n_slots * sizeof(BudSelW));
    // byt_hist_clean: as bud_hist_clean above, for this path's own histograms.
    const size_t hist_cap = h->byt_hist.bytes;
    WQ_ALLOC(h, h->byt_hist, n_slots * kBudBins * 8);
    if (h->byt_hist.bytes != hist_cap) h->byt_hist_clean = 0;
    if (h->byt_hist_clean < h->byt_hist.bytes) {
        WQ_HIP(h, hipMemsetAsync(h->byt_hist.p, 0, h->byt_hist.bytes, s));
        h->byt_hist_clean = h->byt_hist.bytes;
    }
    WQ_HIP(h, hipMemsetAsync(h->bud_ctrl.p, 0, 64, s));
    WQ_HIP(h, hipMemsetAsync(h->byt_sel.p, 0, n_slots * sizeof(BudSelW), s));

    const BytIn in{BudIn{d_peer_offsets, d_msgs, d_msg_pos, d_peer_pos, nullptr, n_peers, (uint32_t)n_in,
                         (uint32_t)std::min<size_t>(n_msgs, 0xFFFFFFFFull),
                         (uint32_t)std::min<size_t>(n_peer_pos, 0xFFFFFFFFull), 0u},
                   d_msg_size, d_budget_bytes, w};
    const BytWs ws{BudWs{h->bud_len.as<uint32_t>(), h->bud_sum.as<uint32_t>(), h->bud_pre.as<uint32_t>(),
                         h->bud_key.as<uint64_t>(), h->bud_row.as<uint32_t>(), h->bud_cls.as<uint8_t>(), nullptr, nullptr,
                         h->bud_words.as<uint64_t>(), h->bud_cnt.as<uint32_t>(), h->bud_base.as<uint32_t>(),
                         h->bud_ctrl.as<uint32_t>()},
                   h->byt_size.as<uint32_t>(), h->byt_scan.as<uint64_t>(), h->byt_sel.as<BudSelW>(),
                   h->byt_hist.as<uint64_t>()};

    const dim3 blk(kBlock);
    const dim3 grid_r(grid_for(rows));
    hipLaunchKernelGGL(k_bud_len, grid_r, blk, 0, s, in.b, ws.b);
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_sat(h, ws.b.len, ws.b.sum, rows)) return rc;
    hipLaunchKernelGGL(k_byt_pre, grid_r, blk, 0, s, in.b, ws.b);
    WQ_HIP(h, hipGetLastError());
    const uint32_t* d_T = ws.b.pre + n_peers;
    const uint64_t* kept_scan = nullptr;
    if (n_in) {
        const dim3 grid_e(grid_for(n_in));
        const dim3 grid_g(grid_for((uint64_t)nG * 64));
        hipLaunchKernelGGL(k_byt_keys, grid_e, blk, 0, s, in, ws);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_bytes(h, BytTerm{ws.size, nullptr, d_T}, ws.scan, n_in + 1)) return rc;
        hipLaunchKernelGGL(k_byt_class, grid_r, blk, 0, s, in, ws);
        WQ_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_byt_cls, grid_e, blk, 0, s, ws, n_peers);
        WQ_HIP(h, hipGetLastError());
        h->byt_hist_clean = 0;  // until every pass has its pick
        for (int pass = 0; pass < kBudPasses; ++pass) {
            hipLaunchKernelGGL(k_byt_hist, dim3(grid_for((n_in + kBudTiles - 1) / kBudTiles)), blk, 0, s, ws, n_peers,
                               bud_shift(pass));
            WQ_HIP(h, hipGetLastError());
            hipLaunchKernelGGL(k_byt_pick, dim3((unsigned)n_slots), dim3(kBudBins), 0, s, ws, bud_shift(pass));
            WQ_HIP(h, hipGetLastError());
        }
        h->byt_hist_clean = h->byt_hist.bytes;
        hipLaunchKernelGGL(k_byt_flag<0>, grid_g, blk, 0, s, in, ws, nG);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_bytes(h, BytTerm{ws.size, ws.b.words, d_T}, ws.scan, n_in + 1)) return rc;
        hipLaunchKernelGGL(k_byt_flag<1>, grid_g, blk, 0, s, in, ws, nG);
        WQ_HIP(h, hipGetLastError());
        if (int rc = scan_u32(h, ws.b.cnt + nG, ws.b.base + nG, nG, false)) return rc;
        hipLaunchKernelGGL(k_byt_offsets, grid_r, blk, 0, s, ws.b, n_peers, nG, d_out_offsets);
        WQ_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_bud_emit, grid_e, blk, 0, s, in.b, ws.b, nG, d_out_msgs);
        WQ_HIP(h, hipGetLastError());
        if (d_out_bytes || d_counters) {
            if (int rc = scan_bytes(h, BytTerm{ws.size, ws.b.words + nG, d_T}, ws.scan, n_in + 1)) return rc;
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
        hipLaunchKernelGGL(k_byt_counters, dim3(1), dim3(1), 0, s, ws.b, n_peers, d_out_offsets, kept_scan, d_counters);
        WQ_HIP(h, hipGetLastError());
    }
    return WQ_OK;
}

}  // namespace wq
