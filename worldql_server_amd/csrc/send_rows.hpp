// send_rows.hpp — the device glue the send-side calls share (wq_budget.hip, wq_rotate.hip,
// wq_pack.hip, wq_frames.hip) around the arithmetic of budget_ops.hpp: the ordinal space of a
// peer-major CSR, the scans over it and the granules' flag words. Everything is TU-local (anonymous
// namespace), as table_prims.hpp.
//
// The ordinal space (budget_ops.hpp, "Ordinals") takes a launch, a scan and a launch:
//
//   len   one lane per row and one behind them: the clamped length, 0 at n_peers
//   scan  scan_sat: the saturating exclusive prefix of the lengths
//   pre   one lane per row and one behind them: the prefix clamped to n_in; a row whose clamped
//         prefix leaves it fewer ordinals than its length overlaps another one: the error bit
//
// A call whose lane does nothing else launches k_rows_len / k_rows_pre; one that has more to do per
// peer, or two CSRs to walk, calls rows_len_step / rows_pre_step from a kernel of its own.
#pragma once

#include "budget_ops.hpp"
#include "table_prims.hpp"

namespace wq {
namespace {

// One CSR's rows and the three buffers of its ordinal space, each of n_peers + 1 entries.
struct RowSpace {
    const uint32_t* off;
    uint32_t n_peers, n_in;
    uint32_t* len;  // clamped lengths
    uint32_t* sum;  // their saturating prefix
    uint32_t* pre;  // the prefix clamped to n_in: row p owns the ordinals [pre[p], pre[p + 1])
};

// Lane p <= n_peers of the length step; `bit` goes into *err when the offsets descend or pass n_in.
__device__ __forceinline__ void rows_len_step(const RowSpace& r, uint64_t p, uint32_t* err, uint32_t bit) {
    bool ok = true;
    r.len[p] = p < r.n_peers ? bud_len(r.off, (uint32_t)p, r.n_in, &ok) : 0u;
    if (!ok) atomicOr(err, bit);
}

// Lane p <= n_peers of the pre step: stores and returns pre[p]; *n is the row's count of ordinals,
// 0 for the lane behind the rows.
__device__ __forceinline__ uint32_t rows_pre_step(const RowSpace& r, uint64_t p, uint32_t* err, uint32_t bit,
                                                  uint32_t* n) {
    const uint32_t a = r.sum[p] < r.n_in ? r.sum[p] : r.n_in;
    r.pre[p] = a;
    *n = 0;
    if (p == r.n_peers) return a;
    const uint32_t b = r.sum[p + 1] < r.n_in ? r.sum[p + 1] : r.n_in;
    *n = b - a;
    if (b - a != r.len[p]) atomicOr(err, bit);  // overlapping rows: cut at n_in ordinals
    return a;
}

__global__ __launch_bounds__(kBlock) void k_rows_len(RowSpace r, uint32_t* err, uint32_t bit) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > r.n_peers) return;
    rows_len_step(r, p, err, bit);
}

__global__ __launch_bounds__(kBlock) void k_rows_pre(RowSpace r, uint32_t* err, uint32_t bit) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > r.n_peers) return;
    uint32_t n;
    rows_pre_step(r, p, err, bit, &n);
}

// The input element of ordinal q of row p.
__device__ __forceinline__ uint32_t rows_elem(const uint32_t* __restrict__ off, const uint32_t* __restrict__ pre,
                                              uint32_t n_in, uint32_t p, uint32_t q) {
    return bud_row_start(off, p, n_in) + (q - pre[p]);
}

// The rows' three buffers are the handle's bud_len / bud_sum / bud_pre in every call: the calls are
// ordered on the handle's stream and no ordinal space outlives its call.
int rows_alloc(wq_router* h, size_t rows) {
    WQ_ALLOC(h, h->bud_len, rows * 4);
    WQ_ALLOC(h, h->bud_sum, rows * 4);
    WQ_ALLOC(h, h->bud_pre, rows * 4);
    return WQ_OK;
}

RowSpace rows_view(wq_router* h, const uint32_t* off, uint32_t n_peers, size_t n_in) {
    return RowSpace{off, n_peers, (uint32_t)n_in, h->bud_len.as<uint32_t>(), h->bud_sum.as<uint32_t>(),
                    h->bud_pre.as<uint32_t>()};
}

// ---- scans (temp storage in h->sort_tmp) ----

// Exclusive scan of in[0 .. n) under the associative `op` (it need not commute), from `zero`.
template <class In, class T, class Op>
int scan_excl(wq_router* h, In in, T* out, const T& zero, size_t n, Op op) {
    size_t bytes = 0;
    WQ_HIP(h, rocprim::exclusive_scan(nullptr, bytes, in, out, zero, n, op, h->stream));
    WQ_ALLOC(h, h->sort_tmp, bytes);
    WQ_HIP(h, rocprim::exclusive_scan(h->sort_tmp.p, bytes, in, out, zero, n, op, h->stream));
    return WQ_OK;
}

int scan_sat(wq_router* h, const uint32_t* in, uint32_t* out, size_t n) { return scan_excl(h, in, out, 0u, n, BudSatAdd()); }

// Exclusive scan of the n terms f(0 .. n).
template <class F, class T, class Op>
int scan_terms(wq_router* h, const F& f, T* out, const T& zero, size_t n, Op op) {
    return scan_excl(h, rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), f), out, zero, n, op);
}
template <class F>
int scan_terms(wq_router* h, const F& f, uint64_t* out, size_t n) {
    return scan_terms(h, f, out, (uint64_t)0, n, rocprim::plus<uint64_t>());
}

// The size of ordinal q, 0 behind the *T ordinals and, with flag words, where its flag is not set.
struct SizeTerm {
    const uint32_t* size;
    const uint64_t* words;  // nullable
    const uint32_t* T;
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t q) const {
        return bud_byte_term(size, words, *T, q);
    }
};

// ---- flag words: one u64 per granule of 64 ordinals (read with flag_at and bud_before) ----

// Every lane of a wave brings its flag: the first lane stores the granule's word and its popcount.
__device__ __forceinline__ void store_flags(uint64_t* words, uint32_t* cnt, uint64_t index, bool f) {
    const uint64_t word = __ballot(f);
    if ((threadIdx.x & 63u) == 0) {
        words[index] = word;
        cnt[index] = (uint32_t)__popcll(word);
    }
}

}  // namespace
}  // namespace wq
