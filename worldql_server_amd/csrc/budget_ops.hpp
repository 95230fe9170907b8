// budget_ops.hpp — the per-element arithmetic of the per-observer send budgets (wq_budget.hip): the
// clamped row lengths and their ordinal space, the distance key of an element with its NaN / missing
// rule and u64 image, the class of a row, the rank of an element of a short row, the digit and match
// tests of the radix select and the keep predicate. __host__ __device__, so
// tests/cpp/peer_budget_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/interest.py (peer_budget_np). The byte budgets' additions are at the end of the
// file (tests/cpp/peer_budget_bytes_host_shim.hip, peer_budget_bytes_np).
//
// Ordinals. Row p is the part of [off[p], off[p + 1]) inside [0, n_in) (pm_row_bounds). The rows'
// lengths are summed with a saturating add and the sums clamped to n_in: row p owns the ordinals
// [pre[p], pre[p + 1]), and ordinal q of row p is input element a_p + (q - pre[p]). For ascending
// offsets the clamp never bites (the rows are disjoint parts of [0, n_in)); offsets that descend can
// make rows overlap, and then the rows behind the first n_in elements are cut short or empty. Either
// way there are at most n_in ordinals, so every per-element array has n_in entries and the output,
// a stable compaction of the ordinals, never passes n_in.
#pragma once

#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "peer_major_ops.hpp"

namespace wq {

// Rows of at most kBudShort elements are ranked by counting; longer ones go through the radix
// select, whose per-row histogram lives in slot pre[p] / kBudShort (two rows longer than kBudShort
// start more than kBudShort ordinals apart: no slot is shared).
constexpr uint32_t kBudShort = 256;
constexpr uint32_t kBudShortLog2 = 8;
constexpr int kBudDigitBits = 8;
constexpr uint32_t kBudBins = 1u << kBudDigitBits;
constexpr int kBudPasses = 64 / kBudDigitBits;
// A histogram pass counts a tile of kBudTile ordinals that lie in one row in LDS; a block takes
// kBudTiles tiles (wq_budget.hip k_sel_hist).
constexpr uint32_t kBudTile = 256;
constexpr uint32_t kBudTiles = 8;
constexpr uint64_t kBudInf = 0x7FF0000000000000ull;  // the bits of +infinity
constexpr uint32_t kBudErrRows = 1u, kBudErrMsg = 2u;

// A row's class: how its keep flags are decided.
enum : uint8_t { kBudAll = 0, kBudNone = 1, kBudShortCut = 2, kBudLongCut = 3 };

// The radix select's state of one long cut row: the digits chosen so far, the elements still to keep
// among the keys that match them, and whether the slot holds a row at all. After the last pass:
// the row's threshold key and the number of elements with exactly that key that are kept.
struct BudSel {
    uint64_t prefix;
    uint32_t need;
    uint32_t active;
};

struct BudSatAdd {
    __host__ __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const {
        const uint64_t s = (uint64_t)a + b;
        return s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
    }
};

// Length of the clamped row p; *ok false when the offsets descend or reach past n_in.
__host__ __device__ __forceinline__ uint32_t bud_len(const uint32_t* __restrict__ off, uint32_t p, uint32_t n_in,
                                                     bool* ok) {
    uint32_t a, b;
    pm_row_bounds(off, p, n_in, a, b);
    *ok = off[p] <= off[p + 1] && off[p + 1] <= n_in;
    return b - a;
}

// First input element of row p.
__host__ __device__ __forceinline__ uint32_t bud_row_start(const uint32_t* __restrict__ off, uint32_t p,
                                                           uint32_t n_in) {
    return off[p] < n_in ? off[p] : n_in;
}

__host__ __device__ __forceinline__ uint32_t bud_budget(const uint32_t* __restrict__ budget, uint32_t k, uint32_t p) {
    return budget ? budget[p] : k;
}

__host__ __device__ __forceinline__ uint8_t bud_class(uint32_t len, uint32_t B) {
    if (len <= B) return kBudAll;
    if (B == 0) return kBudNone;
    return len <= kBudShort ? kBudShortCut : kBudLongCut;
}

// The row that owns ordinal q < pre[n_peers]: the last p with pre[p] <= q (pre ascends from 0, so
// pre[p + 1] > q and p < n_peers).
__host__ __device__ __forceinline__ uint32_t bud_row_of(const uint32_t* __restrict__ pre, uint32_t n_peers,
                                                        uint32_t q) {
    uint32_t lo = 0, hi = n_peers;
    while (hi > lo) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (pre[mid] <= q)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The radius filter's squared distance (include/wq_router.h, "C5: exact radius filter"): f64, left
// to right, no contraction.
__host__ __device__ __forceinline__ double bud_d2(double mx, double my, double mz, double px, double py, double pz) {
    const double dx = mx - px;
    const double dy = my - py;
    const double dz = mz - pz;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return d2;
}

// The u64 image of d2: a sum of squares is never negative, and non-negative doubles order as their
// bit patterns; NaN counts as +infinity.
__host__ __device__ __forceinline__ uint64_t bud_image(double d2) {
    if (d2 != d2) return kBudInf;
    uint64_t u;
    memcpy(&u, &d2, 8);
    return u & 0x7FFFFFFFFFFFFFFFull;
}

// Key of the element with message m seen from peer p. +infinity without reading a position when the
// message or the peer has none; *bad_msg when m >= n_msgs.
__host__ __device__ __forceinline__ uint64_t bud_key(const double* __restrict__ mpos, uint32_t n_msgs,
                                                     const double* __restrict__ ppos, uint32_t n_ppos, uint32_t p,
                                                     uint32_t m, bool* bad_msg) {
    *bad_msg = m >= n_msgs;
    if (m >= n_msgs || p >= n_ppos) return kBudInf;
    const double* a = mpos + 3ull * m;
    const double* b = ppos + 3ull * p;
    return bud_image(bud_d2(a[0], a[1], a[2], b[0], b[1], b[2]));
}

// Short cut row [q0, q0 + len): is ordinal q among the B smallest by (key, position)? Its rank is
// the count of the row's elements before it in that order.
__host__ __device__ __forceinline__ bool bud_short_keeps(const uint64_t* __restrict__ key, uint32_t q0, uint32_t len,
                                                         uint32_t q, uint32_t B) {
    const uint64_t mine = key[q];
    uint32_t rank = 0;
    for (uint32_t i = q0; i < q0 + len; ++i) {
        const uint64_t o = key[i];
        rank += (o < mine || (o == mine && i < q)) ? 1u : 0u;
    }
    return rank < B;
}

// Radix select, pass d of kBudPasses (the top digit first).
__host__ __device__ __forceinline__ int bud_shift(int pass) { return 64 - kBudDigitBits * (pass + 1); }
__host__ __device__ __forceinline__ uint32_t bud_digit(uint64_t key, int shift) {
    return (uint32_t)(key >> shift) & (kBudBins - 1u);
}
// Does the key agree with the digits chosen in the passes before the one at `shift`?
__host__ __device__ __forceinline__ bool bud_matches(uint64_t key, uint64_t prefix, int shift) {
    return shift + kBudDigitBits >= 64 || ((key ^ prefix) >> (shift + kBudDigitBits)) == 0;
}
// The bin whose keys hold the need-th smallest: below = the matching keys in lower bins.
__host__ __device__ __forceinline__ bool bud_picks(uint32_t below, uint32_t count, uint32_t need) {
    return below < need && need - below <= count;
}

// Long cut row after the select: an element is kept when its key is below the row's threshold key,
// or equal to it and among the first thr_ties such elements of the row (tie_rank: the elements with
// the threshold key before it in the row). The last kept tie is the row's threshold position.
__host__ __device__ __forceinline__ bool bud_keeps(uint64_t key, uint32_t tie_rank, uint64_t thr_key,
                                                   uint32_t thr_ties) {
    return key < thr_key || (key == thr_key && tie_rank < thr_ties);
}

// The flag of position x in a granule's flag words.
__host__ __device__ __forceinline__ bool flag_at(const uint64_t* __restrict__ words, uint64_t x) {
    return (words[x >> 6] >> (x & 63u)) & 1ull;
}

// Bits set below position x in a granule's flag words: prefix base[] + popcount (x < 64 * granules).
__host__ __device__ __forceinline__ uint32_t bud_before(const uint32_t* __restrict__ base,
                                                        const uint64_t* __restrict__ words, uint32_t x) {
    const uint64_t below = words[x >> 6] & ((1ull << (x & 63u)) - 1ull);
#if defined(__HIP_DEVICE_COMPILE__)
    return base[x >> 6] + (uint32_t)__popcll(below);
#else
    return base[x >> 6] + (uint32_t)__builtin_popcountll(below);
#endif
}

// ---- byte budgets (wq_peer_budget_bytes_device): the same ordinal space, keys, classes of cut rows
// and flag words; the select sums sizes where the count budget counts keys. An element is kept iff
// the sizes of the row's elements at or before it in (key, position) order sum to at most W, in u64:
// a row has fewer than 2^32 elements of less than 2^32 bytes each, so no sum wraps.

// The weighted select's state of one long cut row: the digits chosen so far and the bytes still free
// for the keys that match them. After the last pass: the row's threshold key and the bytes left for
// the elements with exactly that key.
struct BudSelW {
    uint64_t prefix;
    uint64_t remaining;
    uint32_t active;
    uint32_t pad;
};

__host__ __device__ __forceinline__ uint64_t bud_wbudget(const uint64_t* __restrict__ budget, uint64_t w, uint32_t p) {
    return budget ? budget[p] : w;
}

// Size of the element with message m: 0, without a read, when the message does not exist.
__host__ __device__ __forceinline__ uint32_t bud_size(const uint32_t* __restrict__ msize, uint32_t n_msgs, uint32_t m) {
    return m < n_msgs ? msize[m] : 0u;
}

// A row whose total fits is copied; a cut one is decided by summing in the row (short) or by the
// weighted select (long). A cut row loses at least its last element in (key, position) order.
__host__ __device__ __forceinline__ uint8_t bud_class_bytes(uint32_t len, uint64_t total, uint64_t W) {
    if (total <= W) return kBudAll;
    return len <= kBudShort ? kBudShortCut : kBudLongCut;
}

// The term of ordinal q in a scan of bytes over the ordinals: its size, 0 behind the T ordinals and,
// with flag words, 0 when its flag is not set.
__host__ __device__ __forceinline__ uint64_t bud_byte_term(const uint32_t* __restrict__ size,
                                                           const uint64_t* __restrict__ words, uint32_t T,
                                                           uint64_t q) {
    if (q >= T) return 0;
    if (words && !flag_at(words, q)) return 0;
    return size[q];
}

// Short cut row [q0, q0 + len): do the sizes of the elements not after ordinal q in (key, position)
// order, its own included, fit in W?
__host__ __device__ __forceinline__ bool bud_short_keeps_bytes(const uint64_t* __restrict__ key,
                                                               const uint32_t* __restrict__ size, uint32_t q0,
                                                               uint32_t len, uint32_t q, uint64_t W) {
    const uint64_t mine = key[q];
    uint64_t sum = 0;
    for (uint32_t i = q0; i < q0 + len; ++i) {
        const uint64_t o = key[i];
        sum += (o < mine || (o == mine && i <= q)) ? (uint64_t)size[i] : 0ull;
    }
    return sum <= W;
}

// The bin in which the running byte total first exceeds `remaining`: below = the bytes of the
// matching keys in lower bins. A cut row's matching bytes exceed `remaining`, so exactly one bin is
// picked; bins of zero-size elements are never picked.
__host__ __device__ __forceinline__ bool bud_picks_bytes(uint64_t below, uint64_t bytes, uint64_t remaining) {
    return below <= remaining && remaining - below < bytes;
}

// Long cut row after the weighted select: kept below the threshold key, and at it while the bytes of
// the row's threshold-key elements up to and including this one (tie_bytes) fit in thr_bytes.
__host__ __device__ __forceinline__ bool bud_keeps_bytes(uint64_t key, uint64_t tie_bytes, uint64_t thr_key,
                                                         uint64_t thr_bytes) {
    return key < thr_key || (key == thr_key && tie_bytes <= thr_bytes);
}

}  // namespace wq
