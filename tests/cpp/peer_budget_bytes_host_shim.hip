// Test-only shim: runs the byte budgets' arithmetic (csrc/budget_ops.hpp: the count budget's rows, keys
// and flag words, and the size of an element, the class of a row from its total, the term of a byte
// scan, the weighted rank in a short row, the weighted pick and the keep predicate) on the CPU in the
// passes the kernels of csrc/wq_budget.hip use — rows, saturating scan, the ordinal space, keys and
// sizes, the scan of the sizes, classes, eight histogram-and-pick passes on u64 bins that are zeroed
// on the pick, tie flags, the scan of the ties' sizes, keep flags, offsets from the keep words, emit,
// the scan of the kept sizes — so the result is checked byte for byte against
// worldql_server_amd/interest.py (peer_budget_bytes_np) without a GPU
// (tests/test_peer_budget_bytes_cpp_mirror.py). The GPU instance: tests/test_gpu_peer_budget_bytes.py.
//
// The select's state and histograms are the caller's (`sel`, `hist`), as the handle's are the
// kernels': a second call on the same buffers must find every bin zero.
//
// With -DWQ_PEER_BUDGET_BYTES_SHIM_MAIN the file is a program of its own: random and hostile inputs
// on exactly sized vectors, for a host build under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../worldql_server_amd/csrc/budget_ops.hpp"

extern "C" uint32_t wq_test_budget_bytes_short() { return wq::kBudShort; }
extern "C" uint32_t wq_test_budget_bytes_digit_bits() { return (uint32_t)wq::kBudDigitBits; }
extern "C" uint32_t wq_test_budget_bytes_tile() { return wq::kBudTile; }
extern "C" uint32_t wq_test_budget_bytes_tiles() { return wq::kBudTiles; }
extern "C" size_t wq_test_budget_bytes_slots(size_t n_in) { return n_in / wq::kBudShort + 1; }

// As wq_peer_budget_bytes_device with the positions given. hist: kBudBins u64 per slot, all zero on
// entry and on return; counters = {n_in, n_kept, bytes_in, bytes_kept, rows_cut, error}. Returns the
// number of bins found non-zero on entry.
extern "C" uint64_t wq_test_peer_budget_bytes_host(const uint32_t* off, const uint32_t* msgs, uint32_t n_peers,
                                                   size_t n_in_, const double* mpos, const uint32_t* msize,
                                                   size_t n_msgs, const double* ppos, size_t n_ppos, uint64_t w,
                                                   const uint64_t* budget, uint64_t* hist, uint32_t* out_off,
                                                   uint32_t* out_msgs, uint64_t* out_bytes, uint64_t* counters) {
    using namespace wq;
    const uint32_t n_in = (uint32_t)n_in_;
    const size_t rows = (size_t)n_peers + 1;
    const size_t n_slots = n_in / kBudShort + 1;
    uint32_t rows_cut = 0, error = 0;
    uint64_t dirty = 0;
    for (size_t i = 0; i < n_slots * kBudBins; ++i) dirty += hist[i] != 0;
    // rows: lengths, saturating prefix, the ordinal space
    std::vector<uint32_t> len(rows, 0), sum(rows, 0), pre(rows, 0);
    for (uint32_t p = 0; p < n_peers; ++p) {
        bool ok;
        len[p] = bud_len(off, p, n_in, &ok);
        if (!ok) error |= kBudErrRows;
    }
    for (size_t p = 1; p < rows; ++p) sum[p] = BudSatAdd()(sum[p - 1], len[p - 1]);
    for (size_t p = 0; p < rows; ++p) pre[p] = std::min(sum[p], n_in);
    for (uint32_t p = 0; p < n_peers; ++p)
        if (pre[p + 1] - pre[p] != len[p]) error |= kBudErrRows;
    const uint32_t T = pre[n_peers];
    // keys and sizes
    std::vector<uint64_t> key(T);
    std::vector<uint32_t> row(T), size(T);
    for (uint32_t q = 0; q < T; ++q) {
        const uint32_t p = bud_row_of(pre.data(), n_peers, q);
        const uint32_t j = bud_row_start(off, p, n_in) + (q - pre[p]);
        bool bad;
        key[q] = bud_key(mpos, (uint32_t)n_msgs, ppos, (uint32_t)n_ppos, p, msgs[j], &bad);
        row[q] = p;
        size[q] = bud_size(msize, (uint32_t)n_msgs, msgs[j]);
        if (bad) error |= kBudErrMsg;
    }
    // one scan buffer for the three byte scans, n_in + 1 entries
    std::vector<uint64_t> scan((size_t)n_in + 1, 0);
    auto scan_bytes = [&](const uint64_t* words) {
        uint64_t at = 0;
        for (uint64_t q = 0; q <= n_in; ++q) {
            scan[q] = at;
            at += bud_byte_term(size.data(), words, T, q);
        }
    };
    scan_bytes(nullptr);
    const uint64_t bytes_in = scan[T];
    // classes
    std::vector<uint8_t> rcls(rows, 0), cls(T);
    std::vector<BudSelW> sel(n_slots, BudSelW{0, 0, 0, 0});
    for (uint32_t p = 0; p < n_peers; ++p) {
        const uint64_t W = bud_wbudget(budget, w, p);
        rcls[p] = bud_class_bytes(pre[p + 1] - pre[p], scan[pre[p + 1]] - scan[pre[p]], W);
        if (rcls[p] != kBudAll) rows_cut++;
        if (rcls[p] == kBudLongCut) sel[pre[p] >> kBudShortLog2] = BudSelW{0, W, 1, 0};
    }
    for (uint32_t q = 0; q < T; ++q) cls[q] = rcls[row[q]];
    // weighted select
    for (int pass = 0; pass < kBudPasses; ++pass) {
        const int shift = bud_shift(pass);
        for (uint32_t q = 0; q < T; ++q) {
            if (cls[q] != kBudLongCut) continue;
            const size_t slot = pre[row[q]] >> kBudShortLog2;
            if (size[q] && bud_matches(key[q], sel[slot].prefix, shift))
                hist[slot * kBudBins + bud_digit(key[q], shift)] += size[q];
        }
        for (size_t slot = 0; slot < n_slots; ++slot) {
            if (!sel[slot].active) continue;
            const uint64_t remaining = sel[slot].remaining;
            uint64_t below = 0;
            for (uint32_t t = 0; t < kBudBins; ++t) {
                const uint64_t c = hist[slot * kBudBins + t];
                hist[slot * kBudBins + t] = 0;
                if (bud_picks_bytes(below, c, remaining)) {
                    sel[slot].prefix |= (uint64_t)t << shift;
                    sel[slot].remaining = remaining - below;
                }
                below += c;
            }
        }
    }
    // tie flags, keep flags: a word and a prefix per granule of 64 ordinals
    const uint32_t nG = n_in / 64 + 1;
    std::vector<uint64_t> words(2 * (size_t)nG, 0);
    std::vector<uint32_t> base(2 * (size_t)nG, 0);
    for (uint32_t q = 0; q < T; ++q)
        if (cls[q] == kBudLongCut && key[q] == sel[pre[row[q]] >> kBudShortLog2].prefix) words[q >> 6] |= 1ull << (q & 63);
    scan_bytes(words.data());
    for (uint32_t q = 0; q < T; ++q) {
        bool f = false;
        const uint32_t p = row[q];
        if (cls[q] == kBudAll) {
            f = true;
        } else if (cls[q] == kBudShortCut) {
            f = bud_short_keeps_bytes(key.data(), size.data(), pre[p], pre[p + 1] - pre[p], q, bud_wbudget(budget, w, p));
        } else if (cls[q] == kBudLongCut) {
            const BudSelW s = sel[pre[p] >> kBudShortLog2];
            uint64_t tie_bytes = 0;
            if (key[q] == s.prefix) tie_bytes = scan[q] - scan[pre[p]] + size[q];
            f = bud_keeps_bytes(key[q], tie_bytes, s.prefix, s.remaining);
        }
        if (f) words[(size_t)nG + (q >> 6)] |= 1ull << (q & 63);
    }
    uint32_t at = 0;
    for (uint32_t g = 0; g < nG; ++g) {
        base[(size_t)nG + g] = at;
        at += (uint32_t)__builtin_popcountll(words[(size_t)nG + g]);
    }
    // offsets from the keep words, emit
    for (size_t p = 0; p < rows; ++p) out_off[p] = bud_before(base.data() + nG, words.data() + nG, pre[p]);
    for (uint32_t q = 0; q < T; ++q) {
        if (!((words[(size_t)nG + (q >> 6)] >> (q & 63)) & 1ull)) continue;
        const uint32_t p = row[q];
        const uint32_t j = bud_row_start(off, p, n_in) + (q - pre[p]);
        const uint32_t pos = bud_before(base.data() + nG, words.data() + nG, q);
        if (pos < n_in) out_msgs[pos] = msgs[j];
    }
    scan_bytes(words.data() + nG);
    if (out_bytes)
        for (uint32_t p = 0; p < n_peers; ++p) out_bytes[p] = scan[pre[p + 1]] - scan[pre[p]];
    if (counters) {
        counters[0] = T;
        counters[1] = out_off[n_peers];
        counters[2] = bytes_in;
        counters[3] = scan[T];
        counters[4] = rows_cut;
        counters[5] = error;
    }
    return dirty;
}

#ifdef WQ_PEER_BUDGET_BYTES_SHIM_MAIN
#include <math.h>
#include <stdio.h>

#include <random>

namespace {

struct Case {
    std::vector<uint32_t> off, msgs, msize;
    std::vector<uint64_t> budget;
    std::vector<double> mpos, ppos;
    uint32_t n_peers;
    uint64_t w;
    bool with_budget;
};

struct Out {
    std::vector<uint32_t> oo, om;
    std::vector<uint64_t> ob;
    uint64_t cnt[6];
    uint64_t dirty;
};

// Exactly sized buffers: the address sanitizer sees any read or write past an array. The histograms
// live across the calls of one size, as the handle's do.
Out run(const Case& c, std::vector<uint64_t>& hist) {
    const size_t need = wq_test_budget_bytes_slots(c.msgs.size()) * wq::kBudBins;
    if (hist.size() != need) hist.assign(need, 0);
    Out o{std::vector<uint32_t>((size_t)c.n_peers + 1, 0xDEADBEEFu), std::vector<uint32_t>(c.msgs.size(), 0xDEADBEEFu),
          std::vector<uint64_t>(c.n_peers, 0xDEADBEEFull), {}, 0};
    o.dirty = wq_test_peer_budget_bytes_host(c.off.data(), c.msgs.data(), c.n_peers, c.msgs.size(), c.mpos.data(),
                                             c.msize.data(), c.mpos.size() / 3, c.ppos.data(), c.ppos.size() / 3, c.w,
                                             c.with_budget ? c.budget.data() : nullptr, hist.data(), o.oo.data(),
                                             o.om.data(), o.ob.data(), o.cnt);
    for (uint64_t b : hist) o.dirty += b != 0;
    return o;
}

// The contract for ascending offsets, restated with a sort per row and a running sum.
int check_exact(const Case& c, const Out& o) {
    const size_t n_in = c.msgs.size(), n_msgs = c.mpos.size() / 3, n_ppos = c.ppos.size() / 3;
    int bad = o.oo[0] != 0;
    uint32_t at = 0;
    uint64_t kept_bytes = 0;
    for (uint32_t p = 0; p < c.n_peers; ++p) {
        const size_t a = std::min<size_t>(c.off[p], n_in), b = std::max(a, std::min<size_t>(c.off[p + 1], n_in));
        const uint64_t W = c.with_budget ? c.budget[p] : c.w;
        std::vector<std::pair<double, size_t>> e;
        for (size_t j = a; j < b; ++j) {
            double d2 = INFINITY;
            const uint32_t m = c.msgs[j];
            if (m < n_msgs && p < n_ppos) {
                const double dx = c.mpos[3 * m] - c.ppos[3 * p], dy = c.mpos[3 * m + 1] - c.ppos[3 * p + 1],
                             dz = c.mpos[3 * m + 2] - c.ppos[3 * p + 2];
                d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 != d2) d2 = INFINITY;
            }
            e.push_back({d2, j});
        }
        std::sort(e.begin(), e.end());
        std::vector<size_t> keep;
        unsigned __int128 running = 0;
        uint64_t row_bytes = 0;
        for (auto& x : e) {
            const uint32_t m = c.msgs[x.second];
            const uint64_t s = m < n_msgs ? c.msize[m] : 0;
            running += s;
            if (running <= W) keep.push_back(x.second), row_bytes += s;
        }
        std::sort(keep.begin(), keep.end());
        for (size_t j : keep) bad += at >= n_in || o.om[at++] != c.msgs[j];
        bad += o.oo[p + 1] != at;
        bad += o.ob[p] != row_bytes;
        kept_bytes += row_bytes;
    }
    return bad + (o.cnt[1] != at) + (o.cnt[3] != kept_bytes);
}

// The clauses that hold whatever the offsets are.
int check_formed(const Case& c, const Out& o) {
    const size_t n_in = c.msgs.size();
    int bad = o.oo[0] != 0 || o.oo[c.n_peers] > n_in || o.cnt[1] != o.oo[c.n_peers] || o.cnt[0] > n_in;
    bad += o.dirty != 0;
    bad += o.cnt[3] > o.cnt[2];
    uint64_t total = 0;
    for (uint32_t p = 0; p < c.n_peers; ++p) {
        bad += o.oo[p + 1] < o.oo[p];
        bad += o.ob[p] > (c.with_budget ? c.budget[p] : c.w);
        total += o.ob[p];
    }
    bad += total != o.cnt[3];
    for (size_t i = o.oo[c.n_peers]; i < n_in; ++i) bad += o.om[i] != 0xDEADBEEFu;
    return bad;
}

}  // namespace

int main() {
    std::mt19937_64 rng(12);
    const uint32_t lens[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 258, 511, 513, 3000};
    const uint64_t ws[] = {0, 1, 99, 150, 1000, 5000, 40000, 0xFFFFFFFFull, 0x500000000ull, 0xFFFFFFFFFFFFFFFFull};
    int bad = 0, runs = 0;
    std::vector<uint64_t> hist;
    for (int round = 0; round < 80; ++round) {
        Case c;
        c.n_peers = round % 10 == 0 ? 0 : 1 + rng() % 60;
        const size_t n_msgs = round % 7 == 3 ? 0 : 1 + rng() % 500;
        const size_t n_ppos = round % 5 == 4 ? c.n_peers / 2 : c.n_peers;
        const int grid = 1 + rng() % 6;  // few distinct coordinates: many equal keys
        for (size_t i = 0; i < 3 * n_msgs; ++i) c.mpos.push_back((double)(rng() % grid) * 0.37);
        for (size_t i = 0; i < 3 * n_ppos; ++i) c.ppos.push_back((double)(rng() % grid) * 0.37);
        if (n_msgs > 3) c.mpos[4] = NAN, c.mpos[9] = 1e200;
        for (size_t i = 0; i < n_msgs; ++i) {
            const uint64_t r = rng() % 100;
            c.msize.push_back(r < 15 ? 0u : r < 20 ? 0xFFFFFFFFu : r < 25 ? (uint32_t)(2048 + rng() % 14000)
                                                                         : (uint32_t)(100 + rng() % 101));
        }
        c.off.push_back(0);
        for (uint32_t p = 0; p < c.n_peers; ++p) {
            const uint32_t n = lens[rng() % 16];
            for (uint32_t i = 0; i < n; ++i)
                c.msgs.push_back(rng() % 50 == 0 ? 0xFFFFFFFFu - (uint32_t)(rng() % 2) : (uint32_t)(rng() % (n_msgs + 2)));
            c.off.push_back((uint32_t)c.msgs.size());
        }
        for (uint32_t p = 0; p < c.n_peers; ++p) c.budget.push_back(ws[rng() % 10]);
        c.w = ws[rng() % 10];
        const uint32_t full = (uint32_t)c.msgs.size();
        for (int with_budget = 0; with_budget < 2; ++with_budget) {
            c.with_budget = with_budget;
            Case cut = c;
            cut.msgs.resize(full ? rng() % full : 0);
            for (const Case* pc : {&c, &cut}) {
                const Out o = run(*pc, hist);
                bad += check_exact(*pc, o) + check_formed(*pc, o);
                runs++;
            }
            if (c.n_peers < 2) continue;
            std::vector<std::vector<uint32_t>> hostile;
            std::vector<uint32_t> o = c.off;
            std::reverse(o.begin(), o.end());
            hostile.push_back(o);
            o = c.off;
            o[1 + rng() % (c.n_peers - 1)] = full ? (uint32_t)(rng() % full) : 0u;
            hostile.push_back(o);
            hostile.push_back(std::vector<uint32_t>(c.n_peers + 1, 0xFFFFFFFFu));
            o.assign(c.n_peers + 1, 0u);
            for (uint32_t p = 0; p < c.n_peers; ++p) o[p + 1] = o[p] + (uint32_t)(rng() % 400000000);  // wraps
            hostile.push_back(o);
            for (auto& x : o) x = (uint32_t)rng() % (2 * full + 2);
            hostile.push_back(o);
            for (const auto& ho : hostile) {
                Case hc = c;
                hc.off = ho;
                const Out r1 = run(hc, hist), r2 = run(hc, hist);
                bad += check_formed(hc, r1);
                bad += r1.oo != r2.oo || r1.om != r2.om || r1.ob != r2.ob;
                runs++;
            }
        }
    }
    printf("peer_budget_bytes host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
