// Test-only shim: runs the send budgets' arithmetic (csrc/budget_ops.hpp: the clamped lengths and the
// ordinal space, the key with its NaN / missing rule and u64 image, the class of a row, the rank by
// counting, the digit / match / pick tests of the radix select, the keep predicate and the flag-word
// prefix) on the CPU in the passes the kernels of csrc/wq_budget.hip use — rows, saturating scan,
// rows again, keys, eight histogram-and-pick passes, tie flags, keep flags, emit — so the result is
// checked byte for byte against worldql_server_amd/interest.py (peer_budget_np) without a GPU
// (tests/test_peer_budget_cpp_mirror.py). The GPU instance is checked in tests/test_gpu_peer_budget.py.
//
// With -DWQ_PEER_BUDGET_SHIM_MAIN the file is a program of its own: random and hostile inputs on
// exactly sized vectors, for a host build under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../worldql_server_amd/csrc/budget_ops.hpp"

extern "C" uint32_t wq_test_budget_short() { return wq::kBudShort; }
extern "C" uint32_t wq_test_budget_digit_bits() { return (uint32_t)wq::kBudDigitBits; }
extern "C" uint32_t wq_test_budget_tile() { return wq::kBudTile; }
extern "C" uint32_t wq_test_budget_tiles() { return wq::kBudTiles; }

// As wq_peer_budget_device with the positions given: counters = {n_in, n_kept, rows_cut, error}.
extern "C" void wq_test_peer_budget_host(const uint32_t* off, const uint32_t* msgs, uint32_t n_peers, size_t n_in_,
                                         const double* mpos, size_t n_msgs, const double* ppos, size_t n_ppos,
                                         uint32_t k, const uint32_t* budget, uint32_t* out_off, uint32_t* out_msgs,
                                         uint64_t* counters) {
    using namespace wq;
    const uint32_t n_in = (uint32_t)n_in_;
    const size_t rows = (size_t)n_peers + 1;
    uint32_t rows_cut = 0, error = 0;
    // rows: lengths, saturating prefix, the ordinal space, classes and kept counts
    std::vector<uint32_t> len(rows, 0), sum(rows, 0), pre(rows, 0);
    for (uint32_t p = 0; p < n_peers; ++p) {
        bool ok;
        len[p] = bud_len(off, p, n_in, &ok);
        if (!ok) error |= kBudErrRows;
    }
    for (size_t p = 1; p < rows; ++p) sum[p] = BudSatAdd()(sum[p - 1], len[p - 1]);
    for (size_t p = 0; p < rows; ++p) pre[p] = std::min(sum[p], n_in);
    const size_t n_slots = n_in / kBudShort + 1;
    std::vector<BudSel> sel(n_slots, BudSel{0, 0, 0});
    std::vector<uint32_t> hist(n_slots * kBudBins, 0);
    out_off[0] = 0;
    for (uint32_t p = 0; p < n_peers; ++p) {
        const uint32_t n = pre[p + 1] - pre[p];
        if (n != len[p]) error |= kBudErrRows;
        const uint32_t B = bud_budget(budget, k, p);
        const uint8_t c = bud_class(n, B);
        if (c != kBudAll) rows_cut++;
        if (c == kBudLongCut) sel[pre[p] >> kBudShortLog2] = BudSel{0, B, 1};
        out_off[p + 1] = out_off[p] + std::min(n, B);
    }
    const uint32_t T = pre[n_peers];
    // keys
    std::vector<uint64_t> key(T);
    std::vector<uint32_t> row(T);
    std::vector<uint8_t> cls(T);
    for (uint32_t q = 0; q < T; ++q) {
        const uint32_t p = bud_row_of(pre.data(), n_peers, q);
        const uint32_t j = bud_row_start(off, p, n_in) + (q - pre[p]);
        bool bad;
        key[q] = bud_key(mpos, (uint32_t)n_msgs, ppos, (uint32_t)n_ppos, p, msgs[j], &bad);
        row[q] = p;
        cls[q] = bud_class(pre[p + 1] - pre[p], bud_budget(budget, k, p));
        if (bad) error |= kBudErrMsg;
    }
    // select
    for (int pass = 0; pass < kBudPasses; ++pass) {
        const int shift = bud_shift(pass);
        for (uint32_t q = 0; q < T; ++q) {
            if (cls[q] != kBudLongCut) continue;
            const size_t slot = pre[row[q]] >> kBudShortLog2;
            if (bud_matches(key[q], sel[slot].prefix, shift)) hist[slot * kBudBins + bud_digit(key[q], shift)]++;
        }
        for (size_t slot = 0; slot < n_slots; ++slot) {
            if (!sel[slot].active) continue;
            const uint32_t need = sel[slot].need;
            uint32_t below = 0;
            for (uint32_t t = 0; t < kBudBins; ++t) {
                const uint32_t c = hist[slot * kBudBins + t];
                hist[slot * kBudBins + t] = 0;
                if (bud_picks(below, c, need)) {
                    sel[slot].prefix |= (uint64_t)t << shift;
                    sel[slot].need = need - below;
                }
                below += c;
            }
        }
    }
    // tie flags, keep flags: a word, a count and a prefix per granule of 64 ordinals
    const uint32_t nG = n_in / 64 + 1;
    std::vector<uint64_t> words(2 * (size_t)nG, 0);
    std::vector<uint32_t> base(2 * (size_t)nG, 0);
    auto scan = [&](int side) {
        uint32_t at = 0;
        for (uint32_t g = 0; g < nG; ++g) {
            base[(size_t)side * nG + g] = at;
            at += (uint32_t)__builtin_popcountll(words[(size_t)side * nG + g]);
        }
    };
    for (uint32_t q = 0; q < T; ++q)
        if (cls[q] == kBudLongCut && key[q] == sel[pre[row[q]] >> kBudShortLog2].prefix) words[q >> 6] |= 1ull << (q & 63);
    scan(0);
    for (uint32_t q = 0; q < T; ++q) {
        bool f = false;
        const uint32_t p = row[q];
        if (cls[q] == kBudAll) {
            f = true;
        } else if (cls[q] == kBudShortCut) {
            f = bud_short_keeps(key.data(), pre[p], pre[p + 1] - pre[p], q, bud_budget(budget, k, p));
        } else if (cls[q] == kBudLongCut) {
            const BudSel s = sel[pre[p] >> kBudShortLog2];
            uint32_t tie_rank = 0;
            if (key[q] == s.prefix)
                tie_rank = bud_before(base.data(), words.data(), q) - bud_before(base.data(), words.data(), pre[p]);
            f = bud_keeps(key[q], tie_rank, s.prefix, s.need);
        }
        if (f) words[(size_t)nG + (q >> 6)] |= 1ull << (q & 63);
    }
    scan(1);
    // emit
    for (uint32_t q = 0; q < T; ++q) {
        if (!((words[(size_t)nG + (q >> 6)] >> (q & 63)) & 1ull)) continue;
        const uint32_t p = row[q];
        const uint32_t j = bud_row_start(off, p, n_in) + (q - pre[p]);
        const uint32_t pos = bud_before(base.data() + nG, words.data() + nG, q);
        if (pos < n_in) out_msgs[pos] = msgs[j];
    }
    if (counters) {
        counters[0] = T;
        counters[1] = out_off[n_peers];
        counters[2] = rows_cut;
        counters[3] = error;
    }
}

#ifdef WQ_PEER_BUDGET_SHIM_MAIN
#include <math.h>
#include <stdio.h>

#include <random>

namespace {

struct Case {
    std::vector<uint32_t> off, msgs, budget;
    std::vector<double> mpos, ppos;
    uint32_t n_peers, k;
    bool with_budget;
};

struct Out {
    std::vector<uint32_t> oo, om;
    uint64_t cnt[4];
};

// Exactly sized buffers: the address sanitizer sees any read or write past an array.
Out run(const Case& c) {
    Out o{std::vector<uint32_t>((size_t)c.n_peers + 1, 0xDEADBEEFu), std::vector<uint32_t>(c.msgs.size(), 0xDEADBEEFu), {}};
    wq_test_peer_budget_host(c.off.data(), c.msgs.data(), c.n_peers, c.msgs.size(), c.mpos.data(), c.mpos.size() / 3,
                             c.ppos.data(), c.ppos.size() / 3, c.k, c.with_budget ? c.budget.data() : nullptr,
                             o.oo.data(), o.om.data(), o.cnt);
    return o;
}

// The contract for ascending offsets, restated with a sort per row.
int check_exact(const Case& c, const Out& o) {
    const size_t n_in = c.msgs.size(), n_msgs = c.mpos.size() / 3, n_ppos = c.ppos.size() / 3;
    int bad = o.oo[0] != 0;
    uint32_t at = 0;
    for (uint32_t p = 0; p < c.n_peers; ++p) {
        const size_t a = std::min<size_t>(c.off[p], n_in), b = std::max(a, std::min<size_t>(c.off[p + 1], n_in));
        const size_t B = c.with_budget ? c.budget[p] : c.k;
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
        e.resize(std::min(B, e.size()));
        std::vector<size_t> keep;
        for (auto& x : e) keep.push_back(x.second);
        std::sort(keep.begin(), keep.end());
        for (size_t j : keep) bad += at >= n_in || o.om[at++] != c.msgs[j];
        bad += o.oo[p + 1] != at;
    }
    return bad + (o.cnt[1] != at);
}

// The clauses that hold whatever the offsets are.
int check_formed(const Case& c, const Out& o) {
    const size_t n_in = c.msgs.size();
    int bad = o.oo[0] != 0 || o.oo[c.n_peers] > n_in || o.cnt[1] != o.oo[c.n_peers] || o.cnt[0] > n_in;
    for (uint32_t p = 0; p < c.n_peers; ++p) {
        bad += o.oo[p + 1] < o.oo[p];
        const uint64_t B = c.with_budget ? c.budget[p] : c.k;
        bad += (uint64_t)o.oo[p + 1] - o.oo[p] > B;
    }
    for (size_t i = o.oo[c.n_peers]; i < n_in; ++i) bad += o.om[i] != 0xDEADBEEFu;
    return bad;
}

}  // namespace

int main() {
    std::mt19937_64 rng(12);
    const uint32_t lens[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 258, 511, 513, 3000};
    const uint32_t ks[] = {0, 1, 2, 7, 32, 255, 256, 257, 1000, 0xFFFFFFFFu};
    int bad = 0, runs = 0;
    for (int round = 0; round < 80; ++round) {
        Case c;
        c.n_peers = round % 10 == 0 ? 0 : 1 + rng() % 60;
        const size_t n_msgs = round % 7 == 3 ? 0 : 1 + rng() % 500;
        const size_t n_ppos = round % 5 == 4 ? c.n_peers / 2 : c.n_peers;
        const int grid = 1 + rng() % 6;  // few distinct coordinates: many equal keys
        for (size_t i = 0; i < 3 * n_msgs; ++i) c.mpos.push_back((double)(rng() % grid) * 0.37);
        for (size_t i = 0; i < 3 * n_ppos; ++i) c.ppos.push_back((double)(rng() % grid) * 0.37);
        if (n_msgs > 3) c.mpos[4] = NAN, c.mpos[9] = 1e200;
        c.off.push_back(0);
        for (uint32_t p = 0; p < c.n_peers; ++p) {
            const uint32_t n = lens[rng() % 16];
            for (uint32_t i = 0; i < n; ++i)
                c.msgs.push_back(rng() % 50 == 0 ? 0xFFFFFFFFu - (uint32_t)(rng() % 2) : (uint32_t)(rng() % (n_msgs + 2)));
            c.off.push_back((uint32_t)c.msgs.size());
        }
        for (uint32_t p = 0; p < c.n_peers; ++p) c.budget.push_back(ks[rng() % 10]);
        c.k = ks[rng() % 10];
        const uint32_t full = (uint32_t)c.msgs.size();
        for (int with_budget = 0; with_budget < 2; ++with_budget) {
            c.with_budget = with_budget;
            Case cut = c;
            cut.msgs.resize(full ? rng() % full : 0);
            for (const Case* pc : {&c, &cut}) {
                const Out o = run(*pc);
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
                const Out r1 = run(hc), r2 = run(hc);
                bad += check_formed(hc, r1);
                bad += r1.oo != r2.oo || r1.om != r2.om;
                runs++;
            }
        }
    }
    printf("peer_budget host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
