// Test-only shim: runs the fair share's arithmetic (csrc/rotate_ops.hpp: the occurrence rule, the
// bounds in the kept row, the folded scan terms of a row, the cyclic rank, the running bytes, the
// chosen predicate and the error rules) on the CPU in the passes the kernels of csrc/wq_rotate.hip use
// — rows of both CSRs, saturating scans, the cursor's upper bound, cut flags per granule, the u32 and
// u64 scans, the rows' terms, keep flags, offsets, emit with the cursor — so the result is checked
// byte for byte against worldql_server_amd/interest.py (peer_rotate_np) without a GPU
// (tests/test_peer_rotate_cpp_mirror.py). The GPU instance is checked in tests/test_gpu_peer_rotate.py.
//
// With -DWQ_ROTATE_SHIM_MAIN the file is a program of its own: the case families of
// tests/test_peer_rotate_host.py, random and hostile inputs on exactly sized heap arrays, for a host
// build under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../worldql_server_amd/csrc/rotate_ops.hpp"

extern "C" uint32_t wq_test_rotate_granule() { return wq::kRotGranule; }
extern "C" uint32_t wq_test_rotate_tile() { return wq::kRotTile; }

// As wq_peer_rotate_device (with_sizes: d_msg_size is given, whatever n_msgs is): counters = {n_in,
// n_kept_in, n_chosen, n_out, bytes_chosen, bytes_out, rows_rotated, rows_behind, error}.
extern "C" void wq_test_peer_rotate_host(const uint32_t* off, const uint32_t* msgs, uint32_t n_peers, size_t n_in_,
                                         const uint32_t* koff, const uint32_t* kmsgs, size_t n_kin_,
                                         const uint32_t* msize, size_t n_msgs_, int with_sizes, uint32_t r,
                                         const uint32_t* extra, uint64_t v, const uint64_t* extra_bytes,
                                         uint32_t* cursor, uint32_t* out_off, uint32_t* out_msgs, uint64_t* out_bytes,
                                         uint64_t* counters) {
    using namespace wq;
    const uint32_t n_in = (uint32_t)n_in_, n_kin = (uint32_t)n_kin_;
    const uint32_t n_msgs = (uint32_t)std::min<size_t>(n_msgs_, 0xFFFFFFFFull);
    const size_t rows = (size_t)n_peers + 1;
    uint32_t error = 0, rows_rotated = 0, rows_behind = 0;
    uint64_t bytes_chosen = 0;
    // rows: lengths, saturating prefixes and ordinal spaces of both CSRs; P from the cursor
    std::vector<uint32_t> len(rows, 0), sum(rows, 0), pre(rows, 0), klen(rows, 0), ksum(rows, 0), kpre(rows, 0);
    for (uint32_t p = 0; p < n_peers; ++p) {
        bool ok, kok;
        len[p] = bud_len(off, p, n_in, &ok);
        klen[p] = bud_len(koff, p, n_kin, &kok);
        if (!ok || !kok) error |= kRotErrRows;
    }
    for (size_t p = 1; p < rows; ++p) {
        sum[p] = BudSatAdd()(sum[p - 1], len[p - 1]);
        ksum[p] = BudSatAdd()(ksum[p - 1], klen[p - 1]);
    }
    for (size_t p = 0; p < rows; ++p) {
        pre[p] = std::min(sum[p], n_in);
        kpre[p] = std::min(ksum[p], n_kin);
    }
    std::vector<RotRow> rrow(n_peers);
    for (uint32_t p = 0; p < n_peers; ++p) {
        if (pre[p + 1] - pre[p] != len[p] || kpre[p + 1] - kpre[p] != klen[p]) error |= kRotErrRows;
        rrow[p].P = pre[p] + rot_upper(msgs + bud_row_start(off, p, n_in), pre[p + 1] - pre[p], cursor[p]);
    }
    const uint32_t T = pre[n_peers];
    // cut flags: a word and a prefix per granule of 64 ordinals
    const uint32_t nG = n_in / kRotGranule + 1;
    std::vector<uint64_t> words(2 * (size_t)nG, 0);
    std::vector<uint32_t> base(2 * (size_t)nG, 0);
    auto scan = [&](int side) {
        uint32_t at = 0;
        for (uint32_t g = 0; g < nG; ++g) {
            base[(size_t)side * nG + g] = at;
            at += (uint32_t)__builtin_popcountll(words[(size_t)side * nG + g]);
        }
    };
    std::vector<uint32_t> row(T), size(with_sizes ? T : 0);
    for (uint32_t x = 0; x < T; ++x) {
        const uint32_t p = bud_row_of(pre.data(), n_peers, x);
        const uint32_t i = x - pre[p];
        const uint32_t* full = msgs + bud_row_start(off, p, n_in);
        const uint32_t m = full[i];
        const uint32_t* krow = kmsgs + bud_row_start(koff, p, n_kin);
        if (rot_is_cut(krow, kpre[p + 1] - kpre[p], m, rot_occurrence(full, i))) words[x >> 6] |= 1ull << (x & 63);
        row[x] = p;
        if (with_sizes) {
            size[x] = bud_size(msize, n_msgs, m);
            if (m >= n_msgs) error |= kRotErrMsg;
        }
    }
    scan(0);
    std::vector<uint64_t> bscan((size_t)n_in + 1, 0);
    auto scan_bytes = [&](const uint64_t* w) {
        uint64_t at = 0;
        for (uint64_t q = 0; q <= n_in; ++q) {
            bscan[q] = at;
            at += bud_byte_term(size.data(), w, T, q);
        }
    };
    if (with_sizes) scan_bytes(words.data());
    // the rows' terms
    for (uint32_t p = 0; p < n_peers; ++p) {
        const uint32_t s = pre[p], e = pre[p + 1], P = rrow[p].P;
        const uint32_t Cs = bud_before(base.data(), words.data(), s), CP = bud_before(base.data(), words.data(), P),
                       Ce = bud_before(base.data(), words.data(), e);
        rrow[p] = with_sizes ? rot_row(P, Cs, CP, Ce, bscan[s], bscan[P], bscan[e]) : rot_row(P, Cs, CP, Ce, 0, 0, 0);
    }
    // keep flags
    for (uint32_t x = 0; x < T; ++x) {
        bool f = true;
        if ((words[x >> 6] >> (x & 63)) & 1ull) {
            const uint32_t p = row[x];
            const uint32_t rank = rot_rank(rrow[p], x, bud_before(base.data(), words.data(), x));
            const uint32_t sz = with_sizes ? size[x] : 0u;
            const uint64_t bytes = with_sizes ? rot_bytes(rrow[p], x, bscan[x], sz) : 0ull;
            f = rot_chosen(rank, bytes, rot_share(extra, r, p), with_sizes != 0, rot_share_bytes(extra_bytes, v, p));
            if (f) bytes_chosen += sz;
        }
        if (f) words[(size_t)nG + (x >> 6)] |= 1ull << (x & 63);
    }
    scan(1);
    if (with_sizes) scan_bytes(words.data() + nG);
    // offsets, chosen counts, the per-row counters
    std::vector<uint32_t> n_chosen(rows, 0);
    for (size_t p = 0; p < rows; ++p) {
        const uint32_t s = pre[p];
        const uint32_t o = bud_before(base.data() + nG, words.data() + nG, s);
        out_off[p] = o;
        if (p == n_peers) break;
        const uint32_t e = pre[p + 1];
        const uint32_t n = rot_n_chosen(bud_before(base.data() + nG, words.data() + nG, e) - o, e - s, rrow[p].n_cut);
        n_chosen[p] = n;
        rows_rotated += n > 0;
        rows_behind += n < rrow[p].n_cut;
        if (out_bytes) out_bytes[p] = bscan[e] - bscan[s];
    }
    if (counters) {
        counters[0] = T;
        counters[1] = T - bud_before(base.data(), words.data(), T);
        counters[3] = out_off[n_peers];
        counters[2] = counters[3] - counters[1];
        counters[4] = bytes_chosen;
        counters[5] = with_sizes ? bscan[T] : 0;
        counters[6] = rows_rotated;
        counters[7] = rows_behind;
        counters[8] = error | rot_kept_error(counters[1], kpre[n_peers]);
    }
    // emit, and the cursor
    for (uint32_t x = 0; x < T; ++x) {
        if (!((words[(size_t)nG + (x >> 6)] >> (x & 63)) & 1ull)) continue;
        const uint32_t p = row[x];
        const uint32_t m = msgs[bud_row_start(off, p, n_in) + (x - pre[p])];
        const uint32_t pos = bud_before(base.data() + nG, words.data() + nG, x);
        if (pos < n_in) out_msgs[pos] = m;
        if ((words[x >> 6] >> (x & 63)) & 1ull) {
            const uint32_t rank = rot_rank(rrow[p], x, bud_before(base.data(), words.data(), x));
            if (rank + 1 == n_chosen[p]) cursor[p] = m;
        }
    }
}

#ifdef WQ_ROTATE_SHIM_MAIN
#include <stdio.h>

#include <random>

namespace {

struct Case {
    std::vector<uint32_t> off, msgs, koff, kmsgs, msize, extra, cursor;
    std::vector<uint64_t> extra_bytes;
    uint32_t n_peers, r;
    uint64_t v;
    bool with_sizes, with_extra, with_extra_bytes;
};

struct Out {
    std::vector<uint32_t> oo, om, cursor;
    std::vector<uint64_t> ob;
    uint64_t cnt[9];
};

// Exactly sized heap arrays (an empty vector's data() is never dereferenced): the address sanitizer
// sees any read or write past an array.
Out run(const Case& c) {
    Out o{std::vector<uint32_t>((size_t)c.n_peers + 1, 0xDEADBEEFu), std::vector<uint32_t>(c.msgs.size(), 0xDEADBEEFu),
          c.cursor, std::vector<uint64_t>(c.with_sizes ? c.n_peers : 0, 0xDEADBEEFull), {}};
    wq_test_peer_rotate_host(c.off.data(), c.msgs.data(), c.n_peers, c.msgs.size(), c.koff.data(), c.kmsgs.data(),
                             c.kmsgs.size(), c.msize.data(), c.msize.size(), c.with_sizes, c.r,
                             c.with_extra ? c.extra.data() : nullptr, c.v,
                             c.with_extra_bytes ? c.extra_bytes.data() : nullptr, o.cursor.data(), o.oo.data(),
                             o.om.data(), c.with_sizes ? o.ob.data() : nullptr, o.cnt);
    return o;
}

// The contract for ascending offsets and rows, restated: a merge per row, a rotated list of the cut.
int check_exact(const Case& c, const Out& o) {
    int bad = o.oo[0] != 0;
    uint32_t at = 0;
    for (uint32_t p = 0; p < c.n_peers; ++p) {
        const size_t a = c.off[p], b = c.off[p + 1], ka = c.koff[p], kb = c.koff[p + 1];
        std::vector<size_t> cut;
        size_t j = ka;
        for (size_t i = a; i < b; ++i) {
            while (j < kb && c.kmsgs[j] < c.msgs[i]) ++j;
            if (j < kb && c.kmsgs[j] == c.msgs[i])
                ++j;
            else
                cut.push_back(i);
        }
        size_t lead = 0;
        for (size_t i : cut) lead += c.msgs[i] <= c.cursor[p];
        std::rotate(cut.begin(), cut.begin() + lead, cut.end());
        const uint64_t R = c.with_extra ? c.extra[p] : c.r, V = c.with_extra_bytes ? c.extra_bytes[p] : c.v;
        std::vector<size_t> take;
        uint64_t running = 0;
        for (size_t q = 0; q < cut.size() && q < R; ++q) {
            const uint32_t m = c.msgs[cut[q]];
            running += c.with_sizes && m < c.msize.size() ? c.msize[m] : 0;
            if (c.with_sizes && q > 0 && running > V) break;
            take.push_back(cut[q]);
        }
        bad += o.cursor[p] != (take.empty() ? c.cursor[p] : c.msgs[take.back()]);
        std::vector<bool> gone(b - a, false);
        for (size_t i : cut) gone[i - a] = true;
        for (size_t i : take) gone[i - a] = false;
        uint64_t bytes = 0;
        for (size_t i = a; i < b; ++i) {
            if (gone[i - a]) continue;
            bad += at >= c.msgs.size() || o.om[at++] != c.msgs[i];
            bytes += c.with_sizes && c.msgs[i] < c.msize.size() ? c.msize[c.msgs[i]] : 0;
        }
        bad += o.oo[p + 1] != at;
        if (c.with_sizes) bad += o.ob[p] != bytes;
    }
    return bad + (o.cnt[3] != at);
}

// The clauses that hold whatever the arrays hold.
int check_formed(const Case& c, const Out& o) {
    const size_t n_in = c.msgs.size();
    int bad = o.oo[0] != 0 || o.oo[c.n_peers] > n_in || o.cnt[3] != o.oo[c.n_peers] || o.cnt[0] > n_in;
    for (uint32_t p = 0; p < c.n_peers; ++p) bad += o.oo[p + 1] < o.oo[p];
    for (size_t i = o.oo[c.n_peers]; i < n_in; ++i) bad += o.om[i] != 0xDEADBEEFu;
    return bad;
}

}  // namespace

int main() {
    std::mt19937_64 rng(29);
    const uint32_t lens[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 5, 70, 31, 33, 511, 513, 5000};
    const uint32_t rs[] = {0, 1, 2, 3, 8, 64, 300, 0xFFFFFFFFu};
    int bad = 0, runs = 0;
    for (int round = 0; round < 120; ++round) {
        Case c;
        c.n_peers = round % 10 == 0 ? 0 : 1 + rng() % 40;
        const size_t n_msgs = round % 7 == 3 ? 0 : 1 + rng() % 6000;
        const bool repeats = round % 4 == 1;
        c.off.push_back(0);
        c.koff.push_back(0);
        for (uint32_t p = 0; p < c.n_peers; ++p) {
            const uint32_t n = round == 5 && p == 0 ? 70000u : lens[rng() % 16];
            std::vector<uint32_t> row(n);
            for (auto& m : row)
                m = rng() % 40 == 0 ? 0xFFFFFFFFu - (uint32_t)(rng() % 3) : (uint32_t)(rng() % (repeats ? 9 : n_msgs + 3));
            std::sort(row.begin(), row.end());
            const int mode = (int)(rng() % 5);  // kept: none, all, a third, all but one, a few
            for (uint32_t i = 0; i < n; ++i) {
                const bool keep = mode == 1 || (mode == 2 && rng() % 3 == 0) || (mode == 3 && i != n / 2) ||
                                  (mode == 4 && rng() % 50 == 0);
                if (keep) c.kmsgs.push_back(row[i]);
            }
            c.msgs.insert(c.msgs.end(), row.begin(), row.end());
            c.off.push_back((uint32_t)c.msgs.size());
            c.koff.push_back((uint32_t)c.kmsgs.size());
            // the cursor: anywhere, on an element, the ends
            const int place = (int)(rng() % 5);
            c.cursor.push_back(place == 0   ? 0xFFFFFFFFu
                               : place == 1 ? 0u
                               : place == 2 && n ? row[rng() % n]
                               : place == 3 && n ? row[n - 1]
                                                 : (uint32_t)(rng() % (n_msgs + 5)));
            c.extra.push_back(rs[rng() % 8]);
            c.extra_bytes.push_back(rng() % 3 == 0 ? 0 : rng() % 5000);
        }
        for (size_t i = 0; i < n_msgs; ++i)
            c.msize.push_back(rng() % 9 == 0 ? 0u : round % 11 == 2 ? 0xFFFFFFFFu : (uint32_t)(rng() % 700));
        c.r = rs[rng() % 8];
        c.v = round % 11 == 2 ? 7ull * 0xFFFFFFFFull : rng() % 4000;
        const uint32_t full = (uint32_t)c.msgs.size(), kfull = (uint32_t)c.kmsgs.size();
        for (int variant = 0; variant < 4; ++variant) {
            c.with_sizes = variant & 1;
            c.with_extra = variant >> 1;
            c.with_extra_bytes = c.with_sizes && (round & 1);
            const Out o = run(c);
            bad += check_exact(c, o) + check_formed(c, o);
            runs++;
            if (c.n_peers < 2) continue;
            // hostile offsets in either CSR, arrays cut short, rows that do not ascend
            std::vector<std::vector<uint32_t>> hostile;
            std::vector<uint32_t> h = c.off;
            std::reverse(h.begin(), h.end());
            hostile.push_back(h);
            h = c.off;
            h[1 + rng() % (c.n_peers - 1)] = full ? (uint32_t)(rng() % full) : 0u;
            hostile.push_back(h);
            hostile.push_back(std::vector<uint32_t>(c.n_peers + 1, 0xFFFFFFFFu));
            h.assign(c.n_peers + 1, 0u);
            for (uint32_t p = 0; p < c.n_peers; ++p) h[p + 1] = h[p] + (uint32_t)(rng() % 400000000);  // wraps
            hostile.push_back(h);
            for (auto& x : h) x = (uint32_t)rng() % (2 * full + 2);
            hostile.push_back(h);
            for (const auto& ho : hostile) {
                for (int side = 0; side < 3; ++side) {
                    Case hc = c;
                    if (side != 1) hc.off = ho;
                    if (side != 0) hc.koff = ho;
                    if (side == 2) {
                        hc.msgs.resize(full ? rng() % full : 0);
                        hc.kmsgs.resize(kfull ? rng() % kfull : 0);
                    }
                    const Out r1 = run(hc), r2 = run(hc);
                    bad += check_formed(hc, r1);
                    bad += r1.oo != r2.oo || r1.om != r2.om || r1.cursor != r2.cursor || r1.ob != r2.ob;
                    runs++;
                }
            }
            Case sc = c;
            std::shuffle(sc.msgs.begin(), sc.msgs.end(), rng);
            if (variant & 1) std::shuffle(sc.kmsgs.begin(), sc.kmsgs.end(), rng);
            const Out r1 = run(sc), r2 = run(sc);
            bad += check_formed(sc, r1) + (r1.oo != r2.oo || r1.om != r2.om || r1.cursor != r2.cursor);
            runs++;
        }
    }
    printf("peer_rotate host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
