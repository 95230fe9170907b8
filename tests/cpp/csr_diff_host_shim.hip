// Test-only shim: runs the interest diff's arithmetic (csrc/csr_diff_ops.hpp: clamped row bounds,
// the row of an ordinal, the membership search, the output offset of a row) on the CPU in the shape
// the kernels use it — clamped lengths per row, their saturating prefix, a flag word and a count per
// granule of 64 ordinals, the counts' prefix, then every kept element placed from its granule's
// prefix and every row's offset derived from the same prefix — so the result is checked byte for
// byte against worldql_server_amd/interest.py without a GPU (tests/test_csr_diff_cpp_mirror.py).
// The GPU instance is checked in tests/test_gpu_csr_diff.py.
//
// With -DWQ_CSR_DIFF_SHIM_MAIN the file is a program of its own: random and hostile inputs against
// std::set_difference on the clamped rows, for a host build under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../worldql_server_amd/csrc/csr_diff_ops.hpp"

namespace {

using wq::DiffPair;
using wq::DiffSide;
using wq::kDiffGranule;

// One side's flag pass, as k_diff_flag's flag_side: every granule of the nG the prefix covers.
void flag_side(const DiffSide& src, const DiffSide& oth, const uint32_t* pre, int side, uint32_t M, uint32_t T,
               uint32_t nG, uint64_t* flags, uint32_t* cnt) {
    for (uint32_t g = 0; g < nG; ++g) {
        const uint64_t q0 = (uint64_t)g * kDiffGranule;
        uint64_t word = 0;
        if (q0 < T) {
            const uint32_t last = T - (uint32_t)q0 > kDiffGranule ? (uint32_t)q0 + kDiffGranule - 1 : T - 1;
            const uint32_t rlo = wq::diff_row_of(pre, side, 0, M - 1, (uint32_t)q0);
            const uint32_t rhi = wq::diff_row_of(pre, side, 0, M - 1, last);
            for (uint32_t lane = 0; lane < kDiffGranule; ++lane) {
                const uint32_t q = (uint32_t)q0 + lane;
                if (q < T && wq::diff_keeps(src, oth, pre, side, rlo, rhi, q)) word |= 1ull << lane;
            }
            flags[g] = word;
        }
        cnt[2ull * g + side] = (uint32_t)__builtin_popcountll(word);
    }
}

void emit_side(const DiffSide& src, const uint32_t* pre, int side, uint32_t M, uint32_t T, const uint64_t* flags,
               const uint32_t* base, uint32_t* out, uint32_t out_cap) {
    const uint32_t nGs = T / kDiffGranule + (T % kDiffGranule ? 1u : 0u);
    for (uint32_t g = 0; g < nGs; ++g) {
        const uint64_t word = flags[g];
        if (!word) continue;
        const uint32_t q0 = g * kDiffGranule;
        const uint32_t last = T - q0 > kDiffGranule ? q0 + kDiffGranule - 1 : T - 1;
        const uint32_t rlo = wq::diff_row_of(pre, side, 0, M - 1, q0);
        const uint32_t rhi = wq::diff_row_of(pre, side, 0, M - 1, last);
        for (uint32_t lane = 0; lane < kDiffGranule; ++lane) {
            if (!((word >> lane) & 1ull)) continue;
            uint32_t m;
            bool ok;
            const uint32_t j = wq::diff_source(src, pre, side, rlo, rhi, q0 + lane, &m, &ok);
            const uint32_t pos = base[2ull * g + side] + (uint32_t)__builtin_popcountll(word & ((1ull << lane) - 1ull));
            if (ok && pos < out_cap) out[pos] = src.peers[j];
        }
    }
}

void prefix(const std::vector<DiffPair>& in, std::vector<DiffPair>& out) {
    DiffPair run{0, 0};
    const wq::DiffSatAdd add;
    for (size_t i = 0; i < in.size(); ++i) {
        out[i] = run;
        run = add(run, in[i]);
    }
}

}  // namespace

// counters: {n_entered, n_left, overflow, error}. left_off == NULL: the left side is off.
extern "C" void wq_test_csr_diff_host(size_t n_rows, const uint32_t* old_off, const uint32_t* old_peers,
                                      size_t old_cap, const uint32_t* new_off, const uint32_t* new_peers,
                                      size_t new_cap, uint32_t* ent_off, uint32_t* ent_peers, size_t ent_cap,
                                      uint32_t* left_off, uint32_t* left_peers, size_t left_cap, uint64_t* counters) {
    const uint32_t M = (uint32_t)n_rows;
    const DiffSide nw{new_off, new_peers, (uint32_t)new_cap};
    const DiffSide od{old_off, old_peers, (uint32_t)old_cap};
    const uint32_t lim_n = wq::diff_limit(new_cap), lim_o = left_off ? wq::diff_limit(old_cap) : 0u;
    const uint32_t gn = lim_n / kDiffGranule, go = lim_o / kDiffGranule, nG = std::max(gn, go) + 1;
    std::vector<DiffPair> len(M + 1), pre(M + 1), cnt(nG), base(nG);
    std::vector<uint64_t> flags_e(gn + 1), flags_l(go + 1);
    uint32_t err = 0;
    for (uint32_t m = 0; m < M; ++m) {
        uint32_t a, b, c, d;
        const bool ok_n = wq::diff_row_bounds(nw.off, m, nw.cap, a, b);
        const bool ok_o = wq::diff_row_bounds(od.off, m, od.cap, c, d);
        len[m] = DiffPair{b - a, d - c};
        if (!(ok_n && ok_o)) err |= wq::kDiffErrRows;
    }
    len[M] = DiffPair{0, 0};
    prefix(len, pre);
    const uint32_t* prew = reinterpret_cast<const uint32_t*>(pre.data());
    const uint32_t tn = std::min(pre[M].n, lim_n), to = std::min(pre[M].o, lim_o);
    uint32_t* cntw = reinterpret_cast<uint32_t*>(cnt.data());
    flag_side(nw, od, prew, 0, M, tn, nG, flags_e.data(), cntw);
    flag_side(od, nw, prew, 1, M, to, nG, flags_l.data(), cntw);
    prefix(cnt, base);
    const uint32_t* basew = reinterpret_cast<const uint32_t*>(base.data());
    emit_side(nw, prew, 0, M, tn, flags_e.data(), basew, ent_peers, (uint32_t)ent_cap);
    if (left_off) emit_side(od, prew, 1, M, to, flags_l.data(), basew, left_peers, (uint32_t)left_cap);
    uint32_t e = 0, l = 0;
    for (uint32_t i = 0; i <= M; ++i) {
        e = wq::diff_kept_before(basew, flags_e.data(), 0, std::min(pre[i].n, tn));
        ent_off[i] = e;
        if (left_off) {
            l = wq::diff_kept_before(basew, flags_l.data(), 1, std::min(pre[i].o, to));
            left_off[i] = l;
        }
    }
    counters[0] = e;
    counters[1] = l;
    counters[2] = (e > ent_cap ? 1u : 0u) | (l > left_cap ? 2u : 0u);
    counters[3] = err;
}

#ifdef WQ_CSR_DIFF_SHIM_MAIN
#include <stdio.h>

#include <random>

namespace {

// The clamped rows of a side, as plain vectors (diff_row_bounds per row; the inputs here never reach
// diff_limit, which takes several descending pairs).
std::vector<std::vector<uint32_t>> rows_of(const std::vector<uint32_t>& off, const std::vector<uint32_t>& peers,
                                           uint32_t cap) {
    std::vector<std::vector<uint32_t>> rows(off.size() - 1);
    for (size_t m = 0; m + 1 < off.size(); ++m) {
        uint32_t a, b;
        (void)wq::diff_row_bounds(off.data(), (uint32_t)m, cap, a, b);
        rows[m].assign(peers.begin() + a, peers.begin() + b);
    }
    return rows;
}

int check(const std::vector<uint32_t>& oo, const std::vector<uint32_t>& op, const std::vector<uint32_t>& no,
          const std::vector<uint32_t>& np, bool want_err) {
    const size_t M = oo.size() - 1;
    // exactly sized buffers: the address sanitizer sees any read or write past a capacity
    std::vector<uint32_t> eo(M + 1), lo(M + 1), ep(np.size()), lp(op.size());
    uint64_t c[4];
    wq_test_csr_diff_host(M, oo.data(), op.data(), op.size(), no.data(), np.data(), np.size(), eo.data(), ep.data(),
                          ep.size(), lo.data(), lp.data(), lp.size(), c);
    const auto ro = rows_of(oo, op, (uint32_t)op.size()), rn = rows_of(no, np, (uint32_t)np.size());
    std::vector<uint32_t> we, wl, weo{0}, wlo{0};
    for (size_t m = 0; m < M; ++m) {
        std::set_difference(rn[m].begin(), rn[m].end(), ro[m].begin(), ro[m].end(), std::back_inserter(we));
        std::set_difference(ro[m].begin(), ro[m].end(), rn[m].begin(), rn[m].end(), std::back_inserter(wl));
        weo.push_back((uint32_t)we.size());
        wlo.push_back((uint32_t)wl.size());
    }
    int bad = 0;
    bad += eo != weo || lo != wlo;
    bad += c[0] != we.size() || c[1] != wl.size();
    if (we.size() <= ep.size()) bad += !std::equal(we.begin(), we.end(), ep.begin());
    if (wl.size() <= lp.size()) bad += !std::equal(wl.begin(), wl.end(), lp.begin());
    bad += (c[3] != 0) != want_err;
    return bad;
}

}  // namespace

int main() {
    std::mt19937_64 rng(7);
    const uint32_t lens[] = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 5000};
    int bad = 0, runs = 0;
    for (int round = 0; round < 40; ++round) {
        const size_t M = round == 0 ? 0 : 1 + rng() % 300;
        // odd rounds: each side's peers ascend across the whole array, so rows cut anywhere (the
        // hostile offsets below) are still ascending and distinct
        const bool global = round % 2 == 1;
        std::vector<uint32_t> off[2]{{0}, {0}}, peers[2];
        uint32_t run[2] = {0, 0};
        for (size_t m = 0; m < M; ++m)
            for (int s = 0; s < 2; ++s) {
                const uint32_t n = lens[rng() % (round % 8 == 1 ? 11 : 10)];
                std::vector<uint32_t> row;
                uint32_t v = global ? run[s] : (uint32_t)(rng() % 4);
                for (uint32_t i = 0; i < n; ++i, v += 1 + (uint32_t)(rng() % 3)) row.push_back(v);
                run[s] = v;
                if (!global && n && rng() % 16 == 0) row.back() = 0xFFFFFFFFu;
                peers[s].insert(peers[s].end(), row.begin(), row.end());
                off[s].push_back((uint32_t)peers[s].size());
            }
        bad += check(off[0], peers[0], off[1], peers[1], false);
        runs++;
        if (!global || M < 3 || peers[1].size() < 8) continue;
        // a truncated tick: the peers array ends before offsets[n_rows]
        std::vector<uint32_t> cut(peers[1].begin(), peers[1].begin() + peers[1].size() / 2);
        bad += check(off[0], peers[0], off[1], cut, true);
        // one descending pair, and offsets far past the capacity
        std::vector<uint32_t> o2 = off[1];
        const size_t k = 1 + rng() % (M - 1);
        if (o2[k] > 0) {
            o2[k] = (uint32_t)(rng() % o2[k]);
            bad += check(off[0], peers[0], o2, peers[1], o2[k] < o2[k - 1] || o2[k + 1] < o2[k]);
        }
        o2 = off[1];
        o2[M] = 0xFFFFFFFFu;
        bad += check(off[0], peers[0], o2, peers[1], true);
        runs += 3;
    }
    printf("csr_diff host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
