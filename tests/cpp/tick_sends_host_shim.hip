// Test-only shim: runs the tick sends' arithmetic (csrc/sends_ops.hpp: the host's check of the regions,
// their prefixes, the region and the row that hold an element, its frame, drops and composite key, the
// row check and the per-peer lower bound) on the CPU in the kernels' passes — begin, rows, expand, a stable
// sort by key over the key's bits with u32 or u64 keys, one lower bound per peer — with std::stable_sort
// in place of rocPRIM, so the result is checked byte for byte against worldql_server_amd/interest.py
// (tick_sends_np) without a GPU (tests/test_tick_sends_cpp_mirror.py). The GPU instance is checked in
// tests/test_gpu_tick_sends.py.
//
// With -DWQ_TICK_SENDS_SHIM_MAIN the file is a program of its own: random and hostile layouts on exactly
// sized vectors, for a host build under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../worldql_server_amd/csrc/sends_ops.hpp"

namespace {

template <typename K>
void passes(const wq::SndView& v, uint32_t P, uint32_t* peer_offsets, uint32_t* frames_out, wq_tick_sends_counters* c) {
    std::vector<K> key(P), skey(P);
    std::vector<uint32_t> val(P), order(P);
    for (uint32_t j = 0; j < P; ++j) {
        const int what = wq::snd_elem<K>(v, j, &key[j], &val[j]);
        c->n_covered += what != wq::kSndNone;
        c->n_kept += what == wq::kSndKept;
        c->n_drop_peer += what == wq::kSndDropPeer;
        c->n_drop_frame += what == wq::kSndDropFrame;
        if (what == wq::kSndDropFrame) c->error |= 2u;
    }
    // the radix sort sees the low bits of a key only
    const int bits = wq::pm_key_bits(v.n_peers) + v.frame_bits;
    const K mask = bits >= (int)(8 * sizeof(K)) ? ~(K)0 : (((K)1 << bits) - 1);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return (key[x] & mask) < (key[y] & mask); });
    for (uint32_t i = 0; i < P; ++i) {
        skey[i] = key[order[i]];
        frames_out[i] = val[order[i]];
    }
    for (uint64_t p = 0; p <= v.n_peers; ++p)
        peer_offsets[p] = wq::snd_lower_bound<K>(skey.data(), P, (uint32_t)p, v.frame_bits);
}

}  // namespace

// As wq_tick_sends_device with every array on the host: 0, or 1 where the call is refused (nothing
// written). key_width (out, nullable): 32 or 64, the instantiation that ran (0: no element).
extern "C" int wq_test_tick_sends_host(const wq_tick_sends_in* in, uint32_t* peer_offsets, uint32_t* frames_out,
                                       size_t n_elems, wq_tick_sends_counters* counters, int* key_width) {
    if (!in || !peer_offsets || (n_elems && !frames_out) || wq::snd_check(in, n_elems)) return 1;
    const uint32_t n = in->n_regions, P = (uint32_t)n_elems;
    std::vector<uint32_t> elem_pre((size_t)n + 1);
    std::vector<uint64_t> row_pre((size_t)n + 1);
    wq::snd_prefixes(in->regions, n, elem_pre.data(), row_pre.data());
    wq::SndView v;
    v.reg = in->regions;
    v.elem_pre = elem_pre.data();
    v.row_pre = row_pre.data();
    v.off = in->d_offsets;
    v.peers = in->d_peers;
    v.src[0] = in->d_src[0];
    v.src[1] = in->d_src[1];
    v.connected = in->d_connected;
    v.n_regions = n;
    v.n_peers = in->n_peers;
    v.n_frames = in->n_frames;
    v.frame_bits = wq::snd_frame_bits(in->n_frames);
    wq_tick_sends_counters c{};
    c.n_regions = n;
    c.n_elems = n_elems;
    for (uint64_t i = 0; i < row_pre[n]; ++i)
        if (wq::snd_row_bad(v, i)) c.error |= 1u;
    const bool narrow = wq::pm_key_bits(in->n_peers) + v.frame_bits <= 32;
    if (key_width) *key_width = P == 0 ? 0 : narrow ? 32 : 64;
    if (P == 0)
        for (uint64_t p = 0; p <= in->n_peers; ++p) peer_offsets[p] = 0;
    else if (narrow)
        passes<uint32_t>(v, P, peer_offsets, frames_out, &c);
    else
        passes<uint64_t>(v, P, peer_offsets, frames_out, &c);
    if (counters) *counters = c;
    return 0;
}

#ifdef WQ_TICK_SENDS_SHIM_MAIN
#include <stdio.h>

#include <map>
#include <random>

namespace {

struct Lay {
    std::vector<wq_send_region> reg;
    std::vector<uint32_t> off, peers, src[2], conn;
    uint32_t n_peers = 0, n_frames = 0;
    bool with_conn = false;
};

struct Run {
    int rc;
    std::vector<uint32_t> po, fo;
    wq_tick_sends_counters c;
};

// Exactly sized buffers: the address sanitizer sees any read or write past an array.
Run run(const Lay& l) {
    wq_tick_sends_in in{};
    in.regions = l.reg.data();
    in.n_regions = (uint32_t)l.reg.size();
    in.d_offsets = l.off.data();
    in.n_offsets = l.off.size();
    in.d_peers = l.peers.data();
    in.n_pairs = l.peers.size();
    for (int k = 0; k < 2; ++k) {
        in.d_src[k] = l.src[k].data();
        in.n_src[k] = l.src[k].size();
    }
    in.d_connected = l.with_conn ? l.conn.data() : nullptr;
    in.n_peers = l.n_peers;
    in.n_frames = l.n_frames;
    size_t n_elems = 0;
    for (const auto& g : l.reg) n_elems += g.capacity;
    Run r{0, std::vector<uint32_t>((size_t)l.n_peers + 1, 0xDEADBEEFu), std::vector<uint32_t>(n_elems, 0xDEADBEEFu), {}};
    r.rc = wq_test_tick_sends_host(&in, r.po.data(), r.fo.data(), n_elems, &r.c, nullptr);
    return r;
}

// The contract for ascending offsets, restated with a map: per peer its (frame, element) pairs.
int check_exact(const Lay& l, const Run& r) {
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> want;
    uint64_t ord = 0;
    for (const auto& g : l.reg) {
        for (uint64_t e = 0; e < g.capacity; ++e, ++ord) {
            uint64_t row = g.n_rows;
            if (g.off_at == WQ_SEND_UNIT_ROWS) {
                if (e < g.n_rows) row = e;
            } else {
                for (uint64_t m = 0; m < g.n_rows && row == g.n_rows; ++m) {
                    const uint64_t a = std::min<uint64_t>(l.off[g.off_at + m], g.capacity);
                    const uint64_t b = std::min<uint64_t>(l.off[g.off_at + m + 1], g.capacity);
                    if (a <= e && e < b) row = m;
                }
            }
            if (row == g.n_rows) continue;
            const uint64_t f = (uint64_t)g.frame_base + (g.src_at == WQ_SEND_NO_SRC ? row : l.src[g.src_sel][g.src_at + row]);
            const uint32_t p = l.peers[g.peers_at + e];
            if (f >= l.n_frames || p >= l.n_peers || (l.with_conn && !((l.conn[p >> 5] >> (p & 31)) & 1u))) continue;
            want[p].push_back({f, ord});
        }
    }
    int bad = 0;
    uint32_t at = 0;
    for (uint64_t p = 0; p < l.n_peers; ++p) {
        bad += r.po[p] != at;
        auto it = want.find((uint32_t)p);
        if (it == want.end()) continue;
        std::sort(it->second.begin(), it->second.end());
        for (const auto& fe : it->second) bad += at >= r.fo.size() || r.fo[at++] != fe.first;
    }
    bad += r.po[l.n_peers] != at || r.c.n_kept != at;
    return bad;
}

// The clauses that hold whatever the offsets are.
int check_formed(const Lay& l, const Run& r) {
    const size_t P = r.fo.size();
    int bad = r.rc != 0 || r.po[0] != 0 || r.po[l.n_peers] > P;
    for (uint64_t p = 0; p < l.n_peers; ++p) {
        bad += r.po[p + 1] < r.po[p];
        for (uint32_t i = r.po[p]; i + 1 < std::min<size_t>(r.po[p + 1], P); ++i) bad += r.fo[i + 1] < r.fo[i];
    }
    for (size_t i = 0; i < P; ++i) bad += i < r.po[l.n_peers] ? r.fo[i] >= l.n_frames : r.fo[i] != 0;
    bad += r.c.n_covered != r.c.n_kept + r.c.n_drop_peer + r.c.n_drop_frame || r.c.n_elems != P;
    return bad;
}

}  // namespace

int main() {
    std::mt19937_64 rng(17);
    const uint32_t npeers[] = {0, 1, 2, 31, 32, 33, 300, 65535, 65536, (1u << 20) + 3};
    const uint32_t nframes[] = {0, 1, 2, 9, 400, 65536, 0xFFFFFFFFu};
    int bad = 0, runs = 0;
    for (int round = 0; round < 300; ++round) {
        Lay l;
        l.n_peers = npeers[rng() % 10];
        l.n_frames = nframes[rng() % 7];
        l.conn.resize((l.n_peers + 31) / 32);   // exactly ceil(n_peers / 32) words
        for (auto& w : l.conn) w = (uint32_t)rng();
        const int n_reg = (int)(rng() % 7);
        std::vector<int> csr_regions;
        for (int k = 0; k < n_reg; ++k) {
            wq_send_region g{};
            g.n_rows = (uint32_t)(rng() % 9);
            g.src_sel = (uint32_t)(rng() % 2);
            g.frame_base = rng() % 4 == 0 ? (uint32_t)(rng() % 3) : 0u;
            g.peers_at = (uint32_t)l.peers.size();
            uint32_t pairs = 0;
            if (rng() % 4 == 0) {
                g.off_at = WQ_SEND_UNIT_ROWS;
                pairs = g.n_rows;
            } else {
                g.off_at = (uint32_t)l.off.size();
                l.off.push_back(0);
                for (uint32_t m = 0; m < g.n_rows; ++m) l.off.push_back(pairs += (uint32_t)(rng() % 5));
                csr_regions.push_back(k);
            }
            const uint32_t caps[] = {pairs, pairs, pairs ? (uint32_t)(rng() % pairs) : 0u, pairs + 7, 0};
            g.capacity = caps[rng() % 5];
            for (uint32_t e = 0; e < g.capacity; ++e)
                l.peers.push_back(rng() % 16 == 0 ? 0xFFFFFFFFu : (uint32_t)(rng() % ((uint64_t)l.n_peers + 3)));
            if (rng() % 5 == 0) {
                g.src_at = WQ_SEND_NO_SRC;
            } else {
                g.src_at = (uint32_t)l.src[g.src_sel].size();
                for (uint32_t m = 0; m < g.n_rows; ++m)
                    l.src[g.src_sel].push_back(rng() % 16 == 0 ? 0xFFFFFFFFu : (uint32_t)(rng() % ((uint64_t)l.n_frames + 2)));
            }
            l.reg.push_back(g);
        }
        for (int with_conn = 0; with_conn < 2; ++with_conn) {
            l.with_conn = with_conn;
            const Run r = run(l);
            bad += check_exact(l, r) + check_formed(l, r);
            runs++;
            // hostile offsets in one region: reversed, all 2^32 - 1, junk
            for (int k : csr_regions) {
                const wq_send_region& g = l.reg[k];
                if (g.n_rows < 2) continue;
                for (int kind = 0; kind < 3; ++kind) {
                    Lay h = l;
                    auto first = h.off.begin() + g.off_at, last = first + g.n_rows + 1;
                    if (kind == 0) std::reverse(first, last);
                    if (kind == 1) std::fill(first, last, 0xFFFFFFFFu);
                    if (kind == 2) for (auto it = first; it != last; ++it) *it = (uint32_t)(rng() % (2 * g.capacity + 2));
                    const Run r1 = run(h), r2 = run(h);
                    bad += check_formed(h, r1) + (r1.po != r2.po || r1.fo != r2.fo);
                    runs++;
                }
            }
        }
    }
    printf("tick_sends host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
