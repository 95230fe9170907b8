// Test-only shim: runs the table export's arithmetic (csrc/export_ops.hpp: live-cube test, cube key
// and sort words, the cube of a row, the row's peer, the 40-byte row, the bitmap test) on the CPU in
// the shape the kernels of csrc/wq_table_export.hip use it — flag per table slot / exclusive scan /
// gather of the live cubes / four stable passes over the cube ids / counts in order and their scan /
// emit per granule of 64 rows / flag, count, scan and compacted emit with a peer filter — over a host
// copy of the record, slot and list layout that the shim builds from a list of cubes. The result is
// checked byte for byte against worldql_server_amd/snapshot.py TableRef.export without a GPU
// (tests/test_snapshot_cpp_mirror.py). The GPU instance is checked in tests/test_gpu_snapshot.py.
//
// With -DWQ_TABLE_EXPORT_SHIM_MAIN the file is a program of its own: a seeded random stream of
// tables and filters against a brute-force model, over exactly sized heap buffers, for a host build
// under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../worldql_server_amd/csrc/export_ops.hpp"

namespace {

using namespace wq;

// The table of wq_device.hpp on the host: packable cubes in open-addressed 128-byte records (a list
// of at most kInline peers lives in the inline words only: its list block holds junk), the rest in
// the full-key slot table; list[off] = count, then the ascending peers, then the block's headroom.
struct HostTable {
    std::vector<Record> recs;
    std::vector<Slot> slots;
    std::vector<uint32_t> list;
    uint64_t live = 0;  // cubes that hold a peer (the handle's n_cubes)
    uint64_t rows = 0;  // entries (the handle's st.n)
};

uint64_t pow2_at_least(uint64_t n) {
    uint64_t c = 8;
    while (c < n) c <<= 1;
    return c;
}

void build(HostTable& t, uint16_t cs, size_t n_cubes, const uint32_t* world, const int64_t* key, const uint32_t* off,
           const uint32_t* peers) {
    t.recs.assign(pow2_at_least(4 * n_cubes), Record{});
    t.slots.resize(pow2_at_least(2 * n_cubes));
    for (Slot& s : t.slots) {
        s = Slot{};
        s.world = kWorldEmpty;
    }
    t.list.assign(1, 0u);  // word 0: the shared empty list
    for (size_t c = 0; c < n_cubes; ++c) {
        const uint32_t n = off[c + 1] - off[c];
        const uint32_t* p = peers + off[c];
        const int64_t* k = key + 3 * c;
        t.live += n ? 1 : 0;
        t.rows += n;
        const uint32_t cap = list_capacity(n), lo = (uint32_t)t.list.size();
        t.list.push_back(n);
        uint64_t pk;
        uint32_t ext;
        const bool packed = pack_key(world[c], k[0], k[1], k[2], (double)cs, &pk, &ext);
        const bool inline_only = packed && n <= (uint32_t)kInline;
        for (uint32_t j = 0; j < cap; ++j) t.list.push_back(j < n && !inline_only ? p[j] : 0xDEADBEEFu);
        if (packed) {
            uint64_t i = rec_hash(pk, ext) & (t.recs.size() - 1);
            while (t.recs[i].ext) i = (i + 1) & (t.recs.size() - 1);
            Record& r = t.recs[i];
            r.pk = pk;
            r.ext = ext;
            r.count = n;
            r.list_off = lo;
            r.cap = cap;
            for (int j = 0; j < kInline; ++j) r.peers[j] = (uint32_t)j < n ? p[j] : kNone;
        } else {
            uint64_t i = cube_hash(world[c], k[0], k[1], k[2]) & (t.slots.size() - 1);
            while (t.slots[i].world != kWorldEmpty) i = (i + 1) & (t.slots.size() - 1);
            Slot& s = t.slots[i];
            s.k[0] = k[0];
            s.k[1] = k[1];
            s.k[2] = k[2];
            s.world = world[c];
            s.off = lo;
        }
    }
}

void exclusive_scan(const std::vector<uint32_t>& in, std::vector<uint32_t>& out) {
    uint32_t run = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        out[i] = run;
        run += in[i];
    }
}

// k_exp_emit<MODE> for granule g: 0 every row, 1 flag + count, 2 the kept rows.
void emit_granule(int mode, const ExpTable& t, const std::vector<uint32_t>& base, const std::vector<uint32_t>& ocnt,
                  const std::vector<uint32_t>& osrc, uint32_t C, uint32_t g, const ExpFilter& f,
                  std::vector<uint64_t>& gword, std::vector<uint32_t>& gcnt, const std::vector<uint32_t>& gbase,
                  uint64_t* out, uint32_t capacity) {
    const uint32_t total = base[C];
    const uint64_t row0 = (uint64_t)g * kExpGranule;
    uint64_t ballot = 0;
    const uint64_t word = mode == 2 ? gword[g] : 0;
    for (uint32_t lane = 0; lane < kExpGranule; ++lane) {
        if (row0 + lane >= total) continue;
        if (mode == 2 && !((word >> lane) & 1ull)) continue;
        const uint32_t row = (uint32_t)row0 + lane;
        const uint32_t c0 = exp_cube_of(base.data(), 0, C - 1, (uint32_t)row0);
        const uint32_t c = exp_cube_in_granule(base.data(), c0, C, row);
        const uint64_t i = osrc[c];
        const uint32_t peer = exp_peer(t, i, ocnt[c], row - base[c]);
        const bool keep = mode == 0 || exp_peer_passes(f, peer);
        if (mode == 1) {
            ballot |= keep ? 1ull << lane : 0ull;
            continue;
        }
        if (!keep) continue;
        uint32_t w;
        int64_t k[3];
        exp_cube_key(t, i, &w, k);
        const uint64_t idx = mode == 0 ? row0 + lane
                                       : (uint64_t)gbase[g] + (uint64_t)__builtin_popcountll(word & ((1ull << lane) - 1ull));
        if (idx < capacity) exp_write_row(out, idx, w, peer, k);
    }
    if (mode == 1) {
        gword[g] = ballot;
        gcnt[g] = (uint32_t)__builtin_popcountll(ballot);
    }
}

// export_one of wq_table_export.hip on the host table. Returns 0, or -5 (WQ_E_CAPACITY).
int export_host(const HostTable& h, uint16_t cs, uint32_t f_world, int by_peer, const uint32_t* f_peers,
                uint32_t f_n_peers, uint64_t* out, size_t capacity, size_t* n) {
    *n = 0;
    if (by_peer && f_n_peers == 0) return 0;
    const uint64_t D = h.recs.size() + h.slots.size();
    if (!h.rows || !h.live) return 0;
    const uint32_t C = (uint32_t)std::min<uint64_t>(h.live, D);
    const uint32_t n_gran = (uint32_t)((h.rows + kExpGranule - 1) / kExpGranule);
    const uint32_t cap32 = (uint32_t)std::min<uint64_t>(capacity, 0xFFFFFFFFull);
    const ExpTable t{h.recs.data(), h.recs.size(), h.slots.data(), h.slots.size(), h.list.data(), (int64_t)cs};
    ExpFilter flt{f_world, 0u, nullptr};
    std::vector<uint32_t> bits;
    if (by_peer) {
        uint32_t top = 0;
        for (uint32_t i = 0; i < f_n_peers; ++i) top = std::max(top, f_peers[i]);
        bits.assign((size_t)top / 32 + 1, 0u);
        for (uint32_t i = 0; i < f_n_peers; ++i) bits[f_peers[i] >> 5] |= 1u << (f_peers[i] & 31u);
        flt.bits = bits.data();
        flt.n_bits = (uint32_t)std::min<uint64_t>((uint64_t)bits.size() * 32, 0xFFFFFFFFull);
    }
    // 1-2: flag, scan, gather
    std::vector<uint32_t> flag(D + 1, 0u), pos(D + 1);
    for (uint64_t i = 0; i < D; ++i) flag[i] = exp_cube_count(t, i, flt.world) ? 1u : 0u;
    exclusive_scan(flag, pos);
    std::vector<uint64_t> keys(4ull * C, ~0ull);
    std::vector<uint32_t> cnt(C, 0u), src(C, 0u);
    for (uint64_t i = 0; i < D; ++i) {
        if (!flag[i] || pos[i] >= C) continue;
        const uint32_t j = pos[i];
        uint32_t w;
        int64_t k[3];
        exp_cube_key(t, i, &w, k);
        keys[j] = w;
        keys[(uint64_t)C + j] = exp_ord(k[0]);
        keys[2ull * C + j] = exp_ord(k[1]);
        keys[3ull * C + j] = exp_ord(k[2]);
        cnt[j] = exp_cube_count(t, i, flt.world);
        src[j] = (uint32_t)i;
    }
    // 3: four stable passes, least significant word first (the world pass over its low 32 bits)
    std::vector<uint32_t> idx(C);
    for (uint32_t c = 0; c < C; ++c) idx[c] = c;
    for (int word = 3; word >= 0; --word) {
        const uint64_t* kw = keys.data() + (uint64_t)word * C;
        const uint64_t mask = word ? ~0ull : 0xFFFFFFFFull;
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return (kw[a] & mask) < (kw[b] & mask); });
    }
    // 4: counts in order, row bases
    std::vector<uint32_t> ocnt((size_t)C + 1, 0u), osrc(C), base((size_t)C + 1);
    for (uint32_t c = 0; c < C; ++c) {
        ocnt[c] = cnt[idx[c]];
        osrc[c] = src[idx[c]];
    }
    exclusive_scan(ocnt, base);
    // 5: the rows
    std::vector<uint64_t> gword;
    std::vector<uint32_t> gcnt, gbase;
    if (!by_peer) {
        const uint32_t gr = (uint32_t)((std::min<uint64_t>(cap32, h.rows) + kExpGranule - 1) / kExpGranule);
        for (uint32_t g = 0; g < gr; ++g) emit_granule(0, t, base, ocnt, osrc, C, g, flt, gword, gcnt, gbase, out, cap32);
        *n = base[C];
    } else {
        gword.assign(n_gran, 0);
        gcnt.assign((size_t)n_gran + 1, 0u);
        gbase.assign((size_t)n_gran + 1, 0u);
        for (uint32_t g = 0; g < n_gran; ++g) emit_granule(1, t, base, ocnt, osrc, C, g, flt, gword, gcnt, gbase, out, cap32);
        exclusive_scan(gcnt, gbase);
        if (cap32)
            for (uint32_t g = 0; g < n_gran; ++g)
                emit_granule(2, t, base, ocnt, osrc, C, g, flt, gword, gcnt, gbase, out, cap32);
        *n = gbase[n_gran];
    }
    if (pos[D] > C || base[C] > h.rows) return -3;
    return *n > capacity ? -5 : 0;
}

}  // namespace

// Cube c: world[c], key[3 c ..], peers[off[c] .. off[c + 1]) ascending (none: a cube that was emptied
// and keeps its key). by_peer = 0: every peer. out: capacity rows of 5 words.
extern "C" int wq_test_table_export_host(uint16_t cube_size, size_t n_cubes, const uint32_t* world, const int64_t* key,
                                         const uint32_t* off, const uint32_t* peers, uint32_t f_world, int by_peer,
                                         const uint32_t* f_peers, uint32_t f_n_peers, uint64_t* out, size_t capacity,
                                         size_t* n) {
    HostTable t;
    build(t, cube_size, n_cubes, world, key, off, peers);
    return export_host(t, cube_size, f_world, by_peer, f_peers, f_n_peers, out, capacity, n);
}

#ifdef WQ_TABLE_EXPORT_SHIM_MAIN
#include <stdio.h>

#include <array>
#include <map>
#include <random>
#include <set>

int main() {
    std::mt19937_64 rng(11);
    const uint32_t lens[] = {0, 1, 2, 23, 24, 25, 63, 64, 65, 257, 1025};
    int bad = 0, runs = 0;
    for (int round = 0; round < 60; ++round) {
        const uint16_t cs = round % 3 == 0 ? 10 : 16;
        const size_t nc = round == 0 ? 0 : 1 + rng() % 200;
        std::map<std::array<int64_t, 4>, std::vector<uint32_t>> cubes;  // (world, key) -> peers
        while (cubes.size() < nc) {
            std::array<int64_t, 4> c;
            const uint64_t kind = rng() % 16;
            c[0] = kind == 0 ? (1 << 24) + (int64_t)(rng() % 3) : (int64_t)(rng() % 3);
            for (int d = 1; d < 4; ++d) {
                c[d] = ((int64_t)(rng() % 9) - 4) * cs;
                if (kind == 1) c[d] += 1 + (int64_t)(rng() % 3);                      // off grid
                if (kind == 2) c[d] = (rng() & 1 ? 1 : -1) * (int64_t)((1 << 23) - 1) * cs;  // the packed range's ends
                if (kind == 3) c[d] = (int64_t)rng();                                  // anything
            }
            if (cubes.count(c)) continue;
            std::set<uint32_t> ps;
            const uint32_t n = lens[rng() % 11];
            while (ps.size() < n) ps.insert((uint32_t)(rng() % 3000));
            cubes[c].assign(ps.begin(), ps.end());
        }
        std::vector<uint32_t> world, off{0}, peers;
        std::vector<int64_t> key;
        std::vector<std::array<int64_t, 4>> order;
        for (auto& kv : cubes) order.push_back(kv.first);
        std::shuffle(order.begin(), order.end(), rng);
        for (auto& c : order) {
            world.push_back((uint32_t)c[0]);
            key.insert(key.end(), c.begin() + 1, c.end());
            peers.insert(peers.end(), cubes[c].begin(), cubes[c].end());
            off.push_back((uint32_t)peers.size());
        }
        for (int form = 0; form < 4; ++form) {
            const uint32_t f_world = form & 1 ? (uint32_t)(rng() % 3) : kWorldEmpty;
            const int by_peer = form >> 1;
            std::vector<uint32_t> fp;
            if (by_peer)
                for (uint32_t i = 0, m = (uint32_t)(rng() % 400); i < m; ++i) fp.push_back((uint32_t)(rng() % 3300));
            const std::set<uint32_t> want_p(fp.begin(), fp.end());
            std::vector<uint64_t> want;  // the map iterates in (world, x, y, z) order; peers ascend
            for (auto& kv : cubes) {
                if (f_world != kWorldEmpty && (uint32_t)kv.first[0] != f_world) continue;
                for (uint32_t p : kv.second) {
                    if (by_peer && !want_p.count(p)) continue;
                    want.push_back((uint64_t)(uint32_t)kv.first[0] | ((uint64_t)p << 32));
                    want.push_back(1ull << 8);
                    for (int d = 1; d < 4; ++d) want.push_back((uint64_t)kv.first[d]);
                }
            }
            const size_t rows = want.size() / 5;
            const size_t caps[] = {rows, rows ? rows - 1 : 0, rows / 2, 1, 0, rows + 7};
            for (size_t cap : caps) {
                // exactly sized: the address sanitizer sees any write past the capacity
                std::vector<uint64_t> out(cap * 5, 0x5A5A5A5A5A5A5A5Aull);
                size_t n = ~(size_t)0;
                const int rc = wq_test_table_export_host(cs, order.size(), world.data(), key.data(), off.data(),
                                                         peers.data(), f_world, by_peer, fp.data(), (uint32_t)fp.size(),
                                                         out.data(), cap, &n);
                const size_t kept = std::min(rows, cap);
                bad += n != rows || rc != (rows > cap ? -5 : 0);
                bad += !std::equal(out.begin(), out.begin() + kept * 5, want.begin());
                for (size_t i = kept * 5; i < out.size(); ++i) bad += out[i] != 0x5A5A5A5A5A5A5A5Aull;
                runs++;
            }
        }
    }
    printf("table export host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
