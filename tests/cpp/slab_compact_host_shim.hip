// Test-only shim: runs the slab compaction's arithmetic (csrc/compact_ops.hpp: an entry's term under the
// range rule, the scan's pair and operator, the all-or-nothing decision, the chunk a quad lane writes; the
// element search, window, composer and stores of csrc/pack_ops.hpp) on the CPU in the passes and shapes the
// kernels of csrc/wq_slab_compact.hip use — terms by quads of 16-byte chunks, the scan, the decision, the
// entries by quads with the dense list, then the copy tile by tile in the blocks' consecutive runs, 64 lanes
// of one chunk each — so the result is checked byte for byte against worldql_server_amd/records.py
// (slab_compact_np) without a GPU (tests/test_slab_compact_cpp_mirror.py). The GPU instance:
// tests/test_gpu_slab_compact.py.
//
// With -DWQ_SLAB_COMPACT_SHIM_MAIN the file is a program of its own: random and hostile slabs on exactly
// sized heap arrays, for a host build under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../worldql_server_amd/csrc/compact_ops.hpp"

extern "C" uint32_t wq_test_slab_compact_sizes() {
    return (uint32_t)(sizeof(wq_slab_entry) | sizeof(wq_slab_compact_counters) << 8 | sizeof(wq::CmpChunk) << 16);
}

namespace {

// Chunk t of an entry array, as a lane's one 16-byte load.
wq::CmpChunk load_chunk(const wq_slab_entry* entries, uint64_t t) {
    wq::CmpChunk v;
    memcpy(&v, reinterpret_cast<const uint8_t*>(entries) + 16 * t, 16);
    return v;
}

}  // namespace

// As wq_slab_compact_device, with `blocks` one-wave blocks sharing the tiles (0: the kernel's count).
// Returns the number of tiles that took the whole-tile path.
extern "C" uint64_t wq_test_slab_compact_host(const wq_slab_view* src, const wq_slab_view* dst, uint64_t* cursor,
                                              wq_slab_compact_counters* counters, uint64_t blocks) {
    using namespace wq;
    const uint64_t n = src->n_entries;
    CmpCtrl ctrl{0, 0, 0, 0};
    // size: quads; lane 3 has chunk 3 and takes the bits from lane 2's chunk
    std::vector<uint64_t> term(n);
    for (uint64_t i = 0; i < n; ++i) {
        CmpChunk q[kCmpQuad];
        for (uint32_t c = 0; c < kCmpQuad; ++c) q[c] = load_chunk(src->entries, i * kCmpQuad + c);
        uint32_t err = 0;
        term[i] = cmp_term(q[2].w, cmp_chunk_off(q[3]), q[3].z, q[3].w, src->n_payload_bytes, &err);
        ctrl.error |= err;
        if (cmp_live(term[i])) ctrl.max_need = std::max<uint64_t>(ctrl.max_need, i + 1);
    }
    // scan
    std::vector<CmpKE> KE(n + 1);
    CmpKE at{0, 0};
    for (uint64_t i = 0; i <= n; ++i) {
        KE[i] = at;
        at = CmpPlus()(at, cmp_ke(term.data(), n, i));
    }
    // decide
    std::vector<uint64_t> dE(n + 1), dS(n);
    const CmpKE sum = KE[n];
    ctrl.overflow = cmp_decide(sum.e, ctrl.max_need, *dst);
    ctrl.n_live = sum.k;
    dE[sum.k] = sum.e;
    if (!ctrl.overflow) *cursor = sum.e;
    if (counters) {
        wq_slab_compact_counters c;
        c.n_entries = n, c.n_live = sum.k, c.bytes_live = sum.e, c.entries_need = ctrl.max_need;
        c.overflow = ctrl.overflow, c.error = ctrl.error;
        *counters = c;
    }
    if (ctrl.overflow) return 0;
    // entries: quads over the destination
    for (uint64_t t = 0; t < dst->n_entries * kCmpQuad; ++t) {
        const uint64_t i = t / kCmpQuad;
        const uint32_t c = (uint32_t)(t % kCmpQuad);
        const uint64_t tm = i < n ? term[i] : 0ull;
        const bool kept = cmp_live(tm);
        CmpChunk v{0, 0, 0, 0};
        CmpKE k{0, 0};
        if (kept) {
            v = load_chunk(src->entries, t);
            if (c == 3) {
                k = KE[i];
                dE[k.k] = k.e;
                dS[k.k] = cmp_size(tm) ? cmp_chunk_off(v) : 0ull;
            }
        }
        const CmpChunk w = cmp_entry_chunk(c, v, kept, tm, k.e);
        memcpy(reinterpret_cast<uint8_t*>(dst->entries) + 16 * t, &w, 16);
    }
    // copy
    if (!n || !dst->n_payload_bytes) return 0;
    uint8_t* out = dst->payload;
    const uint8_t* in = src->payload;
    if (!blocks) blocks = pack_blocks(dst->n_payload_bytes);
    const uint32_t T = (uint32_t)ctrl.n_live;
    const uint64_t total = dE[T], tiles = cmp_tiles(total), per = pack_tiles_per_block(total, blocks);
    uint64_t fast_tiles = 0;
    uint32_t hint = 0;
    uint64_t W[kPackWindow + 1], S[kPackWindow];
    for (uint64_t ti = 0; ti < tiles; ++ti) {
        const uint64_t c0 = ti * kPackTile, c1 = std::min(c0 + kPackTile, total);
        const uint32_t e0 = ti % per == 0 ? pack_elem_of(dE.data(), T, c0) : pack_elem_from(dE.data(), T, hint, c0);
        hint = e0;
        const uint64_t r0 = dE[e0], r1 = dE[e0 + 1];
        uint64_t d0[kPackLanes], hi[kPackLanes];
        for (uint32_t lane = 0; lane < kPackLanes; ++lane) {
            d0[lane] = c0 + (uint64_t)lane * kPackChunk;
            hi[lane] = std::min(d0[lane] + kPackChunk, c1);
        }
        if (pack_tile_inside(r0, r1, 0, c0, c1)) {
            for (uint32_t lane = 0; lane < kPackLanes; ++lane)
                pack_store(out, d0[lane], kPackChunk, pack_load16(in + dS[e0] + (d0[lane] - r0)));
            fast_tiles++;
            continue;
        }
        PackChunk v[kPackLanes];
        for (auto& x : v) x = PackChunk{0, 0};
        for (uint64_t wb = e0;; wb += kPackWindow) {
            for (uint32_t i = 0; i <= kPackWindow; ++i) W[i] = pack_win_entry(dE.data(), T, wb, i);
            for (uint32_t i = 0; i < kPackWindow; ++i) S[i] = wb + i < T ? dS[wb + i] : 0ull;
            for (uint32_t lane = 0; lane < kPackLanes; ++lane) {
                const uint64_t a = std::max(d0[lane], W[0]), b = std::min(hi[lane], W[kPackWindow]);
                if (a < b) pack_compose(W, S, in, src->n_payload_bytes, 0, d0[lane], a, b, &v[lane]);
            }
            if (W[kPackWindow] >= c1) {
                hint = (uint32_t)wb + pack_win_find(W, c1 - 1);
                break;
            }
        }
        for (uint32_t lane = 0; lane < kPackLanes; ++lane)
            if (d0[lane] < hi[lane]) pack_store(out, d0[lane], (uint32_t)(hi[lane] - d0[lane]), v[lane]);
    }
    return fast_tiles;
}

#ifdef WQ_SLAB_COMPACT_SHIM_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <random>

namespace {

// Exactly sized, 16-byte aligned heap bytes: the address sanitizer sees the first byte past them.
struct AlignedBytes {
    uint8_t* p = nullptr;
    size_t n = 0;
    AlignedBytes(size_t n_, uint8_t fill) : n(n_) {
        if (n && posix_memalign(reinterpret_cast<void**>(&p), 16, n)) abort();
        if (n) memset(p, fill, n);
    }
    AlignedBytes(const AlignedBytes&) = delete;
    ~AlignedBytes() { free(p); }
};

// The contract restated: live entries in handle order, their bytes appended, everything else zero.
struct Want {
    std::vector<wq_slab_entry> entries;  // as long as the source
    std::vector<uint8_t> bytes;
    uint64_t need_entries = 0, live = 0;
    uint32_t error = 0;
};

Want restate(const std::vector<wq_slab_entry>& src, const std::vector<uint8_t>& arena) {
    Want w;
    w.entries.resize(src.size());
    if (!src.empty()) memset(w.entries.data(), 0, src.size() * sizeof(wq_slab_entry));
    for (size_t i = 0; i < src.size(); ++i) {
        if (!(src[i].bits & WQ_SLAB_LIVE)) continue;
        wq_slab_entry e = src[i];
        const unsigned __int128 end = (unsigned __int128)e.off + e.data_len + e.flex_len;
        if (end > arena.size()) {
            w.error |= 1;
            e.data_len = e.flex_len = 0;
        } else {
            w.bytes.insert(w.bytes.end(), arena.begin() + e.off, arena.begin() + (size_t)end);
        }
        e.off = w.bytes.size() - e.data_len - e.flex_len;
        w.entries[i] = e;
        w.need_entries = i + 1;
        w.live++;
    }
    return w;
}

int run(const std::vector<wq_slab_entry>& src_e, const std::vector<uint8_t>& src_b, const Want& w, uint64_t n_entries,
        uint64_t n_bytes, uint64_t blocks) {
    AlignedBytes se(src_e.size() * sizeof(wq_slab_entry), 0), sb(src_b.size(), 0);
    if (se.n) memcpy(se.p, src_e.data(), se.n);
    if (sb.n) memcpy(sb.p, src_b.data(), sb.n);
    AlignedBytes arena(n_bytes, 0xEE), ent(n_entries * sizeof(wq_slab_entry), 0xEE);
    const wq_slab_view sv{reinterpret_cast<wq_slab_entry*>(se.p), src_e.size(), sb.p, src_b.size()};
    const wq_slab_view dv{reinterpret_cast<wq_slab_entry*>(ent.p), n_entries, arena.p, n_bytes};
    uint64_t cursor = 0xC0FFEE;
    wq_slab_compact_counters cnt;
    wq_test_slab_compact_host(&sv, &dv, &cursor, &cnt, blocks);
    const uint64_t total = w.bytes.size();
    const bool over_a = total > n_bytes, over_e = w.need_entries > n_entries, over = over_a || over_e;
    int bad = cnt.overflow != ((over_a ? 1u : 0u) | (over_e ? 2u : 0u)) || cnt.error != w.error || cnt.bytes_live != total ||
              cnt.entries_need != w.need_entries || cnt.n_live != w.live || cnt.n_entries != src_e.size();
    bad += cursor != (over ? 0xC0FFEE : total);
    for (uint64_t h = 0; h < n_entries; ++h) {
        wq_slab_entry e;
        memset(&e, over ? 0xEE : 0, sizeof e);
        if (!over && h < src_e.size()) e = w.entries[h];
        bad += memcmp(ent.p + h * sizeof e, &e, sizeof e) != 0;
    }
    for (uint64_t i = 0; i < n_bytes; ++i) bad += arena.p[i] != (!over && i < total ? w.bytes[i] : 0xEE);
    // no input is written
    bad += se.n && memcmp(se.p, src_e.data(), se.n) != 0;
    bad += sb.n && memcmp(sb.p, src_b.data(), sb.n) != 0;
    return bad;
}

}  // namespace

int main() {
    std::mt19937_64 rng(53);
    const uint32_t lens[] = {0, 0, 1, 2, 3, 5, 15, 16, 17, 31, 33, 40, 64, 100, 200, 1022, 1024, 1026, 4095, 4097};
    int bad = 0, runs = 0, hostile_rounds = 0;
    for (int round = 0; round < 120; ++round) {
        const bool hostile = round % 3 == 2;
        hostile_rounds += hostile;
        const size_t n = round % 13 == 0 ? 0 : 1 + rng() % (round % 4 == 1 ? 700 : 60);
        std::vector<wq_slab_entry> src(n);
        std::vector<uint8_t> arena;
        // the arena in a random handle order, junk between the payloads
        std::vector<size_t> order(n);
        for (size_t i = 0; i < n; ++i) order[i] = i;
        std::shuffle(order.begin(), order.end(), rng);
        const unsigned p_dead = (unsigned)(rng() % 101);
        for (size_t i : order) {
            wq_slab_entry e;
            for (uint8_t& b : e.uuid) b = (uint8_t)rng();
            for (double& x : e.pos) x = (double)(int64_t)(rng() % 2000) - 1000.0;
            e.world = (uint32_t)rng() % 7;
            const bool big = round == 7 && i == n / 2;
            e.data_len = big ? (1u << 20) + 3 : round % 4 == 1 ? (uint32_t)(rng() % 4) : lens[rng() % 20];
            e.flex_len = round % 4 == 1 ? (uint32_t)(rng() % 3) : lens[rng() % 20];
            e.bits = (uint32_t)(rng() % 8) | (rng() % 100 >= p_dead ? WQ_SLAB_LIVE : 0u);
            for (size_t g = rng() % 4; g; --g) arena.push_back((uint8_t)rng());
            e.off = arena.size();
            for (uint64_t k = 0; k < (uint64_t)e.data_len + e.flex_len; ++k) arena.push_back((uint8_t)rng());
            src[i] = e;
        }
        if (hostile)
            for (size_t i = 0; i < n; ++i) {
                if (rng() % 4) continue;
                wq_slab_entry& e = src[i];
                switch (rng() % 7) {
                    case 0: e.off = arena.size() - std::min<uint64_t>(arena.size(), (uint64_t)e.data_len + e.flex_len) + 1, e.data_len += !e.data_len && !e.flex_len; break;
                    case 1: e.off = arena.size() + 1 + rng() % 5; break;
                    case 2: e.off = 0xFFFFFFFFFFFFFFF8ull, e.data_len = 16; break;
                    case 3: e.data_len = e.flex_len = 0xFFFFFFFFu; break;
                    case 4: e.off = 0xFFFFFFFFFFFFFFFFull, e.data_len = e.flex_len = 0; break;
                    case 5: e.off = src[rng() % n].off; break;  // a shared or overlapping range (or one that leaves)
                    default: e.off = rng(); break;
                }
            }
        const Want w = restate(src, arena);
        const uint64_t total = w.bytes.size(), ne = w.need_entries;
        std::vector<uint64_t> caps{total, total + 1 + rng() % 2000};
        if (total) caps.push_back(total - 1), caps.push_back(0);
        for (uint64_t cap : caps)
            for (uint64_t e : {ne, ne + 3, (uint64_t)n, ne ? ne - 1 : 0}) {
                bad += run(src, arena, w, e, cap, runs % 3 == 0 ? 0 : 1 + rng() % 5);
                runs++;
            }
        // idempotence: the canonical form compacts to itself
        if (total || ne) {
            std::vector<wq_slab_entry> canon(w.entries.begin(), w.entries.begin() + ne);
            const Want again = restate(canon, w.bytes);
            bad += again.bytes != w.bytes || (ne && memcmp(again.entries.data(), canon.data(), ne * sizeof(wq_slab_entry)) != 0);
            bad += run(canon, w.bytes, again, ne, total, 2);
            runs++;
        }
    }
    printf("slab_compact host check: %d rounds (%d hostile), %d runs, %d mismatches\n", 120, hostile_rounds, runs, bad);
    return bad ? 1 : 0;
}
#endif
