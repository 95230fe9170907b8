// Test-only shim: runs the record payload slab's arithmetic (csrc/slab_ops.hpp: an op's two elements under
// the validity rules, the scan's terms, the all-or-nothing decision, the entry of a create, the arena's
// tiles and the head store; the element search, window, composer and stores of csrc/pack_ops.hpp) on the
// CPU in the passes and tile sizes the kernels of csrc/wq_slab.hip use — sizes, the scan, the decision,
// the entries, then the copy tile by tile in the blocks' consecutive runs, 64 lanes of one chunk each —
// so the result is checked byte for byte against worldql_server_amd/records.py (slab_store_np) without a
// GPU (tests/test_slab_store_cpp_mirror.py). The GPU instance: tests/test_gpu_slab_store.py.
//
// With -DWQ_SLAB_SHIM_MAIN the file is a program of its own: random and hostile inputs on exactly sized
// heap arrays, for a host build under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../worldql_server_amd/csrc/slab_ops.hpp"

extern "C" uint32_t wq_test_slab_sizes() {
    return (uint32_t)(sizeof(wq_slab_entry) | sizeof(wq_slab_view) << 8 | sizeof(wq_slab_counters) << 16);
}

// As wq_slab_store_device, with `blocks` one-wave blocks sharing the tiles (0: the kernel's count).
// Returns the number of tiles that took the whole-tile path.
extern "C" uint64_t wq_test_slab_store_host(const wq_rec_op* ops, const wq_rec_op_ref* refs, size_t n_ops,
                                            const uint8_t* frames, const uint64_t* fo, size_t n_frames,
                                            const wq_slab_view* view, uint64_t* cursor, wq_slab_counters* counters,
                                            uint64_t blocks) {
    using namespace wq;
    const SlabIn in{ops, refs, frames, fo, (uint64_t)n_ops, (uint64_t)n_frames};
    const uint32_t T = (uint32_t)(2 * n_ops);
    SlabCtrl ctrl{0, 0, 0, 0, 0};
    // size
    std::vector<uint32_t> size(T);
    std::vector<uint64_t> src(T);
    for (uint64_t q = 0; q < n_ops; ++q) {
        const SlabParts p = slab_parts(in, q);
        size[2 * q] = p.len[0], size[2 * q + 1] = p.len[1];
        src[2 * q] = p.src[0], src[2 * q + 1] = p.src[1];
        ctrl.error |= p.err;
        if (p.create) {
            ctrl.max_need = std::max<uint64_t>(ctrl.max_need, (uint64_t)ops[q].handle + 1);
            ctrl.n_creates++;
        }
    }
    // scan
    std::vector<uint64_t> E((size_t)T + 1, 0);
    uint64_t at = 0;
    for (uint64_t k = 0; k <= T; ++k) {
        E[k] = at;
        at += slab_term(size.data(), T, k);
    }
    // decide
    const uint64_t base = *cursor, total = E[T], end = base + total;
    ctrl.base = base;
    ctrl.overflow = slab_decide(base, total, ctrl.max_need, *view);
    if (!ctrl.overflow) *cursor = end;
    if (counters) {
        wq_slab_counters c;
        c.n_ops = n_ops, c.n_creates = ctrl.n_creates, c.bytes_stored = total, c.bytes_need = total > ~0ull - base ? ~0ull : end;
        c.entries_need = ctrl.max_need, c.cursor = ctrl.overflow ? base : end;
        c.overflow = ctrl.overflow, c.error = ctrl.error;
        *counters = c;
    }
    if (ctrl.overflow) return 0;
    // entries
    for (uint64_t q = 0; q < n_ops; ++q)
        if (ops[q].kind == WQ_RECORD_CREATE)
            view->entries[ops[q].handle] = slab_entry(in, q, base + E[2 * q], size[2 * q], size[2 * q + 1]);
    // copy
    if (!n_ops || !view->n_payload_bytes) return 0;
    uint8_t* out = view->payload;
    if (!blocks) blocks = slab_blocks(view->n_payload_bytes);
    const uint64_t tiles = slab_tiles(base, total), per = slab_tiles_per_block(tiles, blocks);
    const uint64_t n_frame_bytes = slab_frame_bytes(in);
    uint64_t fast_tiles = 0;
    uint32_t hint = 0;
    uint64_t W[kPackWindow + 1], S[kPackWindow];
    for (uint64_t ti = 0; ti < tiles; ++ti) {
        const uint64_t a0 = slab_tile0(base) + ti * kPackTile;
        const uint64_t c0 = std::max(a0, base), c1 = std::min(a0 + kPackTile, end);
        const uint32_t e0 = ti % per == 0 ? pack_elem_of(E.data(), T, c0 - base) : pack_elem_from(E.data(), T, hint, c0 - base);
        hint = e0;
        const uint64_t r0 = base + E[e0], r1 = base + E[e0 + 1];
        uint64_t d0[kPackLanes], lo[kPackLanes], hi[kPackLanes];
        for (uint32_t lane = 0; lane < kPackLanes; ++lane) {
            d0[lane] = a0 + (uint64_t)lane * kPackChunk;
            lo[lane] = std::max(d0[lane], c0);
            hi[lane] = std::min(d0[lane] + kPackChunk, c1);
        }
        if (pack_tile_inside(r0, r1, 0, c0, c1)) {
            for (uint32_t lane = 0; lane < kPackLanes; ++lane)
                pack_store(out, d0[lane], kPackChunk, pack_load16(frames + src[e0] + (d0[lane] - r0)));
            fast_tiles++;
            continue;
        }
        PackChunk v[kPackLanes];
        for (auto& x : v) x = PackChunk{0, 0};
        for (uint64_t wb = e0;; wb += kPackWindow) {
            for (uint32_t i = 0; i <= kPackWindow; ++i) W[i] = base + pack_win_entry(E.data(), T, wb, i);
            for (uint32_t i = 0; i < kPackWindow; ++i) S[i] = wb + i < T ? src[wb + i] : 0ull;
            for (uint32_t lane = 0; lane < kPackLanes; ++lane) {
                const uint64_t a = std::max(lo[lane], W[0]), b = std::min(hi[lane], W[kPackWindow]);
                if (a < b) pack_compose(W, S, frames, n_frame_bytes, 0, d0[lane], a, b, &v[lane]);
            }
            if (W[kPackWindow] >= c1) {
                hint = (uint32_t)wb + pack_win_find(W, c1 - 1);
                break;
            }
        }
        for (uint32_t lane = 0; lane < kPackLanes; ++lane)
            if (lo[lane] < hi[lane]) slab_store(out, d0[lane], lo[lane], hi[lane], v[lane]);
    }
    return fast_tiles;
}

#ifdef WQ_SLAB_SHIM_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>

namespace {

// Exactly sized, 16-byte aligned heap bytes: the address sanitizer sees the first byte past them.
struct AlignedBytes {
    uint8_t* p = nullptr;
    size_t n = 0;
    explicit AlignedBytes(size_t n_, uint8_t fill) : n(n_) {
        if (n && posix_memalign(reinterpret_cast<void**>(&p), 16, n)) abort();
        if (n) memset(p, fill, n);
    }
    AlignedBytes(const AlignedBytes&) = delete;
    ~AlignedBytes() { free(p); }
};

struct Case {
    std::vector<wq_rec_op> ops;
    std::vector<wq_rec_op_ref> refs;
    std::vector<uint8_t> frames;
    std::vector<uint64_t> fo;
};

// The contract restated: creates in op order, data then flex appended at the cursor.
struct Want {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;  // per op
    std::vector<uint32_t> dl, fl;
    uint64_t need_entries = 0, creates = 0;
    uint32_t error = 0;
};

Want restate(const Case& c) {
    Want w;
    const uint64_t nf = c.fo.size() - 1, nb = nf ? c.fo[nf] : 0;
    for (size_t q = 0; q < c.ops.size(); ++q) {
        w.off.push_back(w.bytes.size());
        w.dl.push_back(0), w.fl.push_back(0);
        if (c.ops[q].kind != WQ_RECORD_CREATE) continue;
        w.creates++;
        w.need_entries = std::max<uint64_t>(w.need_entries, (uint64_t)c.ops[q].handle + 1);
        const wq_rec_op_ref& r = c.refs[q];
        const uint32_t len[2] = {(r.bits & 1) ? r.data_len : 0, (r.bits & 2) ? r.flex_len : 0}, off[2] = {r.data_off, r.flex_off};
        if (!len[0] && !len[1]) continue;
        if (r.frame >= nf || c.fo[r.frame] > c.fo[r.frame + 1] || c.fo[r.frame + 1] > nb) {
            w.error |= 1;
            continue;
        }
        const uint64_t a = c.fo[r.frame], fl = c.fo[r.frame + 1] - a;
        for (int k = 0; k < 2; ++k) {
            if (!len[k]) continue;
            if ((uint64_t)off[k] + len[k] > fl) {
                w.error |= k ? 4 : 2;
                continue;
            }
            w.bytes.insert(w.bytes.end(), c.frames.begin() + a + off[k], c.frames.begin() + a + off[k] + len[k]);
            (k ? w.fl : w.dl)[q] = len[k];
        }
    }
    return w;
}

int run(const Case& c, const Want& w, uint64_t cursor0, uint64_t n_entries, uint64_t n_bytes, uint64_t blocks) {
    AlignedBytes arena(n_bytes, 0xEE), ent(n_entries * sizeof(wq_slab_entry), 0xEE);
    wq_slab_view v{reinterpret_cast<wq_slab_entry*>(ent.p), n_entries, arena.p, n_bytes};
    uint64_t cursor = cursor0;
    wq_slab_counters cnt;
    // exactly sized copies of the inputs
    std::vector<wq_rec_op> ops(c.ops);
    std::vector<wq_rec_op_ref> refs(c.refs);
    std::vector<uint8_t> frames(c.frames);
    std::vector<uint64_t> fo(c.fo);
    wq_test_slab_store_host(ops.data(), refs.data(), ops.size(), frames.data(), fo.data(), fo.size() - 1, &v, &cursor, &cnt, blocks);
    const uint64_t total = w.bytes.size();
    const bool over_a = cursor0 > n_bytes || total > n_bytes - cursor0, over_e = w.need_entries > n_entries;
    int bad = cnt.overflow != ((over_a ? 1u : 0u) | (over_e ? 2u : 0u)) || cnt.error != w.error || cnt.bytes_stored != total ||
              cnt.bytes_need != cursor0 + total || cnt.entries_need != w.need_entries || cnt.n_creates != w.creates;
    const bool over = over_a || over_e;
    bad += cursor != (over ? cursor0 : cursor0 + total) || cnt.cursor != cursor;
    std::vector<uint8_t> live(n_entries, 0);
    if (!over)
        for (size_t q = 0; q < c.ops.size(); ++q) {
            if (c.ops[q].kind != WQ_RECORD_CREATE) continue;
            const wq_slab_entry& e = v.entries[c.ops[q].handle];
            live[c.ops[q].handle] = 1;
            bad += e.off != cursor0 + w.off[q] || e.data_len != w.dl[q] || e.flex_len != w.fl[q] || e.world != c.ops[q].world;
            bad += e.bits != ((c.refs[q].bits & 3u) | 4u | 0x80000000u) || memcmp(e.pos, c.ops[q].pos, 24) != 0;
            for (int i = 0; i < 8; ++i)
                bad += e.uuid[i] != (uint8_t)(c.ops[q].uuid_hi >> (8 * (7 - i))) || e.uuid[8 + i] != (uint8_t)(c.ops[q].uuid_lo >> (8 * (7 - i)));
        }
    for (uint64_t h = 0; h < n_entries; ++h)
        if (!live[h])
            for (size_t i = 0; i < sizeof(wq_slab_entry); ++i) bad += ent.p[h * sizeof(wq_slab_entry) + i] != 0xEE;
    for (uint64_t i = 0; i < n_bytes; ++i) {
        const bool in = !over && i >= cursor0 && i < cursor0 + total;
        bad += arena.p[i] != (in ? w.bytes[i - cursor0] : 0xEE);
    }
    return bad;
}

}  // namespace

int main() {
    std::mt19937_64 rng(47);
    const uint32_t lens[] = {0, 0, 1, 2, 3, 5, 15, 16, 17, 31, 33, 40, 64, 100, 200, 1022, 1024, 1026, 4095, 4097};
    int bad = 0, runs = 0;
    for (int round = 0; round < 80; ++round) {
        Case c;
        const size_t n_frames = round % 11 == 0 ? 0 : 1 + rng() % 12;
        c.fo.push_back(0);
        for (size_t f = 0; f < n_frames; ++f) {
            const size_t n = round == 5 && f == 0 ? (1u << 20) + 77 : rng() % 6000;
            for (size_t i = 0; i < n; ++i) c.frames.push_back((uint8_t)rng());
            c.fo.push_back(c.frames.size());
        }
        const size_t n_ops = round % 13 == 0 ? 0 : 1 + rng() % (round % 4 == 1 ? 300 : 40);
        const bool hostile = round % 3 == 2;
        for (size_t q = 0; q < n_ops; ++q) {
            wq_rec_op op{};
            op.kind = rng() % 5 == 0 ? WQ_RECORD_DELETE : WQ_RECORD_CREATE;
            op.world = (uint32_t)rng() % 7;
            for (double& x : op.pos) x = (double)(int64_t)(rng() % 2000) - 1000.0;
            op.uuid_hi = rng(), op.uuid_lo = rng();
            op.handle = (uint32_t)q * 2 + 1;  // distinct
            wq_rec_op_ref r{};
            r.frame = n_frames ? (uint32_t)(rng() % n_frames) : 0;
            const uint64_t fl = n_frames ? c.fo[r.frame + 1] - c.fo[r.frame] : 0;
            r.bits = (uint32_t)rng() % 4;
            const bool big = round == 5 && q == 0;
            if (big) r.frame = 0, r.bits = 3;
            r.data_len = (uint32_t)std::min<uint64_t>(fl, round % 4 == 1 ? rng() % 4 : lens[rng() % 20]);
            r.data_off = (uint32_t)(fl - r.data_len ? rng() % (fl - r.data_len + 1) : 0);
            r.flex_len = big ? 1u << 20 : (uint32_t)std::min<uint64_t>(fl, round % 4 == 1 ? rng() % 3 : lens[rng() % 20]);
            r.flex_off = (uint32_t)(fl - r.flex_len ? rng() % (fl - r.flex_len + 1) : 0);
            if (hostile && rng() % 4 == 0) {
                switch (rng() % 5) {
                    case 0: r.frame = (uint32_t)n_frames + (uint32_t)(rng() % 3); break;
                    case 1: r.data_off = 0xFFFFFFFFu, r.data_len = 0xFFFFFFFFu; break;
                    case 2: r.flex_off = (uint32_t)fl, r.flex_len = 1; break;
                    case 3: r.frame = 0xFFFFFFFFu; break;
                    default: r.data_len = (uint32_t)fl + 1, r.data_off = 0; break;
                }
            }
            c.ops.push_back(op), c.refs.push_back(r);
        }
        std::vector<Case> variants{c};
        if (hostile && n_frames > 2) {  // frame offsets that descend and pass the end
            Case f = c;
            std::swap(f.fo[1], f.fo[2]);
            variants.push_back(f);
            f = c;
            f.fo[n_frames / 2] = 0xFFFFFFFFFFFFFFFFull;
            variants.push_back(f);
        }
        for (const Case& v : variants) {
            const Want w = restate(v);
            const uint64_t total = w.bytes.size();
            for (uint64_t cursor0 : {(uint64_t)0, (uint64_t)(rng() % 40), (uint64_t)1024, (uint64_t)(1000 + rng() % 50)}) {
                const uint64_t fit = cursor0 + total;
                std::vector<uint64_t> caps{fit, fit + 16 + rng() % 2000};
                if (total) caps.push_back(fit - 1), caps.push_back(cursor0 ? cursor0 - 1 : 0);
                for (uint64_t cap : caps)
                    for (uint64_t ne : {w.need_entries, w.need_entries + 3, w.need_entries ? w.need_entries - 1 : 0}) {
                        bad += run(v, w, cursor0, ne, cap, runs % 3 == 0 ? 0 : 1 + rng() % 5);
                        runs++;
                    }
            }
        }
    }
    printf("slab_store host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
