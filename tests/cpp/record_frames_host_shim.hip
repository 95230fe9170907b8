// Test-only shim: runs the record reply builder's arithmetic (csrc/reply_ops.hpp with csrc/frame_ops.hpp and
// csrc/pack_ops.hpp, unchanged) on the CPU in the passes the kernels of csrc/wq_reply.hip use — rows, the terms,
// the segmented scan in blocks of any size, the place pass, the two prefix sums, the row sizes, the scan into the
// frame offsets, then the copy tile by tile in the blocks' consecutive runs, 64 lanes of one chunk each — so
// the result is checked byte for byte against worldql_server_amd/frames.py (build_record_frames_np) without a
// GPU (tests/test_record_frames_cpp_mirror.py). The GPU instance: tests/test_gpu_record_frames.py.
//
// With -DWQ_RECFRAMES_SHIM_MAIN the file is a program of its own: random slabs and rows on exactly sized heap
// arrays against its own restatement of the builder, for a host build under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../worldql_server_amd/csrc/reply_ops.hpp"

// The arguments of wq_frames_build_records_device with the table of wq_frames_set_worlds, all host memory.
struct wq_test_recframes_in {
    wq_frames_src src;
    wq_frames_rec_src rec;
    const uint8_t* table_bytes;
    const uint32_t* table_off;
    uint64_t n_table_bytes;
    uint32_t n_worlds;
    uint32_t scan_block;  // the segmented scan is folded in blocks of this many terms (0: one block)
    uint64_t blocks;      // one-wave blocks of the copy (0: the kernel's count)
};

extern "C" uint32_t wq_test_recframes_sizes() { return (uint32_t)(sizeof(wq_frames_src) | sizeof(wq_frames_rec_src) << 8); }

// As wq_frames_build_records_device. counters (nullable) = {n_frames, n_complete, bytes_need, bytes_written,
// overflow, error}. Returns the number of tiles that took the whole-tile path.
extern "C" uint64_t wq_test_record_frames_host(const wq_test_recframes_in* a, size_t n_msgs, uint8_t* out, size_t capacity,
                                               uint64_t* out_offsets, uint32_t* out_size, uint64_t* counters) {
    using namespace wq;
    auto u8 = [](const void* q) { return static_cast<const uint8_t*>(q); };
    const wq_frames_src& src = a->src;
    const wq_frames_rec_src& rec = a->rec;
    ReplyCtx c;
    FrameSrc& s = c.s;
    s.instruction = src.instruction, s.replication = src.replication, s.sender_uuid = src.sender_uuid;
    s.world = u8(src.world), s.pos = u8(src.pos), s.param = src.param, s.param_offsets = u8(src.param_offsets);
    s.flex = src.flex, s.flex_offsets = u8(src.flex_offsets), s.msg_flags = src.msg_flags;
    std::vector<uint8_t> table(a->n_table_bytes + 2 * kFrWorldSlack, 0);
    if (a->n_table_bytes) memcpy(table.data() + kFrWorldSlack, a->table_bytes, a->n_table_bytes);
    s.world_bytes = table.data() + kFrWorldSlack, s.world_off = a->table_off, s.world_slack = kFrWorldSlack;
    s.n = n_msgs, s.n_param_bytes = src.param_offsets ? src.n_param_bytes : 0;
    s.n_flex_bytes = src.flex_offsets ? src.n_flex_bytes : 0, s.n_world_bytes = a->n_table_bytes;
    s.n_worlds = a->n_worlds, s.instruction_all = src.instruction_all, s.replication_all = src.replication_all;
    const uint32_t nh = (uint32_t)rec.n_handles, n = (uint32_t)n_msgs;
    c.r = ReplySrc{rec.row_offsets, rec.handles, nh, rec.flags, rec.slab.entries, rec.slab.n_entries, rec.slab.payload,
                   rec.slab.n_payload_bytes, rec.world_bytes, u8(rec.world_off), u8(rec.world_len),
                   rec.world_bytes ? rec.n_world_bytes : 0};
    uint32_t error = 0;
    // rows: lengths, saturating prefix, the ordinal space
    const size_t rows = (size_t)n + 1;
    std::vector<uint32_t> len(rows, 0), sum(rows, 0), pre(rows, 0);
    for (uint32_t p = 0; p < n; ++p) {
        bool ok;
        len[p] = bud_len(rec.row_offsets, p, nh, &ok);
        if (!ok) error |= kRpErrRows;
    }
    for (size_t p = 1; p < rows; ++p) sum[p] = BudSatAdd()(sum[p - 1], len[p - 1]);
    for (size_t p = 0; p < rows; ++p) pre[p] = std::min(sum[p], nh);
    for (uint32_t p = 0; p < n; ++p)
        if (pre[p + 1] - pre[p] != len[p]) error |= kRpErrRows;
    const uint32_t T = pre[n];
    std::vector<uint32_t> X((size_t)nh + 1), term((size_t)nh + 1), sz((size_t)nh + 1), first(8 * rows, 0xDEADBEEFu);
    std::vector<uint64_t> P((size_t)nh + 1), K((size_t)nh + 1);
    c.pre = pre.data(), c.X = X.data(), c.term = term.data(), c.sz = sz.data(), c.P = P.data(), c.K = K.data();
    c.first = first.data();
    // terms
    for (uint32_t q = 0; q < T; ++q) term[q] = reply_term(c, bud_row_of(pre.data(), n, q), q, &error);
    // the segmented scan: block sums first, then each block from its prefix, as a device scan brackets it
    {
        const uint64_t N = (uint64_t)nh + 1, B = a->scan_block ? a->scan_block : N;
        auto t = [&](uint64_t q) { return q < T ? term[q] : kRpHead; };
        std::vector<uint32_t> block_sum;
        for (uint64_t b0 = 0; b0 < N; b0 += B) {
            uint32_t acc = t(b0);
            for (uint64_t q = b0 + 1; q < std::min(N, b0 + B); ++q) acc = rp_combine(acc, t(q));
            block_sum.push_back(acc);
        }
        uint32_t carry = 0;
        for (uint64_t b0 = 0, k = 0; b0 < N; b0 += B, ++k) {
            uint32_t acc = carry;
            for (uint64_t q = b0; q < std::min(N, b0 + B); ++q) {
                X[q] = acc;
                acc = rp_combine(acc, t(q));
            }
            carry = rp_combine(carry, block_sum[k]);
        }
    }
    // place, the prefix sums
    for (uint32_t q = 0; q < T; ++q) sz[q] = reply_place(c, bud_row_of(pre.data(), n, q), q);
    uint64_t at = 0, kept = 0;
    for (uint64_t q = 0; q <= nh; ++q) {
        P[q] = at, K[q] = kept;
        if (q < T) at += sz[q], kept += sz[q] != 0;
    }
    // row sizes and their scan
    std::vector<uint32_t> size(n);
    for (uint32_t i = 0; i < n; ++i) {
        size[i] = reply_size(c, i, &error);
        if (out_size) out_size[i] = size[i];
    }
    uint64_t* E = out_offsets;
    at = 0;
    for (uint64_t q = 0; q <= n; ++q) {
        E[q] = at;
        at += frame_term(size.data(), n, q);
    }
    // copy
    const uint64_t need = E[n], written = std::min<uint64_t>(need, capacity);
    uint64_t fast_tiles = 0;
    if (n && capacity) {
        const uint64_t blocks = a->blocks ? a->blocks : pack_blocks(capacity);
        const uint64_t per = pack_tiles_per_block(written, blocks);
        uint32_t hint = 0;
        uint64_t W[kPackWindow + 1];
        for (uint64_t tile = 0; tile * kPackTile < written; ++tile) {
            const uint64_t c0 = tile * kPackTile;
            const uint64_t c1 = written - c0 > kPackTile ? c0 + kPackTile : written;
            const uint32_t e0 = tile % per == 0 ? pack_elem_of(E, n, c0) : pack_elem_from(E, n, hint, c0);
            hint = e0;
            const uint64_t r0 = E[e0], r1 = E[e0 + 1];
            uint64_t d0[kPackLanes], d1[kPackLanes];
            for (uint32_t lane = 0; lane < kPackLanes; ++lane) {
                d0[lane] = c0 + (uint64_t)lane * kPackChunk;
                d1[lane] = d0[lane] >= c1 ? d0[lane] : (c1 - d0[lane] > kPackChunk ? d0[lane] + kPackChunk : c1);
            }
            const uint8_t* from;
            if (c1 - c0 == kPackTile && r1 - r0 >= kPackTile && reply_tile_inside(c, e0, r0, r1, c0, c1, &from)) {
                for (uint32_t lane = 0; lane < kPackLanes; ++lane)
                    pack_store(out, d0[lane], kPackChunk, pack_load16(from + (uint64_t)lane * kPackChunk));
                fast_tiles++;
                continue;
            }
            PackChunk v[kPackLanes];
            for (auto& x : v) x = PackChunk{0, 0};
            for (uint64_t wb = e0;; wb += kPackWindow) {
                for (uint32_t i = 0; i <= kPackWindow; ++i) W[i] = pack_win_entry(E, n, wb, i);
                for (uint32_t lane = 0; lane < kPackLanes; ++lane) {
                    const uint64_t lo = std::max(d0[lane], W[0]), hi = std::min(d1[lane], W[kPackWindow]);
                    if (lo < hi) reply_compose(W, wb, c, d0[lane], lo, hi, &v[lane]);
                }
                if (W[kPackWindow] >= c1) {
                    hint = (uint32_t)wb + pack_win_find(W, c1 - 1);
                    break;
                }
            }
            for (uint32_t lane = 0; lane < kPackLanes; ++lane)
                if (d0[lane] < d1[lane]) pack_store(out, d0[lane], (uint32_t)(d1[lane] - d0[lane]), v[lane]);
        }
    }
    if (counters) {
        counters[0] = n;
        counters[1] = pack_elem_of(E, n, capacity);
        counters[2] = need;
        counters[3] = written;
        counters[4] = need > capacity ? 1 : 0;
        counters[5] = error;
    }
    return fast_tiles;
}

#ifdef WQ_RECFRAMES_SHIM_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>

namespace {

// The reference builder restated from wq_codec.cpp's Builder: bytes pushed at the front of a growing
// buffer, vtables deduplicated by content.
struct RefBuilder {
    std::vector<uint8_t> rev;  // the frame reversed: rev[k] is the byte at revloc k + 1
    std::vector<uint32_t> vts;
    size_t min_align = 0;
    uint32_t used() const { return (uint32_t)rev.size(); }
    void put(const void* p, size_t n) {
        const uint8_t* b = static_cast<const uint8_t*>(p);
        for (size_t i = n; i-- > 0;) rev.push_back(b[i]);
    }
    void pad(size_t n) { rev.insert(rev.end(), n, 0); }
    void align(size_t len, size_t a) {
        min_align = std::max(min_align, a);
        pad((~(size_t(used()) + len) + 1) & (a - 1));
    }
    uint32_t u32(uint32_t v) { align(4, 4); put(&v, 4); return used(); }
    uint32_t off(uint32_t target) { align(4, 4); const uint32_t d = used() + 4 - target; put(&d, 4); return used(); }
    uint32_t str(const void* s, size_t n) { align(n + 1, 4); pad(1); put(s, n); return u32((uint32_t)n); }
    uint32_t bytes(const void* s, size_t n) { align(n, 4); put(s, n); return u32((uint32_t)n); }
    uint8_t at(uint32_t revloc, uint32_t i) const { return rev[revloc - 1 - i]; }
    uint32_t end_table(uint32_t start, const std::vector<std::pair<uint32_t, uint16_t>>& fields) {
        const uint32_t obj = u32(0);
        uint16_t max_id = 0;
        for (auto& f : fields) max_id = std::max(max_id, f.second);
        const uint16_t vt_len = max_id + 2;
        std::vector<uint8_t> vt(vt_len, 0);
        const uint16_t hdr[2] = {vt_len, (uint16_t)(obj - start)};
        memcpy(vt.data(), hdr, 4);
        for (auto& f : fields) {
            const uint16_t o = (uint16_t)(obj - f.first);
            memcpy(vt.data() + f.second, &o, 2);
        }
        uint32_t use = 0;
        for (size_t k = vts.size(); k-- > 0 && !use;) {
            bool same = at(vts[k], 0) == (vt_len & 255) && at(vts[k], 1) == (vt_len >> 8);
            for (uint32_t i = 0; same && i < vt_len; ++i) same = at(vts[k], i) == vt[i];
            if (same) use = vts[k];
        }
        if (!use) {
            put(vt.data(), vt_len);
            use = used();
            vts.push_back(use);
        }
        const int32_t so = (int32_t)use - (int32_t)obj;
        for (int i = 0; i < 4; ++i) rev[obj - 1 - i] = (uint8_t)((uint32_t)so >> (8 * i));
        return obj;
    }
};

std::string uuid_text(const uint8_t* u) {
    static const char* hex = "0123456789abcdef";
    std::string s;
    for (int i = 0; i < 16; ++i) {
        if (i == 4 || i == 6 || i == 8 || i == 10) s += '-';
        s += hex[u[i] >> 4];
        s += hex[u[i] & 15];
    }
    return s;
}

struct Rec {
    uint8_t uuid[16];
    double pos[3];
    std::string world;
    std::vector<uint8_t> data, flex;
    uint32_t shape;
};

std::vector<uint8_t> ref_frame(const uint8_t* sender, const std::string& world, uint8_t ins, uint8_t rep, const double* pos,
                               const std::vector<Rec>& recs) {
    RefBuilder b;
    const std::string su = uuid_text(sender);
    const uint32_t s_off = b.str(su.data(), 36), w_off = b.str(world.data(), world.size());
    std::vector<uint32_t> t;
    for (const Rec& r : recs) {
        const std::string u = uuid_text(r.uuid);
        const uint32_t uu = b.str(u.data(), 36), ww = b.str(r.world.data(), r.world.size());
        const uint32_t dd = (r.shape & 1) ? b.str(r.data.data(), r.data.size()) : 0;
        const uint32_t ff = (r.shape & 2) ? b.bytes(r.flex.data(), r.flex.size()) : 0;
        const uint32_t start = b.used();
        std::vector<std::pair<uint32_t, uint16_t>> f;
        if (r.shape & 2) f.push_back({b.off(ff), 12});
        if (r.shape & 1) f.push_back({b.off(dd), 10});
        f.push_back({b.off(ww), 8});
        if (r.shape & 4) { b.put(r.pos, 24); f.push_back({b.used(), 6}); }
        f.push_back({b.off(uu), 4});
        t.push_back(b.end_table(start, f));
    }
    b.align(4 * t.size(), 4);
    for (size_t i = t.size(); i-- > 0;) b.off(t[i]);
    const uint32_t records = b.u32((uint32_t)t.size());
    b.align(0, 4);
    const uint32_t entities = b.u32(0);
    const uint32_t start = b.used();
    std::vector<std::pair<uint32_t, uint16_t>> f;
    if (pos) { b.put(pos, 24); f.push_back({b.used(), 18}); }
    f.push_back({b.off(entities), 16});
    f.push_back({b.off(records), 14});
    f.push_back({b.off(w_off), 10});
    f.push_back({b.off(s_off), 8});
    if (rep) { b.put(&rep, 1); f.push_back({b.used(), 12}); }
    if (ins) { b.put(&ins, 1); f.push_back({b.used(), 4}); }
    const uint32_t root = b.end_table(start, f);
    b.align(4, b.min_align);
    b.off(root);
    return std::vector<uint8_t>(b.rev.rbegin(), b.rev.rend());
}

}  // namespace

int main() {
    std::mt19937_64 rng(53);
    const char* names[] = {"", "w", "ab", "abc", "four", "a_longer_world_name"};
    const uint32_t lens[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 40, 100, 1022, 1024, 1026, 4097};
    std::string tb;
    std::vector<uint32_t> toff{0};
    for (const char* nm : names) tb += nm, toff.push_back((uint32_t)tb.size());
    int bad = 0, runs = 0;
    for (int round = 0; round < 60; ++round) {
        // a slab of random records
        const size_t n_ent = 1 + rng() % 40;
        std::vector<Rec> recs(n_ent);
        std::vector<uint8_t> arena;
        wq_slab_entry* ent = static_cast<wq_slab_entry*>(aligned_alloc(16, n_ent * sizeof(wq_slab_entry)));
        for (size_t k = 0; k < n_ent; ++k) {
            Rec& r = recs[k];
            for (auto& x : r.uuid) x = (uint8_t)rng();
            for (auto& x : r.pos) x = (double)(int64_t)(rng() % 1000);
            r.shape = (uint32_t)rng() % 8;
            const uint32_t w = (uint32_t)rng() % 6;
            r.world = names[w];
            const uint32_t dl = round == 7 && k == 0 ? (1u << 20) : lens[rng() % (round % 3 ? 10 : 15)], fl = lens[rng() % (round % 3 ? 10 : 15)];
            if (r.shape & 1) for (uint32_t i = 0; i < dl; ++i) r.data.push_back((uint8_t)('a' + rng() % 26));
            if (r.shape & 2) for (uint32_t i = 0; i < fl; ++i) r.flex.push_back((uint8_t)rng());
            wq_slab_entry& e = ent[k];
            memset(&e, 0, sizeof e);
            memcpy(e.uuid, r.uuid, 16);
            memcpy(e.pos, r.pos, 24);
            e.world = w, e.bits = r.shape | WQ_SLAB_LIVE, e.off = arena.size();
            e.data_len = (uint32_t)r.data.size(), e.flex_len = (uint32_t)r.flex.size();
            arena.insert(arena.end(), r.data.begin(), r.data.end());
            arena.insert(arena.end(), r.flex.begin(), r.flex.end());
        }
        // rows
        const uint32_t n = 1 + (uint32_t)(rng() % 20);
        std::vector<uint32_t> off{0}, handles;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t k = round == 3 && i == 0 ? 700 : (uint32_t)(rng() % 5 ? rng() % 6 : rng() % 70);
            for (uint32_t j = 0; j < k; ++j) handles.push_back((uint32_t)(rng() % n_ent));
            off.push_back((uint32_t)handles.size());
        }
        std::vector<uint8_t> sender(16 * n), ins(n), wid_bytes(4 * n), posb(24 * n);
        std::vector<uint32_t> wid(n);
        std::vector<double> pos(3 * n);
        for (auto& x : sender) x = (uint8_t)rng();
        for (uint32_t i = 0; i < n; ++i) ins[i] = (uint8_t)(rng() % 3 ? 10 : 0), wid[i] = (uint32_t)rng() % 6;
        for (auto& x : pos) x = (double)(int64_t)(rng() % 100);
        const bool with_pos = round % 2;
        // the frames the reference builds
        std::vector<uint8_t> want;
        std::vector<uint64_t> wo{0};
        for (uint32_t i = 0; i < n; ++i) {
            std::vector<Rec> row;
            for (uint32_t j = off[i]; j < off[i + 1]; ++j) row.push_back(recs[handles[j]]);
            const auto f = ref_frame(sender.data() + 16 * i, names[wid[i]], ins[i], 1, with_pos ? pos.data() + 3 * i : nullptr, row);
            want.insert(want.end(), f.begin(), f.end());
            wo.push_back(want.size());
        }
        wq_test_recframes_in a;
        memset(&a, 0, sizeof a);
        a.src.instruction = ins.data(), a.src.replication_all = 1, a.src.sender_uuid = sender.data(), a.src.world = wid.data();
        a.src.pos = with_pos ? pos.data() : nullptr;
        a.rec.row_offsets = off.data(), a.rec.handles = handles.data(), a.rec.n_handles = handles.size();
        std::vector<uint8_t> arena_exact(arena);  // exactly sized
        a.rec.slab = wq_slab_view{ent, n_ent, arena_exact.data(), arena_exact.size()};
        a.table_bytes = reinterpret_cast<const uint8_t*>(tb.data()), a.table_off = toff.data(), a.n_table_bytes = tb.size(), a.n_worlds = 6;
        for (size_t cap : {want.size(), (size_t)0, want.size() / 2, want.size() - 1, want.size() + 40}) {
            a.scan_block = (uint32_t)(rng() % 4 ? 1 + rng() % 9 : 0);
            a.blocks = rng() % 3;
            uint8_t* buf = nullptr;  // exactly sized: the sanitizer sees the first byte past the capacity
            if (cap && posix_memalign(reinterpret_cast<void**>(&buf), 16, cap)) abort();
            if (cap) memset(buf, 0xEE, cap);
            std::vector<uint64_t> eo(n + 1, 0xDEAD);
            std::vector<uint32_t> es(n, 0xDEAD);
            uint64_t cnt[6];
            wq_test_record_frames_host(&a, n, buf, cap, eo.data(), es.data(), cnt);
            const size_t written = std::min(cap, want.size());
            bad += eo != wo || cnt[2] != want.size() || cnt[3] != written || cnt[5] != 0 || cnt[4] != (want.size() > cap);
            for (size_t i = 0; i < written; ++i) bad += buf[i] != want[i];
            for (size_t i = written; i < cap; ++i) bad += buf[i] != 0xEE;
            free(buf);
            runs++;
        }
        free(ent);
    }
    printf("record_frames host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
