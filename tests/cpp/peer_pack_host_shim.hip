// Test-only shim: runs the send buffers' arithmetic (csrc/pack_ops.hpp: the frame of a message and its
// validity rules, the record sizes' scan terms, the element that covers a byte, the window search and
// the chunk composer with its masked 16-byte loads, and the narrow stores; rows from
// csrc/budget_ops.hpp) on the CPU in the passes and tile sizes the kernels of csrc/wq_pack.hip use —
// rows, saturating scan, the ordinal space, sizes, the scan of the record sizes, the peers' and the
// elements' offsets, then the copy tile by tile in the blocks' consecutive runs: one search per tile
// (from the last tile's end inside a run), the whole-tile path, windows of kPackWindow elements, 64
// lanes of one chunk each — so the result is checked byte for byte against
// worldql_server_amd/interest.py (peer_pack_np) without a GPU (tests/test_peer_pack_cpp_mirror.py).
// The GPU instance: tests/test_gpu_peer_pack.py.
//
// With -DWQ_PEER_PACK_SHIM_MAIN the file is a program of its own: random and hostile inputs on
// exactly sized vectors, for a host build under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../worldql_server_amd/csrc/pack_ops.hpp"

extern "C" uint32_t wq_test_pack_tile() { return wq::kPackTile; }
extern "C" uint32_t wq_test_pack_chunk() { return wq::kPackChunk; }
extern "C" uint32_t wq_test_pack_window() { return wq::kPackWindow; }
extern "C" uint32_t wq_test_pack_run() { return (uint32_t)wq::kPackRun; }

// As wq_peer_pack_device. counters (nullable) = {n_in, n_complete, bytes_need, bytes_written, overflow,
// error}. Returns the number of tiles that took the whole-tile path.
extern "C" uint64_t wq_test_peer_pack_host(const uint32_t* off, const uint32_t* msgs, uint32_t n_peers, size_t n_in_,
                                           const uint8_t* frames, const uint64_t* fo, size_t n_msgs,
                                           size_t n_frame_bytes, uint32_t flags, uint8_t* out, size_t capacity,
                                           uint64_t* out_peer_bytes, uint64_t* out_elem_bytes, uint64_t* counters) {
    using namespace wq;
    const uint32_t n_in = (uint32_t)n_in_;
    const uint32_t pre_bytes = pack_prefix_bytes(flags);
    const size_t rows = (size_t)n_peers + 1;
    uint32_t error = 0;
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
    // sizes
    std::vector<uint32_t> size(n_in);
    std::vector<uint64_t> src(n_in);
    for (uint32_t q = 0; q < T; ++q) {
        const uint32_t p = bud_row_of(pre.data(), n_peers, q);
        const uint32_t j = bud_row_start(off, p, n_in) + (q - pre[p]);
        size[q] = pack_frame(fo, n_msgs, n_frame_bytes, msgs[j], &src[q], &error);
    }
    // the scan of the record sizes: n_in + 1 entries
    std::vector<uint64_t> E((size_t)n_in + 1, 0);
    uint64_t at = 0;
    for (uint64_t q = 0; q <= n_in; ++q) {
        E[q] = at;
        at += pack_rec_term(size.data(), T, pre_bytes, q);
    }
    for (size_t p = 0; p < rows; ++p) out_peer_bytes[p] = E[pre[p]];
    if (out_elem_bytes)
        for (uint32_t q = 0; q < T; ++q) out_elem_bytes[q] = E[q];
    // copy
    const uint64_t need = E[T];
    const uint64_t written = std::min<uint64_t>(need, capacity);
    uint64_t fast_tiles = 0;
    uint32_t hint = 0;
    uint64_t W[kPackWindow + 1], S[kPackWindow];
    const uint64_t blocks = capacity ? pack_blocks(capacity) : 0;
    const uint64_t per = blocks ? pack_tiles_per_block(written, blocks) : 0;
    for (uint64_t tile = 0; tile * kPackTile < written; ++tile) {
        const uint64_t c0 = tile * kPackTile;
        const uint64_t c1 = written - c0 > kPackTile ? c0 + kPackTile : written;
        // a block's first tile searches all of E; the next one starts from where the last one ended
        if (tile % per == 0) hint = pack_elem_of(E.data(), T, c0);
        const uint32_t e0 = tile % per == 0 ? hint : pack_elem_from(E.data(), T, hint, c0);
        hint = e0;
        const uint64_t r0 = E[e0], r1 = E[e0 + 1];
        uint64_t d0[kPackLanes], d1[kPackLanes];
        for (uint32_t lane = 0; lane < kPackLanes; ++lane) {
            d0[lane] = c0 + (uint64_t)lane * kPackChunk;
            d1[lane] = d0[lane] >= c1 ? d0[lane] : (c1 - d0[lane] > kPackChunk ? d0[lane] + kPackChunk : c1);
        }
        if (pack_tile_inside(r0, r1, pre_bytes, c0, c1)) {
            for (uint32_t lane = 0; lane < kPackLanes; ++lane)
                pack_store(out, d0[lane], kPackChunk, pack_load16(frames + src[e0] + (d0[lane] - r0 - pre_bytes)));
            fast_tiles++;
            continue;
        }
        PackChunk v[kPackLanes];
        for (auto& x : v) x = PackChunk{0, 0};
        for (uint64_t wb = e0;; wb += kPackWindow) {
            for (uint32_t i = 0; i <= kPackWindow; ++i) W[i] = pack_win_entry(E.data(), T, wb, i);
            for (uint32_t i = 0; i < kPackWindow; ++i) S[i] = wb + i < T ? src[wb + i] : 0ull;
            for (uint32_t lane = 0; lane < kPackLanes; ++lane) {
                const uint64_t lo = std::max(d0[lane], W[0]), hi = std::min(d1[lane], W[kPackWindow]);
                if (lo < hi) pack_compose(W, S, frames, n_frame_bytes, pre_bytes, d0[lane], lo, hi, &v[lane]);
            }
            if (W[kPackWindow] >= c1) {
                hint = (uint32_t)wb + pack_win_find(W, c1 - 1);  // the element of the tile's last byte
                break;
            }
        }
        for (uint32_t lane = 0; lane < kPackLanes; ++lane)
            if (d0[lane] < d1[lane]) pack_store(out, d0[lane], (uint32_t)(d1[lane] - d0[lane]), v[lane]);
    }
    if (counters) {
        counters[0] = T;
        counters[1] = pack_elem_of(E.data(), T, capacity);
        counters[2] = need;
        counters[3] = written;
        counters[4] = need > capacity ? 1 : 0;
        counters[5] = error;
    }
    return fast_tiles;
}

#ifdef WQ_PEER_PACK_SHIM_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <random>

namespace {

struct Case {
    std::vector<uint32_t> off, msgs;
    std::vector<uint8_t> frames;
    std::vector<uint64_t> fo;
    uint32_t n_peers;
};

struct Out {
    std::vector<uint8_t> out;  // exactly `capacity` bytes
    std::vector<uint64_t> pb, eb;
    uint64_t cnt[6];
};

// d_out must be 16-byte aligned and is sized exactly: an aligned allocation of `capacity` bytes, so
// the address sanitizer sees a store past bytes_written when it also passes the capacity.
struct AlignedBytes {
    uint8_t* p = nullptr;
    size_t n = 0;
    explicit AlignedBytes(size_t n_) : n(n_) {
        if (n && posix_memalign(reinterpret_cast<void**>(&p), 16, n)) abort();
        for (size_t i = 0; i < n; ++i) p[i] = 0xEE;
    }
    ~AlignedBytes() { free(p); }
};

Out run(const Case& c, uint32_t flags, size_t capacity, bool with_elem) {
    AlignedBytes buf(capacity);
    Out o{{}, std::vector<uint64_t>((size_t)c.n_peers + 1, 0xDEADBEEFull), std::vector<uint64_t>(c.msgs.size(), 0xDEADBEEFull), {}};
    wq_test_peer_pack_host(c.off.data(), c.msgs.data(), c.n_peers, c.msgs.size(), c.frames.data(), c.fo.data(),
                           c.fo.size() - 1, c.frames.size(), flags, buf.p, capacity, o.pb.data(),
                           with_elem ? o.eb.data() : nullptr, o.cnt);
    o.out.assign(buf.p, buf.p + capacity);
    return o;
}

// The contract restated: walk the rows up to n_in elements, append record after record.
struct Want {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> pb, eb;
    uint32_t error = 0;
};

Want restate(const Case& c, uint32_t flags) {
    Want w;
    const size_t n_in = c.msgs.size(), n_msgs = c.fo.size() - 1;
    size_t walked = 0;
    for (uint32_t p = 0; p < c.n_peers; ++p) {
        const size_t a = std::min<size_t>(c.off[p], n_in), b = std::max(a, std::min<size_t>(c.off[p + 1], n_in));
        if (c.off[p] > c.off[p + 1] || c.off[p + 1] > n_in) w.error |= 1;
        const size_t n = std::min(b - a, n_in - walked);
        if (n != b - a) w.error |= 1;
        walked += n;
        w.pb.push_back(w.bytes.size());
        for (size_t j = a; j < a + n; ++j) {
            const uint32_t m = c.msgs[j];
            uint64_t s = 0, e = 0;
            if (m >= n_msgs) {
                w.error |= 2;
            } else if (c.fo[m] > c.fo[m + 1] || c.fo[m + 1] > c.frames.size() || c.fo[m + 1] - c.fo[m] >= (1ull << 32)) {
                w.error |= 4;
            } else {
                s = c.fo[m], e = c.fo[m + 1];
            }
            w.eb.push_back(w.bytes.size());
            if (flags & 1u)
                for (int i = 0; i < 4; ++i) w.bytes.push_back((uint8_t)((e - s) >> (8 * i)));
            w.bytes.insert(w.bytes.end(), c.frames.begin() + s, c.frames.begin() + e);
        }
    }
    w.pb.push_back(w.bytes.size());
    return w;
}

int check(const Case& c, uint32_t flags, size_t capacity, const Out& o, const Want& w, bool with_elem) {
    const uint64_t need = w.bytes.size(), written = std::min<uint64_t>(need, capacity);
    int bad = o.pb != w.pb;
    for (size_t q = 0; q < c.msgs.size(); ++q)
        bad += o.eb[q] != (with_elem && q < w.eb.size() ? w.eb[q] : 0xDEADBEEFull);
    for (uint64_t i = 0; i < written; ++i) bad += o.out[i] != w.bytes[i];
    for (uint64_t i = written; i < capacity; ++i) bad += o.out[i] != 0xEE;
    uint64_t complete = 0;
    for (size_t q = 0; q < w.eb.size(); ++q) complete += (q + 1 < w.eb.size() ? w.eb[q + 1] : need) <= capacity;
    bad += o.cnt[0] != w.eb.size() || o.cnt[1] != complete || o.cnt[2] != need || o.cnt[3] != written;
    bad += o.cnt[4] != (need > capacity) || o.cnt[5] != w.error;
    return bad;
}

}  // namespace

int main() {
    std::mt19937_64 rng(31);
    const uint32_t sizes[] = {0, 0, 1, 1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099, 2500};
    const uint32_t lens[] = {0, 0, 1, 2, 3, 7, 40, 70, 130, 300};
    int bad = 0, runs = 0;
    for (int round = 0; round < 60; ++round) {
        Case c;
        c.n_peers = round % 12 == 0 ? 0 : 1 + rng() % 24;
        const size_t n_msgs = round % 9 == 4 ? 0 : 1 + rng() % 60;
        c.fo.push_back(0);
        const bool tiny = round % 4 == 1;  // runs of empty and one-byte frames
        for (size_t i = 0; i < n_msgs; ++i) {
            const uint32_t s = round == 7 && i == 1 ? (1u << 20) + 5 : tiny ? (uint32_t)(rng() % 3 == 0) : sizes[rng() % 23];
            for (uint32_t k = 0; k < s; ++k) c.frames.push_back((uint8_t)rng());
            c.fo.push_back(c.frames.size());
        }
        c.off.push_back(0);
        for (uint32_t p = 0; p < c.n_peers; ++p) {
            const uint32_t n = lens[rng() % 10];
            for (uint32_t i = 0; i < n; ++i)
                c.msgs.push_back(rng() % 40 == 0 ? 0xFFFFFFFFu - (uint32_t)(rng() % 2) : (uint32_t)(rng() % (n_msgs + 1)));
            c.off.push_back((uint32_t)c.msgs.size());
        }
        std::vector<Case> variants{c};
        if (n_msgs > 3) {  // frame offsets that descend and reach past the end
            Case f = c;
            std::swap(f.fo[1], f.fo[2]);
            f.fo[n_msgs] = f.frames.size() + 9;
            variants.push_back(f);
            f = c;
            f.fo[n_msgs / 2] = 0xFFFFFFFFFFFFFFFFull;
            variants.push_back(f);
        }
        if (c.n_peers >= 2) {  // hostile rows
            const uint32_t full = (uint32_t)c.msgs.size();
            Case h = c;
            std::reverse(h.off.begin(), h.off.end());
            variants.push_back(h);
            h = c;
            h.off[1 + rng() % (c.n_peers - 1)] = full ? (uint32_t)(rng() % full) : 0u;
            variants.push_back(h);
            h = c;
            h.off.assign(c.n_peers + 1, 0xFFFFFFFFu);
            variants.push_back(h);
            for (auto& x : h.off) x = (uint32_t)rng() % (2 * full + 2);
            variants.push_back(h);
            h = c;
            h.msgs.resize(full ? rng() % full : 0);  // rows reach past n_in
            variants.push_back(h);
        }
        for (const Case& v : variants) {
            for (uint32_t flags = 0; flags < 2; ++flags) {
                const Want w = restate(v, flags);
                const uint64_t need = w.bytes.size();
                std::vector<size_t> caps{(size_t)need, 0};
                if (need) caps.push_back(need - 1), caps.push_back(rng() % need);
                if (need > 20) caps.push_back(need - 17), caps.push_back((need / 2) & ~(size_t)15);
                if (v.n_peers) caps.push_back(w.pb[rng() % (v.n_peers + 1)]);
                caps.push_back(need + 33);
                for (size_t cap : caps) {
                    const bool with_elem = rng() % 4 != 0;
                    bad += check(v, flags, cap, run(v, flags, cap, with_elem), w, with_elem);
                    runs++;
                }
            }
        }
    }
    printf("peer_pack host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
