// Test-only shim: runs the frame builder's arithmetic (csrc/frame_ops.hpp: a message's fields under the
// validity rules, the builder's push sequence replayed on counters, the size, the payload spans and
// the chunk sink with its masked 16-byte loads; tiles, window search and stores from
// csrc/pack_ops.hpp) on the CPU in the passes and tile sizes the kernels of csrc/wq_frames.hip use —
// sizes, the scan into the frame offsets, then the copy tile by tile in the blocks' consecutive runs:
// one search per tile (from the last tile's end inside a run), the whole-tile path, windows of
// kPackWindow frames, 64 lanes of one chunk each — so the result is checked byte for byte against
// worldql_server_amd/frames.py (build_frames_np) without a GPU (tests/test_frames_build_cpp_mirror.py).
// The GPU instance: tests/test_gpu_frames_build.py.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../worldql_server_amd/csrc/frame_ops.hpp"

extern "C" uint32_t wq_test_frames_tile() { return wq::kPackTile; }
extern "C" uint64_t wq_test_frames_max() { return wq::kFrameMax; }

// The arguments of wq_frames_build_device with the table of wq_frames_set_worlds, all host memory.
struct wq_test_frames_in {
    const uint8_t* instruction;
    const uint8_t* replication;
    const uint8_t* sender_uuid;
    const uint8_t* world;
    const uint8_t* pos;
    const uint8_t* param;
    const uint8_t* param_offsets;
    const uint8_t* flex;
    const uint8_t* flex_offsets;
    const uint8_t* msg_flags;
    const uint8_t* world_bytes;
    const uint32_t* world_off;
    uint64_t n, n_param_bytes, n_flex_bytes, n_world_bytes;
    uint32_t n_worlds;
    uint8_t instruction_all, replication_all;
};

// As wq_frames_build_device. counters (nullable) = {n_frames, n_complete, bytes_need, bytes_written,
// overflow, error}. Returns the number of tiles that took the whole-tile path.
extern "C" uint64_t wq_test_frames_build_host(const wq_test_frames_in* a, uint8_t* out, size_t capacity,
                                              uint64_t* out_offsets, uint32_t* out_size, uint64_t* counters) {
    using namespace wq;
    FrameSrc s;
    s.instruction = a->instruction, s.replication = a->replication, s.sender_uuid = a->sender_uuid;
    s.world = a->world, s.pos = a->pos, s.param = a->param, s.param_offsets = a->param_offsets;
    s.flex = a->flex, s.flex_offsets = a->flex_offsets, s.msg_flags = a->msg_flags;
    // the table as the handle keeps it: zero slack on both sides of the names
    std::vector<uint8_t> table(a->n_world_bytes + 2 * kFrWorldSlack, 0);
    if (a->n_world_bytes) memcpy(table.data() + kFrWorldSlack, a->world_bytes, a->n_world_bytes);
    s.world_bytes = table.data() + kFrWorldSlack, s.world_off = a->world_off, s.world_slack = kFrWorldSlack;
    s.n = a->n, s.n_param_bytes = a->param_offsets ? a->n_param_bytes : 0;
    s.n_flex_bytes = a->flex_offsets ? a->n_flex_bytes : 0, s.n_world_bytes = a->n_world_bytes;
    s.n_worlds = a->n_worlds, s.instruction_all = a->instruction_all, s.replication_all = a->replication_all;
    const uint32_t T = (uint32_t)s.n;
    uint32_t error = 0;
    // sizes
    std::vector<uint32_t> size(T);
    for (uint32_t i = 0; i < T; ++i) {
        const FrameMsg m = frame_msg(s, i);
        error |= m.err;
        size[i] = frame_size(m, &error);
        if (out_size) out_size[i] = size[i];
    }
    // the scan: n + 1 entries, into the caller's offsets
    uint64_t at = 0;
    for (uint64_t q = 0; q <= T; ++q) {
        out_offsets[q] = at;
        at += frame_term(size.data(), T, q);
    }
    const uint64_t* E = out_offsets;
    // copy
    const uint64_t need = E[T];
    const uint64_t written = std::min<uint64_t>(need, capacity);
    uint64_t fast_tiles = 0;
    uint32_t hint = 0;
    uint64_t W[kPackWindow + 1];
    const uint64_t blocks = capacity && T ? pack_blocks(capacity) : 0;
    const uint64_t per = blocks ? pack_tiles_per_block(written, blocks) : 1;
    for (uint64_t tile = 0; blocks && tile * kPackTile < written; ++tile) {
        const uint64_t c0 = tile * kPackTile;
        const uint64_t c1 = written - c0 > kPackTile ? c0 + kPackTile : written;
        const uint32_t e0 = tile % per == 0 ? pack_elem_of(E, T, c0) : pack_elem_from(E, T, hint, c0);
        hint = e0;
        const uint64_t r0 = E[e0], r1 = E[e0 + 1];
        uint64_t d0[kPackLanes], d1[kPackLanes];
        for (uint32_t lane = 0; lane < kPackLanes; ++lane) {
            d0[lane] = c0 + (uint64_t)lane * kPackChunk;
            d1[lane] = d0[lane] >= c1 ? d0[lane] : (c1 - d0[lane] > kPackChunk ? d0[lane] + kPackChunk : c1);
        }
        if (c1 - c0 == kPackTile && r1 - r0 >= kPackTile) {
            const uint8_t* from;
            if (frame_tile_inside(s, frame_msg(s, e0), r0, r1, c0, c1, &from)) {
                for (uint32_t lane = 0; lane < kPackLanes; ++lane)
                    pack_store(out, d0[lane], kPackChunk, pack_load16(from + (uint64_t)lane * kPackChunk));
                fast_tiles++;
                continue;
            }
        }
        PackChunk v[kPackLanes];
        for (auto& x : v) x = PackChunk{0, 0};
        for (uint64_t wb = e0;; wb += kPackWindow) {
            for (uint32_t i = 0; i <= kPackWindow; ++i) W[i] = pack_win_entry(E, T, wb, i);
            for (uint32_t lane = 0; lane < kPackLanes; ++lane) {
                const uint64_t lo = std::max(d0[lane], W[0]), hi = std::min(d1[lane], W[kPackWindow]);
                if (lo < hi) frame_compose(W, wb, s, d0[lane], lo, hi, &v[lane]);
            }
            if (W[kPackWindow] >= c1) {
                hint = (uint32_t)wb + pack_win_find(W, c1 - 1);  // the frame of the tile's last byte
                break;
            }
        }
        for (uint32_t lane = 0; lane < kPackLanes; ++lane)
            if (d0[lane] < d1[lane]) pack_store(out, d0[lane], (uint32_t)(d1[lane] - d0[lane]), v[lane]);
    }
    if (counters) {
        counters[0] = T;
        counters[1] = pack_elem_of(E, T, capacity);
        counters[2] = need;
        counters[3] = written;
        counters[4] = need > capacity ? 1 : 0;
        counters[5] = error;
    }
    return fast_tiles;
}

// With -DWQ_FRAMES_SHIM_MAIN the file is a program of its own: random and hostile inputs on exactly
// sized heap arrays, for a host build under -fsanitize=address,undefined. It checks what needs no
// second serializer: every capacity's output is a prefix of the whole one, nothing is written behind
// bytes_written, and offsets, sizes and counters do not depend on the capacity.
#ifdef WQ_FRAMES_SHIM_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>

namespace {

struct AlignedBytes {
    uint8_t* p = nullptr;
    size_t n = 0;
    explicit AlignedBytes(size_t n_) : n(n_) {
        if (n && posix_memalign(reinterpret_cast<void**>(&p), 16, n)) abort();
        for (size_t i = 0; i < n; ++i) p[i] = 0xEE;
    }
    ~AlignedBytes() { free(p); }
};

template <typename T>
const uint8_t* raw(const std::vector<T>& v) {
    return reinterpret_cast<const uint8_t*>(v.data());
}

}  // namespace

int main() {
    std::mt19937_64 rng(41);
    const uint32_t lens[] = {0, 0, 1, 2, 3, 5, 15, 16, 17, 31, 33, 64, 100, 1023, 1024, 1025, 2500, 5000};
    int bad = 0, runs = 0;
    for (int round = 0; round < 80; ++round) {
        const size_t n = round % 10 == 3 ? 0 : 1 + rng() % 70;
        const uint32_t n_worlds = round % 7 == 2 ? 0 : 1 + rng() % 6;
        std::vector<uint8_t> wbytes;
        std::vector<uint32_t> woff{0};
        for (uint32_t w = 0; w < n_worlds; ++w) {
            for (uint32_t k = rng() % 12; k; --k) wbytes.push_back((uint8_t)('a' + rng() % 26));
            woff.push_back((uint32_t)wbytes.size());
        }
        std::vector<uint8_t> ins(n), rep(n), flags(n), uuid(16 * n), param, flex;
        std::vector<uint32_t> world(n);
        std::vector<double> pos(3 * n);
        std::vector<uint64_t> po{0}, fo{0};
        for (size_t i = 0; i < n; ++i) {
            ins[i] = (uint8_t)(rng() % 3 ? 7 : rng()), rep[i] = (uint8_t)(rng() % 3), flags[i] = (uint8_t)rng();
            world[i] = rng() % 9 == 0 ? (uint32_t)rng() : (uint32_t)(rng() % (n_worlds + 1));
            for (int k = 0; k < 16; ++k) uuid[16 * i + k] = (uint8_t)rng();
            for (int k = 0; k < 3; ++k) pos[3 * i + k] = (double)(int64_t)rng() / 1e6;
            for (uint32_t k = round == 5 && i == 1 ? (1u << 20) + 7 : lens[rng() % 18]; k; --k) param.push_back((uint8_t)rng());
            po.push_back(param.size());
            for (uint32_t k = round == 6 && i == 2 ? (1u << 20) + 9 : lens[rng() % 18]; k; --k) flex.push_back((uint8_t)rng());
            fo.push_back(flex.size());
        }
        if (round % 4 == 1 && n > 3) {  // hostile offsets: descending, past the end, far
            std::swap(po[1], po[2]);
            fo[n] = flex.size() + 5;
            fo[n / 2] = 0xFFFFFFFFFFFFFFFFull;
            po[n - 1] = (1ull << 32) + 3;
        }
        const int combo = round % 64;  // which nullable inputs are given
        wq_test_frames_in a;
        memset(&a, 0, sizeof(a));
        a.instruction = (combo & 1) ? ins.data() : nullptr, a.instruction_all = 7;
        a.replication = (combo & 2) ? rep.data() : nullptr, a.replication_all = 1;
        a.sender_uuid = uuid.data(), a.world = raw(world);
        a.pos = (combo & 4) ? raw(pos) : nullptr;
        static const uint8_t none = 0;
        if (combo & 8) a.param = param.empty() ? &none : param.data(), a.param_offsets = raw(po), a.n_param_bytes = param.size();
        if (combo & 16) a.flex = flex.empty() ? &none : flex.data(), a.flex_offsets = raw(fo), a.n_flex_bytes = flex.size();
        a.msg_flags = (combo & 32) ? flags.data() : nullptr;
        a.world_bytes = wbytes.data(), a.world_off = n_worlds ? woff.data() : nullptr;
        a.n = n, a.n_world_bytes = wbytes.size(), a.n_worlds = n_worlds;

        std::vector<uint64_t> off0(n + 1), cnt0(6);
        std::vector<uint32_t> size0(n);
        wq_test_frames_build_host(&a, nullptr, 0, off0.data(), size0.data(), cnt0.data());
        const size_t need = off0[n];
        AlignedBytes whole(need);
        std::vector<uint64_t> off(n + 1), cnt(6);
        std::vector<uint32_t> size(n);
        wq_test_frames_build_host(&a, whole.p, need, off.data(), size.data(), cnt.data());
        bad += off != off0 || size != size0 || cnt[2] != need || cnt[3] != need || cnt[4] != 0 || cnt[5] != cnt0[5];
        runs++;
        std::vector<size_t> caps{1, need / 2, need ? need - 1 : 0, need + 33};
        for (int k = 0; k < 4; ++k) caps.push_back(need ? rng() % need : 0);
        for (size_t cap : caps) {
            if (cap == 0) continue;
            AlignedBytes cut(cap);
            wq_test_frames_build_host(&a, cut.p, cap, off.data(), nullptr, cnt.data());
            const size_t written = std::min(cap, need);
            bad += off != off0 || cnt[3] != written || cnt[4] != (need > cap) || cnt[5] != cnt0[5];
            bad += written && memcmp(cut.p, whole.p, written) != 0;
            for (size_t i = written; i < cap; ++i) bad += cut.p[i] != 0xEE;
            runs++;
        }
    }
    printf("frames_build host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
