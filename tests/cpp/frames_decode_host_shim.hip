// Test-only shim: runs the ingest decoder's arithmetic (csrc/decode_ops.hpp: the bounded reader, the
// verifier walk, UTF-8 by chunks, parse_uuid, the sanitizer stream, the world and sender lookups) on the
// CPU in the passes the kernels of csrc/wq_decode.hip use — the walk frame by frame with the work list,
// the strings pass in the grid's order (blocks striding over the entries, kDecSlices blocks sharing a
// string tile by tile, kDecBlock lanes of kDecChunk bytes), the finish with its per-block sums — so the
// result is checked byte for byte against worldql_server_amd/ingest.py (decode_frames_np) without a GPU
// (tests/test_frames_decode_cpp_mirror.py). The GPU instance: tests/test_gpu_frames_decode.py.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../worldql_server_amd/csrc/decode_ops.hpp"

extern "C" uint32_t wq_test_decode_lane() { return wq::kDecLane; }
extern "C" uint32_t wq_test_decode_chunk() { return wq::kDecChunk; }
extern "C" uint32_t wq_test_decode_tile() { return wq::kDecTile; }
extern "C" uint32_t wq_test_decode_list_default() { return wq::kDecListDefault; }

// The arguments of wq_frames_decode_device with the tables of wq_frames_set_worlds and
// wq_ingest_set_peers, all host memory. list_cap < 0: the default.
struct wq_test_decode_in {
    const uint8_t* frames;
    const uint64_t* offsets;
    uint64_t n_frames, n_frame_bytes;
    const uint8_t* world_bytes;
    const uint32_t* world_off;  // [n_worlds + 1], from 0
    const uint8_t* peer_uuids;
    const uint32_t* peer_ids;
    uint32_t n_worlds, n_peers;
    int64_t list_cap;
};

// As wq_frames_decode_device. stats (nullable) = {entries the list took, chunks the strings pass
// checked}. Returns 0, or -1 for a sender uuid that occurs twice (wq_ingest_set_peers refuses it).
extern "C" int wq_test_frames_decode_host(const wq_test_decode_in* a, const wq_ingest_out* out,
                                          wq_ingest_counters* counters, uint64_t* stats) {
    using namespace wq;
    std::vector<uint64_t> whash, phi, plo;
    std::vector<uint32_t> wid, pid;
    if (a->n_worlds) dec_world_index(a->world_bytes, a->world_off, a->n_worlds, &whash, &wid);
    if (a->n_peers && !dec_peer_index(a->peer_uuids, a->peer_ids, a->n_peers, &phi, &plo, &pid)) return -1;
    DecTables t;
    t.world_bytes = a->world_bytes, t.world_off = a->world_off, t.world_hash = whash.data(), t.world_id = wid.data();
    t.peer_hi = phi.data(), t.peer_lo = plo.data(), t.peer_id = pid.data();
    t.n_worlds = a->n_worlds, t.n_peers = a->n_peers;

    const uint64_t n = a->n_frames;
    const uint32_t cap = a->list_cap < 0 ? kDecListDefault : (uint32_t)a->list_cap;
    std::vector<DecEntry> entries(cap);  // exactly the capacity: a slot too many is a heap overflow
    uint32_t appended = 0;
    DecList list{entries.data(), &appended, cap};
    std::vector<uint32_t> word(n);
    wq_ingest_counters c;
    memset(&c, 0, sizeof(c));
    // walk
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t err = 0;
        word[i] = dec_walk(a->frames, a->offsets, i, n, a->n_frame_bytes, list, t, *out, &err);
        c.error |= err;
    }
    // strings
    uint64_t chunks = 0;
    const uint32_t cnt = std::min(appended, cap);
    const uint32_t gx = std::min(cap, kDecListBlocks);
    for (uint32_t bx = 0; bx < gx; ++bx)
        for (uint32_t by = 0; by < kDecSlices; ++by)
            for (uint32_t k = bx; k < cnt; k += gx) {
                const DecEntry e = entries[k];
                for (uint64_t t0 = (uint64_t)by * kDecTile; t0 < e.len; t0 += (uint64_t)kDecSlices * kDecTile)
                    for (uint32_t lane = 0; lane < kDecBlock; ++lane) {
                        const uint64_t c0 = t0 + (uint64_t)lane * kDecChunk;
                        if (c0 >= e.len) break;
                        ++chunks;
                        if (!dec_entry_chunk_ok(a->frames, e, c0)) word[e.frame] |= kDecTentBad;
                    }
            }
    // finish
    uint64_t* const sums[6] = {&c.n_ok, &c.n_invalid, &c.n_missing, &c.n_bad_uuid, &c.n_world_unresolved,
                               &c.n_sender_unknown};
    for (uint64_t b0 = 0; b0 < n; b0 += kDecBlock) {
        uint32_t block[6] = {0, 0, 0, 0, 0, 0};
        for (uint64_t i = b0; i < std::min<uint64_t>(n, b0 + kDecBlock); ++i) dec_count(dec_finish(word[i], i, *out), block);
        for (int k = 0; k < 6; ++k) *sums[k] += block[k];
    }
    c.n_frames = n;
    if (counters) *counters = c;
    if (stats) stats[0] = cnt, stats[1] = chunks;
    return 0;
}

// The stand-alone form: the program below runs a corpus file through the shim on exactly sized heap
// arrays, for a host build under -fsanitize=address,undefined together with csrc/wq_codec.cpp. It checks,
// against wq_decode_messages, the struct of every frame of the corpus at every alignment residue mod 16
// and work-list capacity 0, 1 and the default, of every strict truncation of the corpus' first frames
// and of single-byte corruptions of them, each frame alone in a heap block of exactly its size.
//   file: u64 n, u64 n_bytes, u64 offsets[n + 1], u8 data[n_bytes]
#ifdef WQ_DECODE_SHIM_MAIN
#include <stdio.h>
#include <stdlib.h>

namespace {

struct Outs {
    std::vector<wq_decoded_msg> msg;
    std::vector<double> pos;
    std::vector<uint32_t> world, sender, flex;
    std::vector<uint8_t> repl, ins, uuid, flags;
    wq_ingest_out o;
    explicit Outs(size_t n) : msg(n), pos(3 * n), world(n), sender(n), flex(2 * n), repl(n), ins(n), uuid(16 * n), flags(n) {
        o.msg = msg.data(), o.pos = pos.data(), o.world = world.data(), o.sender = sender.data();
        o.repl = repl.data(), o.instruction = ins.data(), o.sender_uuid = uuid.data(), o.flex_range = flex.data();
        o.flags = flags.data();
    }
};

int run_one(const uint8_t* data, const uint64_t* off, size_t n, size_t nbytes, int64_t cap, const wq_decoded_msg* want) {
    static const uint8_t names[] = "worldw00chat_fs_server_1";
    static const uint32_t noff[] = {0, 5, 8, 24};
    wq_test_decode_in a;
    memset(&a, 0, sizeof(a));
    a.frames = data, a.offsets = off, a.n_frames = n, a.n_frame_bytes = nbytes;
    a.world_bytes = names, a.world_off = noff, a.n_worlds = 3, a.list_cap = cap;
    Outs o(n);
    wq_ingest_counters c;
    if (wq_test_frames_decode_host(&a, &o.o, &c, nullptr)) return 1;
    int bad = n && memcmp(o.msg.data(), want, n * sizeof(wq_decoded_msg)) != 0;
    bad += c.n_ok + c.n_invalid + c.n_missing + c.n_bad_uuid != n;
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t hdr[2];
    if (fread(hdr, 8, 2, f) != 2) return 2;
    const size_t n = hdr[0], nbytes = hdr[1];
    std::vector<uint64_t> off(n + 1);
    std::vector<uint8_t> data(nbytes);
    if (fread(off.data(), 8, n + 1, f) != n + 1 || fread(data.data(), 1, nbytes, f) != nbytes) return 2;
    fclose(f);
    std::vector<wq_decoded_msg> want(n);
    if (wq_decode_messages(data.data(), off.data(), n, want.data(), 1)) return 2;
    int bad = 0, runs = 0;
    // the corpus at every residue mod 16, on a heap block that ends with its last byte
    for (size_t shift = 0; shift < 16; ++shift)
        for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)-1}) {
            uint8_t* block = static_cast<uint8_t*>(malloc(nbytes + shift));
            memcpy(block + shift, data.data(), nbytes);
            bad += run_one(block + shift, off.data(), n, nbytes, cap, want.data());
            free(block);
            ++runs;
        }
    // each of the first frames alone: whole, every strict truncation, one byte changed to two values
    for (size_t i = 0; i < std::min<size_t>(n, 24); ++i) {
        const size_t len = off[i + 1] - off[i];
        const uint8_t* src = data.data() + off[i];
        auto one = [&](const uint8_t* bytes, size_t m) {
            uint8_t* block = static_cast<uint8_t*>(malloc(m ? m : 1));
            if (m) memcpy(block, bytes, m);
            const uint64_t o2[2] = {0, m};
            wq_decoded_msg w;
            wq_decode_messages(block, o2, 1, &w, 1);
            bad += run_one(block, o2, 1, m, (int64_t)(runs % 3) - 1, &w);
            free(block);
            ++runs;
        };
        for (size_t m = 0; m <= len; ++m) one(src, m);
        if (len <= 600) {
            std::vector<uint8_t> v(src, src + len);
            for (size_t k = 0; k < len; ++k)
                for (uint8_t val : {(uint8_t)0xFF, (uint8_t)(v[k] ^ 0x04)}) {
                    const uint8_t keep = v[k];
                    v[k] = val;
                    one(v.data(), len);
                    v[k] = keep;
                }
        }
    }
    printf("frames_decode host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
