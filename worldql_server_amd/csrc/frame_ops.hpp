// frame_ops.hpp — the arithmetic of the frame builder (wq_frames.hip, wq_frames_build_device): the
// fields of a flat message under the validity rules, the builder's push sequence replayed on counters
// (frame_walk) and the sinks that turn the replay into a size, into the spans of the two payloads or
// into the bytes of one 16-byte destination chunk. __host__ __device__, so
// tests/cpp/frames_build_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/frames.py (build_frames_np).
//
// The bytes are defined by wq_codec.cpp: serialize_one driving Builder. The buffer fills from the back,
// so every position is a "revloc", the bytes used once a piece has been pushed. frame_walk is that
// push sequence for a message without records and entities with `used` as its only state: the same
// align, string, bytes, offsets, slot, end_table and finish steps in the same order. Each step tells
// the sink what it pushed: a little-endian value of up to four bytes, or a run of bytes of some kind
// (parameter, uuid text, world name, flex, position). Everything the sink is not told about is zero:
// alignment, the strings' NULs and the vtable's absent slots. A piece that ends at revloc r in a frame
// of `size` bytes starts at byte size - r of the frame. A flat frame has one table and one vtable, so
// the builder's vtable dedupe never fires and is not restated.
//
// The copy runs over the output bytes like the send buffers' (pack_ops.hpp, whose tiles, chunks,
// window search, masks and stores it shares): E is the frame offsets, an element is a frame.
#pragma once

#include "pack_ops.hpp"

namespace wq {

constexpr uint64_t kFrameMax = 1ull << 30;  // wq_codec.cpp kMaxFrame: the host returns WQ_SER_TOO_LARGE above
constexpr uint32_t kFrErrWorld = 1u;        // error bit 0: a world id >= n_worlds
constexpr uint32_t kFrErrParam = 2u;        // bit 1: a parameter range descends, passes the end or spans 2^32
constexpr uint32_t kFrErrFlex = 4u;         // bit 2: the same for flex
constexpr uint32_t kFrErrLarge = 8u;        // bit 3: a frame above kFrameMax
constexpr uint32_t kFrHasPos = 1u, kFrHasParam = 2u, kFrHasFlex = 4u;  // msg_flags bits
constexpr uint32_t kFrUuidText = 36;
constexpr uint32_t kFrWorldSlack = 16;       // zero bytes the handle keeps on both sides of the world table

// Message vtable slots (wq_codec.cpp S_*)
enum : uint32_t { kFrInstr = 4, kFrParam = 6, kFrSender = 8, kFrWorld = 10, kFrRepl = 12, kFrRecords = 14,
                  kFrEntities = 16, kFrPos = 18, kFrFlex = 20 };

// Kinds of byte runs the walk pushes.
enum : uint32_t { kFrRunParam = 0, kFrRunUuid = 1, kFrRunWorld = 2, kFrRunFlex = 3, kFrRunPos = 4 };

// wq_frames_src plus the handle's world table. Every pointer may have any alignment.
struct FrameSrc {
    const uint8_t* instruction;
    const uint8_t* replication;
    const uint8_t* sender_uuid;
    const uint8_t* world;  // u32[n]
    const uint8_t* pos;    // f64[3 n]
    const uint8_t* param;
    const uint8_t* param_offsets;  // u64[n + 1]
    const uint8_t* flex;
    const uint8_t* flex_offsets;  // u64[n + 1]
    const uint8_t* msg_flags;
    const uint8_t* world_bytes;   // the table's names back to back
    const uint32_t* world_off;    // [n_worlds + 1]
    uint64_t n, n_param_bytes, n_flex_bytes, n_world_bytes;
    uint32_t n_worlds;
    uint32_t world_slack;  // readable bytes before world_bytes and behind world_bytes + n_world_bytes: 0 or kFrWorldSlack
    uint8_t instruction_all, replication_all;
};

// The fields of one message after the validity rules.
struct FrameMsg {
    uint64_t param_src, flex_src, world_src;  // where the bytes start in their arrays
    uint32_t param_len, flex_len, world_len;
    uint32_t has;  // kFrHas*
    uint32_t err;  // kFrErr* of this message, kFrErrLarge excepted
    uint8_t instruction, replication;
};

template <typename T>
__host__ __device__ __forceinline__ T frame_ld(const uint8_t* p, uint64_t i) {
    T v;
    __builtin_memcpy(&v, p + i * sizeof(T), sizeof(T));
    return v;
}

// A payload range [off[i], off[i + 1]) of an array of n_bytes: false, with the range taken as empty,
// when it descends, reaches past n_bytes or spans 2^32 bytes or more (pack_frame's rules).
__host__ __device__ __forceinline__ bool frame_range(const uint8_t* off, uint64_t i, uint64_t n_bytes, uint64_t* src,
                                                     uint32_t* len) {
    const uint64_t a = frame_ld<uint64_t>(off, i), b = frame_ld<uint64_t>(off, i + 1);
    *src = 0;
    *len = 0;
    if (a > b || b > n_bytes || b - a >= (1ull << 32)) return false;
    *src = a;
    *len = (uint32_t)(b - a);
    return true;
}

// Message i (i < s.n). A field is there when its array is given and, with msg_flags, its bit is set.
__host__ __device__ __forceinline__ FrameMsg frame_msg(const FrameSrc& s, uint64_t i) {
    FrameMsg m;
    m.err = 0;
    m.instruction = s.instruction ? s.instruction[i] : s.instruction_all;
    m.replication = s.replication ? s.replication[i] : s.replication_all;
    const uint32_t given = (s.pos ? kFrHasPos : 0u) | (s.param_offsets ? kFrHasParam : 0u) |
                           (s.flex_offsets ? kFrHasFlex : 0u);
    m.has = s.msg_flags ? (uint32_t)s.msg_flags[i] & given : given;
    const uint32_t w = frame_ld<uint32_t>(s.world, i);
    m.world_src = 0;
    m.world_len = 0;
    if (w < s.n_worlds) {
        m.world_src = s.world_off[w];
        m.world_len = s.world_off[w + 1] - s.world_off[w];
    } else {
        m.err |= kFrErrWorld;
    }
    m.param_src = m.flex_src = 0;
    m.param_len = m.flex_len = 0;
    if ((m.has & kFrHasParam) && !frame_range(s.param_offsets, i, s.n_param_bytes, &m.param_src, &m.param_len))
        m.err |= kFrErrParam;
    if ((m.has & kFrHasFlex) && !frame_range(s.flex_offsets, i, s.n_flex_bytes, &m.flex_src, &m.flex_len))
        m.err |= kFrErrFlex;
    return m;
}

// The builder on counters: `used` and min_align, and what each push tells the sink.
template <typename Sink>
struct FrameBuilder {
    Sink& k;
    uint64_t used = 0;
    uint64_t min_align = 0;
    __host__ __device__ explicit FrameBuilder(Sink& sink) : k(sink) {}

    __host__ __device__ __forceinline__ void align(uint64_t len, uint64_t a) {
        min_align = min_align > a ? min_align : a;
        used += (~(used + len) + 1) & (a - 1);
    }
    __host__ __device__ __forceinline__ uint64_t push_u8(uint8_t v) {
        used += 1;
        k.value(used, 1, v);
        return used;
    }
    __host__ __device__ __forceinline__ uint64_t push_u32(uint32_t v) {
        align(4, 4);
        used += 4;
        k.value(used, 4, v);
        return used;
    }
    __host__ __device__ __forceinline__ uint64_t push_off(uint64_t target) {
        align(4, 4);
        const uint64_t slot = used + 4;
        used += 4;
        k.value(used, 4, (uint32_t)(slot - target));
        return used;
    }
    __host__ __device__ __forceinline__ uint64_t push_vec3() {  // size 24, alignment 1
        used += 24;
        k.run(kFrRunPos, used, 24);
        return used;
    }
    __host__ __device__ __forceinline__ uint64_t string(uint32_t kind, uint32_t n) {  // NUL, bytes, length
        align((uint64_t)n + 1, 4);
        used += 1;
        used += n;
        if (n) k.run(kind, used, n);
        return push_u32(n);
    }
    __host__ __device__ __forceinline__ uint64_t bytes(uint32_t kind, uint32_t n) {
        align(n, 4);
        used += n;
        if (n) k.run(kind, used, n);
        return push_u32(n);
    }
    __host__ __device__ __forceinline__ uint64_t offsets0() {  // an empty vector of offsets
        align(0, 4);
        return push_u32(0);
    }
};

// serialize_one for a flat message: returns the frame's size, which may exceed kFrameMax.
template <typename Sink>
__host__ __device__ __forceinline__ uint64_t frame_walk(const FrameMsg& m, Sink& sink) {
    FrameBuilder<Sink> b(sink);
    const bool has_param = m.has & kFrHasParam, has_flex = m.has & kFrHasFlex, has_pos = m.has & kFrHasPos;
    const uint64_t param = has_param ? b.string(kFrRunParam, m.param_len) : 0;
    const uint64_t sender = b.string(kFrRunUuid, kFrUuidText);
    const uint64_t world = b.string(kFrRunWorld, m.world_len);
    const uint64_t records = b.offsets0();
    const uint64_t entities = b.offsets0();
    const uint64_t flex = has_flex ? b.bytes(kFrRunFlex, m.flex_len) : 0;
    // Message::create: the slots in its order; 0 = not pushed
    const uint64_t start = b.used;
    const uint64_t l_flex = has_flex ? b.push_off(flex) : 0;
    const uint64_t l_pos = has_pos ? b.push_vec3() : 0;
    const uint64_t l_ent = b.push_off(entities);
    const uint64_t l_rec = b.push_off(records);
    const uint64_t l_world = b.push_off(world);
    const uint64_t l_sender = b.push_off(sender);
    const uint64_t l_param = has_param ? b.push_off(param) : 0;
    const uint64_t l_repl = m.replication ? b.push_u8(m.replication) : 0;   // defaults are not written
    const uint64_t l_instr = m.instruction ? b.push_u8(m.instruction) : 0;
    // end_table: the soffset, then the vtable right below it
    const uint64_t obj = b.push_u32(0);  // the host rewrites this word once the vtable is placed: told below
    const uint32_t max_id = has_flex ? kFrFlex : has_pos ? kFrPos : kFrEntities;
    const uint32_t vt_len = max_id + 2;
    b.used += vt_len;
    const uint64_t vt = b.used;
    sink.value(vt, 2, vt_len);
    sink.value(vt - 2, 2, (uint32_t)(obj - start));
    if (l_flex) sink.value(vt - kFrFlex, 2, (uint32_t)(obj - l_flex));
    if (l_pos) sink.value(vt - kFrPos, 2, (uint32_t)(obj - l_pos));
    sink.value(vt - kFrEntities, 2, (uint32_t)(obj - l_ent));
    sink.value(vt - kFrRecords, 2, (uint32_t)(obj - l_rec));
    sink.value(vt - kFrWorld, 2, (uint32_t)(obj - l_world));
    sink.value(vt - kFrSender, 2, (uint32_t)(obj - l_sender));
    if (l_param) sink.value(vt - kFrParam, 2, (uint32_t)(obj - l_param));
    if (l_repl) sink.value(vt - kFrRepl, 2, (uint32_t)(obj - l_repl));
    if (l_instr) sink.value(vt - kFrInstr, 2, (uint32_t)(obj - l_instr));
    sink.value(obj, 4, (uint32_t)(vt - obj));  // the soffset
    // finish
    b.align(4, b.min_align);
    b.push_off(obj);
    return b.used;
}

struct FrameNoSink {
    __host__ __device__ __forceinline__ void value(uint64_t, uint32_t, uint32_t) {}
    __host__ __device__ __forceinline__ void run(uint32_t, uint64_t, uint32_t) {}
};

// The frame's size: 0 with *err |= kFrErrLarge above kFrameMax.
__host__ __device__ __forceinline__ uint32_t frame_size(const FrameMsg& m, uint32_t* err) {
    FrameNoSink k;
    const uint64_t size = frame_walk(m, k);
    if (size > kFrameMax) {
        *err |= kFrErrLarge;
        return 0u;
    }
    return (uint32_t)size;
}

// The term of message q in the scan of the sizes: 0 behind the n messages.
__host__ __device__ __forceinline__ uint64_t frame_term(const uint32_t* __restrict__ size, uint64_t n, uint64_t q) {
    return q < n ? (uint64_t)size[q] : 0ull;
}

// Where the two payloads end (revloc) in the frame; length 0 when absent or empty.
struct FrameSpanSink {
    uint64_t param_end = 0, flex_end = 0;
    uint32_t param_len = 0, flex_len = 0;
    __host__ __device__ __forceinline__ void value(uint64_t, uint32_t, uint32_t) {}
    __host__ __device__ __forceinline__ void run(uint32_t kind, uint64_t rev_end, uint32_t len) {
        if (kind == kFrRunParam) param_end = rev_end, param_len = len;
        if (kind == kFrRunFlex) flex_end = rev_end, flex_len = len;
    }
};

// Does a payload of the frame that starts at output byte r0 hold the whole tile [c0, c1)? Then *from
// is the address of the source byte of output byte c0.
__host__ __device__ __forceinline__ bool frame_tile_inside(const FrameSrc& s, const FrameMsg& m, uint64_t r0, uint64_t r1,
                                                           uint64_t c0, uint64_t c1, const uint8_t** from) {
    if (c1 - c0 != kPackTile || r1 - r0 < kPackTile) return false;
    FrameSpanSink k;
    const uint64_t size = frame_walk(m, k);
    const uint64_t pg = r0 + size - k.param_end, fg = r0 + size - k.flex_end;
    if (k.param_len && pg <= c0 && c1 <= pg + k.param_len) {
        *from = s.param + m.param_src + (c0 - pg);
        return true;
    }
    if (k.flex_len && fg <= c0 && c1 <= fg + k.flex_len) {
        *from = s.flex + m.flex_src + (c0 - fg);
        return true;
    }
    return false;
}

// Byte k of a chunk.
__host__ __device__ __forceinline__ uint8_t frame_chunk_byte(const PackChunk& v, uint32_t k) {
    return (uint8_t)(k < 8 ? v.lo >> (8 * k) : v.hi >> (8 * (k - 8)));
}

// Collects the bytes of the output that frame i holds inside the chunk [d0, d0 + 16): d0 <= lo < hi <=
// d0 + 16, and [lo, hi) inside the frame [r0, r0 + size). A frame's size is a multiple of four (finish
// aligns to min_align >= 4), so r0 is one too, and d0 is a multiple of 16: a value of 4, 2 or 1 bytes
// is naturally aligned in the output and never straddles a chunk or one of its 8-byte halves. Values
// are therefore ORed into `acc` whole wherever they fall in the chunk and `acc` is cut to [lo, hi)
// once, in done(). Runs come from one 16-byte load laid over the chunk and masked to the run when
// those 16 source bytes all lie inside their array (the world table has kFrWorldSlack bytes of slack
// on both sides for that), else byte by byte; the uuid's 16 bytes are loaded once and its text
// computed. Nothing outside [0, n_*_bytes) of the payloads, the message's uuid and position and the
// table with its slack is read.
struct FrameChunkSink {
    const FrameSrc& s;
    const FrameMsg& m;
    uint64_t i, r0, size, d0, lo, hi;
    PackChunk acc{0ull, 0ull};

    __host__ __device__ __forceinline__ void value(uint64_t rev_end, uint32_t, uint32_t v) {
        const uint64_t at = r0 + size - rev_end - d0;  // wraps far above 16 for a value before the chunk
        const uint64_t x = (uint64_t)v << (8 * (at & 7));
        acc.lo |= at < 8 ? x : 0ull;
        acc.hi |= (at >= 8 && at < kPackChunk) ? x : 0ull;
    }
    __host__ __device__ __forceinline__ void or_byte(uint32_t at, uint64_t byte) {
        if (at < 8)
            acc.lo |= byte << (8 * at);
        else
            acc.hi |= byte << (8 * (at - 8));
    }
    __host__ __device__ __forceinline__ void run(uint32_t kind, uint64_t rev_end, uint32_t len) {
        const uint64_t g = r0 + size - rev_end;
        const uint64_t a = g > lo ? g : lo, b = g + len < hi ? g + len : hi;
        if (a >= b) return;
        if (kind == kFrRunUuid) {
            const PackChunk u = pack_load16(s.sender_uuid + 16 * i);
            for (uint64_t c = a; c < b; ++c) {
                const uint32_t j = (uint32_t)(c - g);
                uint8_t ch = (uint8_t)'-';
                if (!(j == 8 || j == 13 || j == 18 || j == 23)) {
                    const uint32_t d = j - (j > 8) - (j > 13) - (j > 18) - (j > 23);
                    const uint32_t byte = frame_chunk_byte(u, d >> 1);
                    const uint32_t nib = (d & 1u) ? (byte & 15u) : (byte >> 4);
                    ch = (uint8_t)(nib < 10 ? '0' + nib : 'a' + (nib - 10));
                }
                or_byte((uint32_t)(c - d0), ch);
            }
            return;
        }
        const uint8_t* base;
        uint64_t total, off, slack = 0;
        if (kind == kFrRunParam) {
            base = s.param, total = s.n_param_bytes, off = m.param_src;
        } else if (kind == kFrRunFlex) {
            base = s.flex, total = s.n_flex_bytes, off = m.flex_src;
        } else if (kind == kFrRunWorld) {
            base = s.world_bytes, total = s.n_world_bytes, off = m.world_src, slack = s.world_slack;
        } else {
            base = s.pos, total = 24 * s.n, off = 24 * i;
        }
        const uint64_t t = off + d0 + slack, u = g;  // chunk byte j is base[t - slack - u + j]
        if (t >= u && t - u + kPackChunk <= total + 2 * slack) {
            pack_merge(&acc, pack_load16(base - slack + (t - u)), (uint32_t)(a - d0), (uint32_t)(b - d0));
        } else {
            for (uint64_t c = a; c < b; ++c) or_byte((uint32_t)(c - d0), base[off + (c - g)]);
        }
    }
    // The frame's bytes of the chunk, cut to [lo, hi), ORed into *out.
    __host__ __device__ __forceinline__ void done(PackChunk* out) const {
        pack_merge(out, acc, (uint32_t)(lo - d0), (uint32_t)(hi - d0));
    }
};

// The composer: ORs into *out the bytes [lo_c, hi_c) of the chunk [d0, d0 + 16) from the frames of
// the window W (W[k] = E[min(wb + k, n)], pack_ops.hpp). Needs W[0] <= lo_c < hi_c <=
// min(d0 + 16, W[kPackWindow]) and d0 <= lo_c.
__host__ __device__ __forceinline__ void frame_compose(const uint64_t* W, uint64_t wb, const FrameSrc& s, uint64_t d0,
                                                       uint64_t lo_c, uint64_t hi_c, PackChunk* out) {
    uint32_t k = pack_win_find(W, lo_c);
    uint64_t c = lo_c;
    while (c < hi_c) {
        while (W[k + 1] <= c) ++k;  // empty frames; W[kPackWindow] >= hi_c > c ends it
        const uint64_t r0 = W[k], r1 = W[k + 1];
        const uint64_t e = r1 < hi_c ? r1 : hi_c;
        const FrameMsg m = frame_msg(s, wb + k);
        FrameChunkSink sink{s, m, wb + k, r0, r1 - r0, d0, c, e};
        frame_walk(m, sink);
        sink.done(out);
        c = e;
    }
}

}  // namespace wq
