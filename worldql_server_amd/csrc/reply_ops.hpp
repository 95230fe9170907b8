// reply_ops.hpp — the arithmetic of the record reply builder (wq_reply.hip, wq_frames_build_records_device):
// frames of messages that carry a `records` vector read from the payload slab (slab_ops.hpp) through a CSR
// of handles. A sibling of frame_ops.hpp, whose builder-on-counters, message fields and chunk arithmetic it
// uses. __host__ __device__, so tests/cpp/record_frames_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/frames.py (build_record_frames_np).
//
// The bytes are wq_codec.cpp's: serialize_one pushes the parameter, sender and world strings, then every
// record (pack_record), the offsets vector, the empty entities vector, flex, the table. reply_walk is that
// sequence with the records as one block of rec_bytes and the vector as n slots; rec_walk is pack_record
// and end_table for one record from the fill `used0` it starts at. What the builder's vtable dedupe does
// is restated as two facts: a record's vtable depends on its shape alone (data, flex, position), and it is
// written only at the shape's first occurrence in the frame; later records point their soffset at it.
//
// Ordinals: the rows are the send side's (budget_ops.hpp: clamped, at most n_handles in total), ordinal q
// of row p is handle element bud_row_start(p) + q - pre[p]. A segmented scan over the ordinals carries a
// 13-bit state per row prefix (RpState): the shapes seen, and the last kept record's shape with whether it
// was new, which says whether it left the fill at 2 mod 4 (a vtable of 10 or 14 bytes). With the exclusive
// state X[q] a record's bytes are known locally (its align absorbs the residue), so P, the u64 prefix sum
// of the records' sizes, places every record: record q of row p starts at fill rec_start + P[q] - P[pre[p]].
// K counts the kept records before q, and first[8 p + shape] is the ordinal of a shape's first occurrence.
#pragma once

#include "../../include/wq_router.h"
#include "frame_ops.hpp"

namespace wq {

constexpr uint32_t kRpErrHandle = 16u;  // error bit 4: a handle >= n_entries or an entry that is not live
constexpr uint32_t kRpErrArena = 32u;   // bit 5: a payload range that leaves the arena
constexpr uint32_t kRpErrRows = 64u;    // bit 6: rows that descend, pass n_handles or overlap
constexpr uint32_t kRpSkipEmpty = 1u;   // WQ_FRAMES_SKIP_EMPTY

// Record vtable slots (wq_codec.cpp SR_*) and the kinds of byte runs rec_walk pushes.
enum : uint32_t { kRpUuid = 4, kRpPos = 6, kRpWorld = 8, kRpData = 10, kRpFlex = 12 };
enum : uint32_t { kRpRunUuid = 5, kRpRunWorld = 6, kRpRunData = 7, kRpRunFlex = 8, kRpRunPos = 9 };

// RpState: the segmented scan's value.
constexpr uint32_t kRpHead = 1u << 31, kRpHasLast = 1u << 8, kRpNew = 1u << 12;

struct ReplySrc {
    const uint32_t* row_offsets;  // [n + 1]
    const uint32_t* handles;
    uint32_t n_handles;
    uint32_t flags;
    const wq_slab_entry* entries;
    uint64_t n_entries;
    const uint8_t* arena;
    uint64_t n_arena;
    const uint8_t* world_bytes;  // per-message names (nullable: src.world ids)
    const uint8_t* world_off;    // u64[n]
    const uint8_t* world_len;    // u32[n]
    uint64_t n_world_bytes;
};

// Everything the passes share: the message source, the record source and the scratch.
struct ReplyCtx {
    FrameSrc s;
    ReplySrc r;
    const uint32_t* pre;  // [n + 1] the rows' ordinal space
    uint32_t* X;          // [T + 1] exclusive RpState
    uint32_t* term;       // [T + 1] the scan's terms
    uint32_t* sz;         // [T] record sizes
    uint64_t* P;          // [T + 1]
    uint64_t* K;          // [T + 1]
    uint32_t* first;      // [8 n]
};

__host__ __device__ __forceinline__ uint32_t rp_vt_len(uint32_t shape) { return (shape & 2u) ? 14u : (shape & 1u) ? 12u : 10u; }

__host__ __device__ __forceinline__ uint32_t rp_combine(uint32_t a, uint32_t b) {
    if (b & kRpHead) return b;
    uint32_t out = (a & kRpHead) | ((a | b) & 0xFFu);
    if (b & kRpHasLast) {
        const uint32_t shape = (b >> 9) & 7u;
        out |= kRpHasLast | (shape << 9);
        if ((b & kRpNew) && !((a >> shape) & 1u)) out |= kRpNew;
    } else {
        out |= a & (kRpHasLast | (7u << 9) | kRpNew);
    }
    return out;
}
struct RpCombine {
    __host__ __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return rp_combine(a, b); }
};
// The fill's residue mod 4 the state's last kept record left: 2 behind a new vtable of 10 or 14 bytes.
__host__ __device__ __forceinline__ uint32_t rp_residue(uint32_t x) {
    return ((x & kRpHasLast) && (x & kRpNew)) ? (rp_vt_len((x >> 9) & 7u) & 3u) : 0u;
}

// One record after the validity rules.
struct RecFields {
    const wq_slab_entry* e;
    uint64_t data_src, flex_src, world_src;
    uint32_t data_len, flex_len, world_len;
    uint32_t shape, err;
    bool kept;
};

__host__ __device__ __forceinline__ RecFields rec_eval(const FrameSrc& s, const ReplySrc& r, uint32_t handle) {
    RecFields f;
    f.e = nullptr;
    f.data_src = f.flex_src = f.world_src = 0;
    f.data_len = f.flex_len = f.world_len = 0;
    f.shape = 0, f.err = 0, f.kept = false;
    if (handle >= r.n_entries || !(r.entries[handle].bits & WQ_SLAB_LIVE)) {
        f.err = kRpErrHandle;
        return f;
    }
    const wq_slab_entry* e = r.entries + handle;
    f.e = e, f.kept = true, f.shape = e->bits & 7u;
    const uint64_t off = e->off, n = r.n_arena;
    const uint64_t dl = e->data_len, fl = e->flex_len;
    if (e->bits & WQ_SLAB_DATA) {
        if (off > n || dl > n - off)
            f.err |= kRpErrArena;
        else
            f.data_src = off, f.data_len = (uint32_t)dl;
    }
    if (e->bits & WQ_SLAB_FLEX) {
        if (off > n || dl + fl > n - off)
            f.err |= kRpErrArena;
        else
            f.flex_src = off + dl, f.flex_len = (uint32_t)fl;
    }
    if (e->world < s.n_worlds) {
        f.world_src = s.world_off[e->world];
        f.world_len = s.world_off[e->world + 1] - s.world_off[e->world];
    } else {
        f.err |= kFrErrWorld;
    }
    return f;
}

// pack_record and end_table from the fill used0: returns the fill behind the record; *obj is the table's
// revloc. `first`: the vtable is written here; else the soffset points at vt_use.
template <typename Sink>
__host__ __device__ __forceinline__ uint64_t rec_walk(const RecFields& f, uint64_t used0, bool first, uint64_t vt_use,
                                                      Sink& sink, uint64_t* obj_out) {
    FrameBuilder<Sink> b(sink);
    b.used = used0;
    const bool has_data = f.shape & 1u, has_flex = f.shape & 2u, has_pos = f.shape & 4u;
    const uint64_t uuid = b.string(kRpRunUuid, kFrUuidText);
    const uint64_t world = b.string(kRpRunWorld, f.world_len);
    const uint64_t data = has_data ? b.string(kRpRunData, f.data_len) : 0;
    const uint64_t flex = has_flex ? b.bytes(kRpRunFlex, f.flex_len) : 0;
    const uint64_t start = b.used;
    const uint64_t l_flex = has_flex ? b.push_off(flex) : 0;
    const uint64_t l_data = has_data ? b.push_off(data) : 0;
    const uint64_t l_world = b.push_off(world);
    uint64_t l_pos = 0;
    if (has_pos) {
        b.used += 24;
        sink.run(kRpRunPos, b.used, 24);
        l_pos = b.used;
    }
    const uint64_t l_uuid = b.push_off(uuid);
    b.used += 4;  // the soffset, told below
    const uint64_t obj = b.used;
    if (first) {
        const uint32_t vt_len = rp_vt_len(f.shape);
        b.used += vt_len;
        const uint64_t vt = b.used;
        sink.value(vt, 2, vt_len);
        sink.value(vt - 2, 2, (uint32_t)(obj - start));
        if (l_flex) sink.value(vt - kRpFlex, 2, (uint32_t)(obj - l_flex));
        if (l_data) sink.value(vt - kRpData, 2, (uint32_t)(obj - l_data));
        sink.value(vt - kRpWorld, 2, (uint32_t)(obj - l_world));
        if (l_pos) sink.value(vt - kRpPos, 2, (uint32_t)(obj - l_pos));
        sink.value(vt - kRpUuid, 2, (uint32_t)(obj - l_uuid));
        vt_use = vt;
    }
    sink.value(obj, 4, (uint32_t)(vt_use - obj));  // the soffset: negative towards an earlier record's vtable
    *obj_out = obj;
    return b.used;
}

// A row's records as the message walk needs them.
struct RowRec {
    uint32_t s, e;       // its ordinals
    uint64_t rec_bytes;  // the records' bytes
    uint64_t n_kept;
};
struct ReplyLayout {
    uint64_t rec_start, vec_begin, size;
};

__host__ __device__ __forceinline__ RowRec reply_row(const ReplyCtx& c, uint64_t i) {
    RowRec w;
    w.s = c.pre[i], w.e = c.pre[i + 1];
    w.rec_bytes = c.P[w.e] - c.P[w.s];
    w.n_kept = c.K[w.e] - c.K[w.s];
    return w;
}

// Message i: frame_msg with the per-message world names and the nullable sender.
__host__ __device__ __forceinline__ FrameMsg reply_msg(const ReplyCtx& c, uint64_t i) {
    if (!c.r.world_bytes) return frame_msg(c.s, i);
    const FrameSrc& t = c.s;
    FrameMsg m;
    {
        // frame_msg's fields without its world lookup
        m.err = 0;
        m.instruction = t.instruction ? t.instruction[i] : t.instruction_all;
        m.replication = t.replication ? t.replication[i] : t.replication_all;
        const uint32_t given = (t.pos ? kFrHasPos : 0u) | (t.param_offsets ? kFrHasParam : 0u) | (t.flex_offsets ? kFrHasFlex : 0u);
        m.has = t.msg_flags ? (uint32_t)t.msg_flags[i] & given : given;
        m.param_src = m.flex_src = 0;
        m.param_len = m.flex_len = 0;
        if ((m.has & kFrHasParam) && !frame_range(t.param_offsets, i, t.n_param_bytes, &m.param_src, &m.param_len)) m.err |= kFrErrParam;
        if ((m.has & kFrHasFlex) && !frame_range(t.flex_offsets, i, t.n_flex_bytes, &m.flex_src, &m.flex_len)) m.err |= kFrErrFlex;
    }
    const uint64_t a = frame_ld<uint64_t>(c.r.world_off, i), ln = frame_ld<uint32_t>(c.r.world_len, i);
    m.world_src = 0, m.world_len = 0;
    if (a > c.r.n_world_bytes || ln > c.r.n_world_bytes - a)
        m.err |= kFrErrWorld;
    else
        m.world_src = a, m.world_len = (uint32_t)ln;
    return m;
}

// serialize_one with the row's records as a block: frame_walk's sequence with the records and their
// offsets vector in place of the empty vector. The sink is told everything but the records and the slots.
template <typename Sink>
__host__ __device__ __forceinline__ ReplyLayout reply_walk(const FrameMsg& m, const RowRec& w, Sink& sink) {
    FrameBuilder<Sink> b(sink);
    ReplyLayout L;
    const bool has_param = m.has & kFrHasParam, has_flex = m.has & kFrHasFlex, has_pos = m.has & kFrHasPos;
    const uint64_t param = has_param ? b.string(kFrRunParam, m.param_len) : 0;
    const uint64_t sender = b.string(kFrRunUuid, kFrUuidText);
    const uint64_t world = b.string(kFrRunWorld, m.world_len);
    L.rec_start = b.used;
    b.used += w.rec_bytes;
    b.align(4 * w.n_kept, 4);  // absorbs the last record's residue
    L.vec_begin = b.used;
    b.used += 4 * w.n_kept;  // the slots, last record first
    const uint64_t records = b.push_u32((uint32_t)w.n_kept);
    const uint64_t entities = b.offsets0();
    const uint64_t flex = has_flex ? b.bytes(kFrRunFlex, m.flex_len) : 0;
    const uint64_t start = b.used;
    const uint64_t l_flex = has_flex ? b.push_off(flex) : 0;
    const uint64_t l_pos = has_pos ? b.push_vec3() : 0;
    const uint64_t l_ent = b.push_off(entities);
    const uint64_t l_rec = b.push_off(records);
    const uint64_t l_world = b.push_off(world);
    const uint64_t l_sender = b.push_off(sender);
    const uint64_t l_param = has_param ? b.push_off(param) : 0;
    const uint64_t l_repl = m.replication ? b.push_u8(m.replication) : 0;
    const uint64_t l_instr = m.instruction ? b.push_u8(m.instruction) : 0;
    const uint64_t obj = b.push_u32(0);
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
    sink.value(obj, 4, (uint32_t)(vt - obj));
    b.align(4, b.min_align);
    b.push_off(obj);
    L.size = b.used;
    return L;
}

// ---- the passes ----

// The handle of ordinal q of row p.
__host__ __device__ __forceinline__ uint32_t reply_handle(const ReplyCtx& c, uint32_t p, uint32_t q) {
    return c.r.handles[bud_row_start(c.r.row_offsets, p, c.r.n_handles) + (q - c.pre[p])];
}

// Element pass, ordinal q < T of row p: the scan's term; *err gets the record's error bits.
__host__ __device__ __forceinline__ uint32_t reply_term(const ReplyCtx& c, uint32_t p, uint32_t q, uint32_t* err) {
    const RecFields f = rec_eval(c.s, c.r, reply_handle(c, p, q));
    *err |= f.err;
    uint32_t t = q == c.pre[p] ? kRpHead : 0u;
    if (f.kept) t |= (1u << f.shape) | kRpHasLast | (f.shape << 9) | kRpNew;
    return t;
}

// The exclusive state in front of ordinal q of a row that starts at s.
__host__ __device__ __forceinline__ uint32_t reply_state(const ReplyCtx& c, uint32_t s, uint32_t q) {
    return q == s ? 0u : c.X[q] & ~kRpHead;
}

// Place pass, ordinal q of row p: the record's size (saturating at 2^31) and, for a shape's first
// occurrence, its entry in `first`.
__host__ __device__ __forceinline__ uint32_t reply_place(const ReplyCtx& c, uint32_t p, uint32_t q) {
    const RecFields f = rec_eval(c.s, c.r, reply_handle(c, p, q));
    if (!f.kept) return 0u;
    const uint32_t x = reply_state(c, c.pre[p], q);
    const bool first = !((x >> f.shape) & 1u);
    if (first) c.first[8ull * p + f.shape] = q;
    FrameNoSink k;
    uint64_t obj;
    const uint64_t used0 = rp_residue(x);
    const uint64_t size = rec_walk(f, used0, first, 0, k, &obj) - used0;
    return size > (1ull << 31) ? (1u << 31) : (uint32_t)size;
}

// Row pass, message i: the frame's size under the 2^30 rule and WQ_FRAMES_SKIP_EMPTY.
__host__ __device__ __forceinline__ uint32_t reply_size(const ReplyCtx& c, uint64_t i, uint32_t* err) {
    const FrameMsg m = reply_msg(c, i);
    *err |= m.err;
    const RowRec w = reply_row(c, i);
    if (!w.n_kept && (c.r.flags & kRpSkipEmpty)) return 0u;
    FrameNoSink k;
    const uint64_t size = reply_walk(m, w, k).size;
    if (size > kFrameMax) {
        *err |= kFrErrLarge;
        return 0u;
    }
    return (uint32_t)size;
}

// ---- the copy ----

// ORs into acc the part [a, b) (output bytes) of a run that starts at output byte g and whose source is
// base[off ..] in an array of `total` bytes with `slack` readable bytes on both sides: one masked 16-byte
// load laid over the chunk at d0 when those 16 bytes lie inside the array, else byte by byte.
__host__ __device__ __forceinline__ void rp_copy_run(PackChunk* acc, const uint8_t* base, uint64_t total, uint64_t slack,
                                                     uint64_t off, uint64_t g, uint64_t d0, uint64_t a, uint64_t b) {
    const uint64_t t = off + d0 + slack;
    if (t >= g && t - g + kPackChunk <= total + 2 * slack) {
        pack_merge(acc, pack_load16(base - slack + (t - g)), (uint32_t)(a - d0), (uint32_t)(b - d0));
        return;
    }
    for (uint64_t x = a; x < b; ++x) {
        const uint64_t byte = base[off + (x - g)];
        const uint32_t at = (uint32_t)(x - d0);
        if (at < 8)
            acc->lo |= byte << (8 * at);
        else
            acc->hi |= byte << (8 * (at - 8));
    }
}

// The same for the 36 characters of a uuid (u: its 16 bytes, nullptr: the nil uuid).
__host__ __device__ __forceinline__ void rp_copy_uuid(PackChunk* acc, const uint8_t* u16, uint64_t g, uint64_t d0, uint64_t a,
                                                      uint64_t b) {
    PackChunk u{0ull, 0ull};
    if (u16) u = pack_load16(u16);
    for (uint64_t x = a; x < b; ++x) {
        const uint32_t j = (uint32_t)(x - g);
        uint64_t ch = '-';
        if (!(j == 8 || j == 13 || j == 18 || j == 23)) {
            const uint32_t d = j - (j > 8) - (j > 13) - (j > 18) - (j > 23);
            const uint32_t byte = frame_chunk_byte(u, d >> 1);
            const uint32_t nib = (d & 1u) ? (byte & 15u) : (byte >> 4);
            ch = nib < 10 ? '0' + nib : 'a' + (nib - 10);
        }
        const uint32_t at = (uint32_t)(x - d0);
        if (at < 8)
            acc->lo |= ch << (8 * at);
        else
            acc->hi |= ch << (8 * (at - 8));
    }
}

// Collects what the message (rec == nullptr) or one record of frame i puts into the chunk [d0, d0 + 16),
// cut to [lo, hi): FrameChunkSink's arithmetic (values are naturally aligned in the output and ORed whole,
// cut once in done()) with the reply's sources.
struct ReplyChunkSink {
    const ReplyCtx& c;
    const FrameMsg* m;
    const RecFields* rec;
    uint64_t i, top, d0, lo, hi;  // top: the output byte behind the frame
    PackChunk acc{0ull, 0ull};

    __host__ __device__ __forceinline__ void value(uint64_t rev_end, uint32_t, uint32_t v) {
        const uint64_t at = top - rev_end - d0;
        const uint64_t x = (uint64_t)v << (8 * (at & 7));
        acc.lo |= at < 8 ? x : 0ull;
        acc.hi |= (at >= 8 && at < kPackChunk) ? x : 0ull;
    }
    __host__ __device__ __forceinline__ void run(uint32_t kind, uint64_t rev_end, uint32_t len) {
        const uint64_t g = top - rev_end;
        const uint64_t a = g > lo ? g : lo, b = g + len < hi ? g + len : hi;
        if (a >= b) return;
        const FrameSrc& s = c.s;
        switch (kind) {
            case kFrRunUuid: rp_copy_uuid(&acc, s.sender_uuid ? s.sender_uuid + 16 * i : nullptr, g, d0, a, b); break;
            case kRpRunUuid: rp_copy_uuid(&acc, rec->e->uuid, g, d0, a, b); break;
            case kFrRunParam: rp_copy_run(&acc, s.param, s.n_param_bytes, 0, m->param_src, g, d0, a, b); break;
            case kFrRunFlex: rp_copy_run(&acc, s.flex, s.n_flex_bytes, 0, m->flex_src, g, d0, a, b); break;
            case kFrRunWorld:
                if (c.r.world_bytes)
                    rp_copy_run(&acc, c.r.world_bytes, c.r.n_world_bytes, 0, m->world_src, g, d0, a, b);
                else
                    rp_copy_run(&acc, s.world_bytes, s.n_world_bytes, s.world_slack, m->world_src, g, d0, a, b);
                break;
            case kFrRunPos: rp_copy_run(&acc, s.pos, 24 * s.n, 0, 24 * i, g, d0, a, b); break;
            case kRpRunWorld: rp_copy_run(&acc, s.world_bytes, s.n_world_bytes, s.world_slack, rec->world_src, g, d0, a, b); break;
            case kRpRunData: rp_copy_run(&acc, c.r.arena, c.r.n_arena, 0, rec->data_src, g, d0, a, b); break;
            case kRpRunFlex: rp_copy_run(&acc, c.r.arena, c.r.n_arena, 0, rec->flex_src, g, d0, a, b); break;
            default: rp_copy_run(&acc, reinterpret_cast<const uint8_t*>(rec->e->pos), 24, 0, 0, g, d0, a, b); break;
        }
    }
    __host__ __device__ __forceinline__ void done(PackChunk* out) const {
        pack_merge(out, acc, (uint32_t)(lo - d0), (uint32_t)(hi - d0));
    }
};

// The first ordinal q in [s, e] with P[q + 1] - P[s] > rel (e when there is none): the record whose bytes
// reach past the relative fill `rel`.
__host__ __device__ __forceinline__ uint32_t rp_record_past(const uint64_t* P, uint32_t s, uint32_t e, uint64_t rel) {
    uint32_t lo = s, hi = e;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (P[mid + 1] - P[s] > rel)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// The k-th kept ordinal of the row [s, e) (k < its kept count): the last q with K[q] - K[s] <= k.
__host__ __device__ __forceinline__ uint32_t rp_kept_at(const uint64_t* K, uint32_t s, uint32_t e, uint64_t k) {
    uint32_t lo = s, hi = e - 1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (K[mid] - K[s] <= k)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// Where record q of row i = [s, e) starts (fill) and how it is placed.
struct RecPlace {
    RecFields f;
    uint64_t used0, vt_use;
    bool first;
};
__host__ __device__ __forceinline__ RecPlace reply_rec(const ReplyCtx& c, uint64_t i, const RowRec& w, uint64_t rec_start,
                                                       uint32_t q) {
    RecPlace p;
    p.f = rec_eval(c.s, c.r, reply_handle(c, (uint32_t)i, q));
    const uint32_t x = reply_state(c, w.s, q);
    p.first = !((x >> p.f.shape) & 1u);
    p.used0 = rec_start + (c.P[q] - c.P[w.s]);
    // a shape's vtable is the last thing its first record pushes: it starts at that record's end
    p.vt_use = p.first ? 0 : rec_start + (c.P[c.first[8 * i + p.f.shape] + 1] - c.P[w.s]);
    return p;
}

// ORs into *out the bytes [lo, hi) of the chunk [d0, d0 + 16) that frame i = [r0, r0 + size) holds.
__host__ __device__ __forceinline__ void reply_compose_frame(const ReplyCtx& c, uint64_t i, uint64_t r0, uint64_t size,
                                                             uint64_t d0, uint64_t lo, uint64_t hi, PackChunk* out) {
    const FrameMsg m = reply_msg(c, i);
    const RowRec w = reply_row(c, i);
    const uint64_t top = r0 + size;
    ReplyChunkSink sink{c, &m, nullptr, i, top, d0, lo, hi};
    const ReplyLayout L = reply_walk(m, w, sink);
    // the chunk's bytes are the pieces with revloc in (r_lo, r_hi]
    const uint64_t r_lo = top - hi, r_hi = top - lo;
    if (w.rec_bytes && r_hi > L.rec_start && r_lo < L.rec_start + w.rec_bytes) {
        const uint64_t rel = r_lo > L.rec_start ? r_lo - L.rec_start : 0;
        for (uint32_t q = rp_record_past(c.P, w.s, w.e, rel); q < w.e && L.rec_start + (c.P[q] - c.P[w.s]) < r_hi; ++q) {
            if (c.P[q + 1] == c.P[q]) continue;  // left out
            const RecPlace p = reply_rec(c, i, w, L.rec_start, q);
            sink.rec = &p.f;
            uint64_t obj;
            rec_walk(p.f, p.used0, p.first, p.vt_use, sink, &obj);
        }
    }
    // the slots: slot k ends at revloc vec_begin + 4 (n - k)
    if (w.n_kept && r_hi > L.vec_begin && r_lo < L.vec_begin + 4 * w.n_kept) {
        const uint64_t j0 = r_lo > L.vec_begin ? (r_lo - L.vec_begin) / 4 + 1 : 1;  // first j with vec_begin + 4 j > r_lo
        FrameNoSink none;
        for (uint64_t j = j0; j <= w.n_kept && L.vec_begin + 4 * j - 4 < r_hi; ++j) {
            const uint32_t q = rp_kept_at(c.K, w.s, w.e, w.n_kept - j);
            const RecPlace p = reply_rec(c, i, w, L.rec_start, q);
            uint64_t obj;
            rec_walk(p.f, p.used0, false, 0, none, &obj);
            sink.value(L.vec_begin + 4 * j, 4, (uint32_t)(L.vec_begin + 4 * j - obj));
        }
    }
    sink.done(out);
}

// The composer over the window W of frame offsets (pack_ops.hpp), as frame_compose.
__host__ __device__ __forceinline__ void reply_compose(const uint64_t* W, uint64_t wb, const ReplyCtx& c, uint64_t d0,
                                                       uint64_t lo_c, uint64_t hi_c, PackChunk* out) {
    uint32_t k = pack_win_find(W, lo_c);
    uint64_t x = lo_c;
    while (x < hi_c) {
        while (W[k + 1] <= x) ++k;
        const uint64_t r0 = W[k], r1 = W[k + 1];
        const uint64_t e = r1 < hi_c ? r1 : hi_c;
        reply_compose_frame(c, wb + k, r0, r1 - r0, d0, x, e, out);
        x = e;
    }
}

// Where the payloads end (revloc); length 0 when absent or empty.
struct ReplySpanSink {
    uint64_t end[4] = {0, 0, 0, 0};  // param, flex, record data, record flex
    uint32_t len[4] = {0, 0, 0, 0};
    __host__ __device__ __forceinline__ void value(uint64_t, uint32_t, uint32_t) {}
    __host__ __device__ __forceinline__ void run(uint32_t kind, uint64_t rev_end, uint32_t n) {
        const int k = kind == kFrRunParam ? 0 : kind == kFrRunFlex ? 1 : kind == kRpRunData ? 2 : kind == kRpRunFlex ? 3 : -1;
        if (k >= 0) end[k] = rev_end, len[k] = n;
    }
};

// Does one payload of frame i = [r0, r1) hold the whole tile [c0, c1)? Then *from is the address of the
// source byte of output byte c0.
__host__ __device__ __forceinline__ bool reply_tile_inside(const ReplyCtx& c, uint64_t i, uint64_t r0, uint64_t r1, uint64_t c0,
                                                           uint64_t c1, const uint8_t** from) {
    if (c1 - c0 != kPackTile || r1 - r0 < kPackTile) return false;
    const FrameMsg m = reply_msg(c, i);
    const RowRec w = reply_row(c, i);
    ReplySpanSink k;
    const ReplyLayout L = reply_walk(m, w, k);
    const uint64_t top = r0 + L.size;
    const uint64_t src[2] = {m.param_src, m.flex_src};
    const uint8_t* base[2] = {c.s.param, c.s.flex};
    for (int t = 0; t < 2; ++t) {
        const uint64_t g = top - k.end[t];
        if (k.len[t] && g <= c0 && c1 <= g + k.len[t]) {
            *from = base[t] + src[t] + (c0 - g);
            return true;
        }
    }
    const uint64_t r_hi = top - c0;  // the revloc of the piece that starts at c0
    if (!w.rec_bytes || r_hi <= L.rec_start || r_hi > L.rec_start + w.rec_bytes) return false;
    const uint32_t q = rp_record_past(c.P, w.s, w.e, r_hi - L.rec_start - 1);
    if (q >= w.e) return false;
    const RecPlace p = reply_rec(c, i, w, L.rec_start, q);
    uint64_t obj;
    rec_walk(p.f, p.used0, p.first, p.vt_use, k, &obj);
    const uint64_t rsrc[2] = {p.f.data_src, p.f.flex_src};
    for (int t = 0; t < 2; ++t) {
        const uint64_t g = top - k.end[2 + t];
        if (k.len[2 + t] && g <= c0 && c1 <= g + k.len[2 + t]) {
            *from = c.r.arena + rsrc[t] + (c0 - g);
            return true;
        }
    }
    return false;
}

}  // namespace wq
