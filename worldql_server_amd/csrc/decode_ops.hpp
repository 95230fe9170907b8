// decode_ops.hpp — the arithmetic of the ingest decoder (wq_decode.hip, wq_frames_decode_device): a
// bounded byte reader that composes unaligned little-endian values, the FlatBuffers 2.0.0 verifier walk
// over Message, Record and Entity, valid_utf8 in a form that can start anywhere in a string,
// parse_uuid, the world-name sanitizer as a byte stream, and the world and sender lookups.
// __host__ __device__, so tests/cpp/frames_decode_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/ingest.py (decode_frames_np).
//
// The contract is wq_codec.cpp's decode_one, check for check and in its order. What differs is where
// the work runs:
//   walk     one lane per frame: the whole structure, every string of up to kDecLane bytes, the decode
//            rules, the lookups. A longer string is appended to a work list (DecList) and taken as valid
//            for the rest of the walk; a lane that finds the list full validates the string itself.
//   strings  the listed strings, kDecChunk bytes per lane: UTF-8 validity is local, a chunk needs at
//            most 3 bytes before it to find where its first sequence starts and at most 3 behind it to
//            end its last one. An invalid chunk ORs kDecTentBad into the frame's word.
//   finish   a frame with kDecTentBad is rewritten to the verifier's failure: it ranks before every
//            decode error, so a long string can overturn a frame only to WQ_DEC_INVALID_FLATBUFFER.
// A frame is shorter than 2^32 bytes, so every position fits u64 arithmetic without the host's
// saturating adds: no sum below can wrap.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/wq_codec.h"
#include "../../include/wq_router.h"

namespace wq {

#define WQ_DEC_HD __host__ __device__ __forceinline__

constexpr uint32_t kDecLane = 256;       // L: a string of up to L bytes is validated by the walking lane
constexpr uint32_t kDecChunk = 16;       // bytes one lane validates in the strings pass
constexpr uint32_t kDecBlock = 256;      // lanes of a block in every pass
constexpr uint32_t kDecTile = kDecChunk * kDecBlock;  // 4 KiB: one step of a block in the strings pass
constexpr uint32_t kDecSlices = 16;      // blocks that share one listed string, tile by tile
constexpr uint32_t kDecListDefault = 65536;  // work-list entries unless the debug setter says otherwise
constexpr uint32_t kDecListBlocks = 256;     // blocks (x) of the strings pass; they stride over the entries
constexpr uint32_t kDecErrOffsets = 1u;  // error bit 0: frame offsets descend or reach past n_frame_bytes
constexpr uint32_t kDecErrHuge = 2u;     // error bit 1: a frame of 2^32 bytes or more
constexpr uint32_t kDecMaxTables = 1000000, kDecMaxDepth = 64;
constexpr uint64_t kDecMaxApparent = 1ull << 31;
constexpr uint32_t kDecNoPeer = 0xFFFFFFFFu;
constexpr uint32_t kDecWorldSlack = 16;  // frame_ops.hpp kFrWorldSlack: the zero bytes before the handle's world names

// flags bits (wq_ingest_out.flags)
constexpr uint32_t kDecOk = 1u, kDecHasPos = 2u, kDecHasParam = 4u, kDecHasFlex = 8u, kDecGlobal = 16u,
                   kDecWorldKnown = 32u, kDecSenderKnown = 64u;
// the frame's word between the passes: flags in bits 0-7, status in bits 8-9, the strings pass's verdict
constexpr uint32_t kDecTentBad = 1u << 16;

// Message vtable slots (WorldQLFB_generated.rs:939-947), Record / Entity (:485-489, :704-708)
enum : uint32_t { kDmInstr = 4, kDmParam = 6, kDmSender = 8, kDmWorld = 10, kDmRepl = 12, kDmRecords = 14,
                  kDmEntities = 16, kDmPos = 18, kDmFlex = 20 };
enum : uint32_t { kDrUuid = 4, kDrPos = 6, kDrWorld = 8, kDrData = 10, kDrFlex = 12 };

// A listed long string: where it starts in the frame bytes, its frame and its length.
struct DecEntry {
    uint64_t start;
    uint32_t frame, len;
};

struct DecList {
    DecEntry* e;
    uint32_t* count;  // entries appended; may pass cap by the lanes that raced for the last slots
    uint32_t cap;
};

// The handle's two tables. Worlds: the names of wq_frames_set_worlds, and their ids ordered by
// (hash of the name, id). Senders: the uuids as two big-endian u64 in ascending order, and their ids.
struct DecTables {
    const uint8_t* world_bytes;
    const uint32_t* world_off;
    const uint64_t* world_hash;
    const uint32_t* world_id;
    const uint64_t* peer_hi;
    const uint64_t* peer_lo;
    const uint32_t* peer_id;
    uint32_t n_worlds, n_peers;
};

// ---- the reader: b[0 .. n), every access below a range check -----------------------------------
struct DecV {
    const uint8_t* b;
    uint64_t n;
    uint64_t apparent;
    uint32_t tables;
    int depth;
    bool ok;
    DecList list;
    uint64_t base;   // the frame's first byte in the frame bytes
    uint32_t frame;

    WQ_DEC_HD bool fail() { return ok = false; }
    WQ_DEC_HD bool aligned(uint64_t pos, uint64_t a) { return (pos % a == 0) || fail(); }
    WQ_DEC_HD bool range(uint64_t pos, uint64_t size) {
        if (pos + size > n) return fail();
        apparent += size;
        if (apparent > kDecMaxApparent) return fail();
        return true;
    }
    WQ_DEC_HD uint32_t rd16(uint64_t p) const { return (uint32_t)b[p] | ((uint32_t)b[p + 1] << 8); }
    WQ_DEC_HD uint32_t rd32(uint64_t p) const {
        return (uint32_t)b[p] | ((uint32_t)b[p + 1] << 8) | ((uint32_t)b[p + 2] << 16) | ((uint32_t)b[p + 3] << 24);
    }
    WQ_DEC_HD uint64_t rd64(uint64_t p) const { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }
    WQ_DEC_HD bool u32_at(uint64_t pos, uint32_t* v) {
        if (!aligned(pos, 4) || !range(pos, 4)) return false;
        *v = rd32(pos);
        return true;
    }
    WQ_DEC_HD bool u16_at(uint64_t pos, uint32_t* v) {
        if (!aligned(pos, 2) || !range(pos, 2)) return false;
        *v = rd16(pos);
        return true;
    }
    WQ_DEC_HD bool follow(uint64_t pos, uint64_t* out) {
        uint32_t off;
        if (!u32_at(pos, &off)) return false;
        *out = pos + off;
        return true;
    }
    WQ_DEC_HD bool vec_range(uint64_t pos, uint64_t elem, uint64_t* start, uint64_t* len) {
        uint32_t l;
        if (!u32_at(pos, &l)) return false;
        const uint64_t s = pos + 4;
        if (!aligned(s, elem)) return false;
        if (!range(s, (uint64_t)l * elem)) return false;
        *start = s;
        *len = l;
        return true;
    }
};

// Rust std::str::from_utf8 acceptance of the sequences that start in s[from .. until) of the string
// s[0 .. len): no overlongs, no surrogates, <= U+10FFFF; a sequence may end behind `until`, never behind
// `len`. (0, len) is the whole string.
WQ_DEC_HD bool dec_utf8_range(const uint8_t* s, uint64_t len, uint64_t from, uint64_t until) {
    uint64_t i = from;
    while (i < until) {
        const uint8_t c = s[i];
        if (c < 0x80) {
            ++i;
            continue;
        }
        uint64_t k;
        uint8_t lo = 0x80, hi = 0xBF;
        if (c >= 0xC2 && c <= 0xDF) k = 1;
        else if (c == 0xE0) { k = 2; lo = 0xA0; }
        else if ((c >= 0xE1 && c <= 0xEC) || c == 0xEE || c == 0xEF) k = 2;
        else if (c == 0xED) { k = 2; hi = 0x9F; }
        else if (c == 0xF0) { k = 3; lo = 0x90; }
        else if (c >= 0xF1 && c <= 0xF3) k = 3;
        else if (c == 0xF4) { k = 3; hi = 0x8F; }
        else return false;
        if (i + k >= len) return false;  // truncated by the string's end
        if (s[i + 1] < lo || s[i + 1] > hi) return false;
        for (uint64_t j = 2; j <= k; ++j)
            if (s[i + j] < 0x80 || s[i + j] > 0xBF) return false;
        i += k + 1;
    }
    return true;
}

// One chunk [c0, c1) of a string: the sequence that holds byte c0 starts at most 3 bytes before it (a
// fourth continuation byte in a row belongs to no sequence), and the check runs from there. The string
// is valid exactly when every chunk is: a lead or ASCII byte always starts a sequence, and a
// continuation byte is reached by the check of the chunk that holds its lead, or refused here.
WQ_DEC_HD bool dec_utf8_chunk(const uint8_t* s, uint64_t len, uint64_t c0, uint64_t c1) {
    uint64_t from = c0;
    for (uint32_t back = 0; from > 0 && (s[from] & 0xC0) == 0x80; ++back) {
        if (back == 3) return false;
        --from;
    }
    return dec_utf8_range(s, len, from, c1);
}

WQ_DEC_HD bool dec_list_push(DecV& v, uint64_t start, uint64_t len) {
    const DecList& l = v.list;
    if (!l.cap || *l.count >= l.cap) return false;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t k = atomicAdd(l.count, 1u);
    if (k >= l.cap) return false;
#else
    const uint32_t k = (*l.count)++;
#endif
    l.e[k].start = v.base + start;
    l.e[k].frame = v.frame;
    l.e[k].len = (uint32_t)len;
    return true;
}

struct DecStr {
    bool present;
    uint32_t off, len;
};

// &str: a vector of u8, UTF-8, a NUL right behind it
WQ_DEC_HD bool dec_verify_str(DecV& v, uint64_t pos, DecStr* s) {
    uint64_t start, len;
    if (!v.aligned(pos, 4) || !v.vec_range(pos, 1, &start, &len)) return false;
    if (len <= kDecLane || !dec_list_push(v, start, len)) {
        if (!dec_utf8_range(v.b + start, len, 0, len)) return v.fail();
    }
    const uint64_t end = start + len;
    if (end >= v.n || v.b[end] != 0) return v.fail();
    s->present = true;
    s->off = (uint32_t)start;
    s->len = (uint32_t)len;
    return true;
}

struct DecTable {
    uint64_t pos, vt, vt_len;
};

WQ_DEC_HD bool dec_visit_table(DecV& v, uint64_t pos, DecTable* t) {
    if (++v.tables > kDecMaxTables) return v.fail();
    uint32_t raw;
    if (!v.u32_at(pos, &raw)) return false;
    const int32_t so = (int32_t)raw;
    uint64_t vt;
    if (so > 0) {  // the vtable precedes the table
        if ((uint64_t)so > pos) return v.fail();
        vt = pos - (uint64_t)so;
    } else {
        vt = pos + (uint64_t)(-(int64_t)so);
    }
    if (vt >= v.n) return v.fail();
    uint32_t vl;
    if (!v.u16_at(vt, &vl)) return false;
    if (!v.aligned(vt + vl, 2) || !v.range(vt, vl)) return false;
    if (++v.depth > (int)kDecMaxDepth) return v.fail();
    t->pos = pos;
    t->vt = vt;
    t->vt_len = vl;
    return true;
}

WQ_DEC_HD bool dec_field(DecV& v, const DecTable& t, uint64_t voff, uint64_t* fpos) {
    *fpos = 0;
    if (voff < t.vt_len) {
        uint32_t fo;
        if (!v.u16_at(t.vt + voff, &fo)) return false;
        if (fo > 0) *fpos = t.pos + fo;
    }
    return true;
}

WQ_DEC_HD bool dec_field_str(DecV& v, const DecTable& t, uint64_t voff, DecStr* s) {
    uint64_t fp, sp;
    if (!dec_field(v, t, voff, &fp)) return false;
    if (!fp) return true;
    return v.follow(fp, &sp) && dec_verify_str(v, sp, s);
}

WQ_DEC_HD bool dec_field_u8(DecV& v, const DecTable& t, uint64_t voff, uint8_t* out) {
    uint64_t fp;
    if (!dec_field(v, t, voff, &fp)) return false;
    *out = 0;
    if (!fp) return true;
    if (!v.range(fp, 1)) return false;
    *out = v.b[fp];
    return true;
}

// Vec3d is [u8; 24], alignment 1: *at is where it lies, 0 when absent
WQ_DEC_HD bool dec_field_vec3(DecV& v, const DecTable& t, uint64_t voff, bool* has, uint64_t* at) {
    uint64_t fp;
    if (!dec_field(v, t, voff, &fp)) return false;
    *has = false;
    *at = 0;
    if (!fp) return true;
    if (!v.range(fp, 24)) return false;
    *has = true;
    *at = fp;
    return true;
}

WQ_DEC_HD bool dec_field_bytes(DecV& v, const DecTable& t, uint64_t voff, DecStr* s) {
    uint64_t fp, vp, st, l;
    if (!dec_field(v, t, voff, &fp)) return false;
    if (!fp) return true;
    if (!(v.follow(fp, &vp) && v.aligned(vp, 4) && v.vec_range(vp, 1, &st, &l))) return false;
    s->present = true;
    s->off = (uint32_t)st;
    s->len = (uint32_t)l;
    return true;
}

// ---- uuid 0.8.2 Uuid::parse_str: simple, hyphenated, urn:uuid: ---------------------------------
WQ_DEC_HD int dec_hexv(uint8_t c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

WQ_DEC_HD uint32_t dec_group_end(int g) { return g == 0 ? 8u : g == 1 ? 12u : g == 2 ? 16u : g == 3 ? 20u : 32u; }

WQ_DEC_HD bool dec_parse_uuid(const uint8_t* s, uint32_t len, uint8_t out[16]) {
    if (len == 45 && s[0] == 'u' && s[1] == 'r' && s[2] == 'n' && s[3] == ':' && s[4] == 'u' && s[5] == 'u' &&
        s[6] == 'i' && s[7] == 'd' && s[8] == ':') {
        s += 9;
        len -= 9;
    } else if (len != 32 && len != 36) {
        return false;
    }
    int digit = 0, group = 0;
    uint8_t acc = 0;
    for (uint32_t i = 0; i < len; ++i) {
        const uint8_t c = s[i];
        if (digit >= 32 && group != 4) return false;
        const int h = dec_hexv(c);
        if (digit % 2 == 0) {
            if (h >= 0) {
                acc = (uint8_t)h;
            } else if (c == '-') {
                if (group > 4 || dec_group_end(group) != (uint32_t)digit) return false;
                ++group;
                --digit;
            } else {
                return false;
            }
        } else {
            if (h < 0) return false;
            acc = (uint8_t)(acc * 16 + h);
            out[digit / 2] = acc;
        }
        ++digit;
    }
    return digit == 32;
}

// ---- Record / Entity, and a vector of them -------------------------------------------------------
WQ_DEC_HD bool dec_record_like(DecV& v, uint64_t pos, bool entity, int* dec) {
    DecTable t;
    if (!dec_visit_table(v, pos, &t)) return false;
    DecStr uuid{false, 0, 0}, world{false, 0, 0}, data{false, 0, 0}, flex{false, 0, 0};
    bool has_pos;
    uint64_t at;
    if (!dec_field_str(v, t, kDrUuid, &uuid) || !dec_field_vec3(v, t, kDrPos, &has_pos, &at) ||
        !dec_field_str(v, t, kDrWorld, &world) || !dec_field_str(v, t, kDrData, &data) ||
        !dec_field_bytes(v, t, kDrFlex, &flex))
        return false;
    --v.depth;
    if (*dec != WQ_DEC_OK) return true;  // the first decode error wins
    if (!uuid.present || (entity && !has_pos) || !world.present) {
        *dec = WQ_DEC_MISSING_FIELD;
        return true;
    }
    uint8_t u[16];
    if (!dec_parse_uuid(v.b + uuid.off, uuid.len, u)) *dec = WQ_DEC_BAD_UUID;
    return true;
}

// The loop is bounded by the frame: vec_range has placed all 4 * len bytes inside it.
WQ_DEC_HD bool dec_table_vector(DecV& v, const DecTable& t, uint64_t voff, bool entity, uint32_t* count, int* dec) {
    uint64_t fp, vp, start, len;
    *count = 0;
    if (!dec_field(v, t, voff, &fp)) return false;
    if (!fp) return true;
    if (!v.follow(fp, &vp) || !v.aligned(vp, 4) || !v.vec_range(vp, 4, &start, &len)) return false;
    for (uint64_t i = 0; i < len; ++i) {
        uint64_t rp;
        if (!v.follow(start + 4 * i, &rp) || !dec_record_like(v, rp, entity, dec)) return false;
    }
    *count = (uint32_t)len;
    return true;
}

// What the walk leaves of one frame: the struct of wq_decode_messages and the flex range it lacks.
struct DecFrame {
    wq_decoded_msg m;
    uint32_t flex_off, flex_len;
    bool has_flex;
};

// decode_one (wq_codec.cpp) of b[0 .. n).
WQ_DEC_HD void dec_frame(const uint8_t* b, uint64_t n, const DecList& list, uint64_t base, uint32_t frame, DecFrame* o) {
    memset(o, 0, sizeof(*o));
    DecV v{b, n, 0, 0, 0, true, list, base, frame};
    DecTable t;
    uint64_t root, pos_at = 0;
    DecStr param{false, 0, 0}, sender{false, 0, 0}, world{false, 0, 0}, flex{false, 0, 0};
    uint8_t instr = 0, repl = 0;
    bool has_pos = false;
    uint32_t nrec = 0, nent = 0;
    int rec_dec = WQ_DEC_OK, ent_dec = WQ_DEC_OK;
    bool verified = v.follow(0, &root) && dec_visit_table(v, root, &t) && dec_field_u8(v, t, kDmInstr, &instr) &&
                    dec_field_str(v, t, kDmParam, &param) && dec_field_str(v, t, kDmSender, &sender) &&
                    dec_field_str(v, t, kDmWorld, &world) && dec_field_u8(v, t, kDmRepl, &repl);
    // records, then entities: one body for both vectors, so the Record / Entity walk is compiled once
#pragma nounroll
    for (int pass = 0; verified && pass < 2; ++pass) {
        uint32_t count = 0;
        int dec = WQ_DEC_OK;
        verified = dec_table_vector(v, t, pass ? kDmEntities : kDmRecords, pass != 0, &count, &dec);
        if (pass) nent = count, ent_dec = dec;
        else nrec = count, rec_dec = dec;
    }
    verified = verified && dec_field_vec3(v, t, kDmPos, &has_pos, &pos_at) && dec_field_bytes(v, t, kDmFlex, &flex);
    if (!verified || !v.ok) {
        o->m.status = WQ_DEC_INVALID_FLATBUFFER;
        return;
    }
    if (!world.present || !sender.present) {
        o->m.status = WQ_DEC_MISSING_FIELD;
        return;
    }
    if (rec_dec != WQ_DEC_OK) {
        o->m.status = rec_dec;
        return;
    }
    if (ent_dec != WQ_DEC_OK) {
        o->m.status = ent_dec;
        return;
    }
    uint8_t u[16];
    if (!dec_parse_uuid(b + sender.off, sender.len, u)) {
        o->m.status = WQ_DEC_BAD_UUID;
        return;
    }
    for (int k = 0; k < 16; ++k) o->m.sender_uuid[k] = u[k];
    o->m.status = WQ_DEC_OK;
    o->m.instruction = instr <= 12 ? instr : (uint8_t)WQ_INSTR_UNKNOWN;
    o->m.replication = repl <= 2 ? repl : 0;
    o->m.has_position = has_pos ? 1 : 0;
    o->m.has_parameter = param.present ? 1 : 0;
    if (has_pos) {
        for (int k = 0; k < 3; ++k) {  // the bits as they lie, NaN payloads included
            const uint64_t w = v.rd64(pos_at + 8 * k);
            memcpy(&o->m.position[k], &w, 8);
        }
    }
    o->m.world_off = world.off;
    o->m.world_len = world.len;
    o->m.param_off = param.off;
    o->m.param_len = param.len;
    o->m.n_records = nrec;
    o->m.n_entities = nent;
    o->has_flex = flex.present;
    o->flex_off = flex.present ? flex.off : 0;
    o->flex_len = flex.present ? flex.len : 0;
}

// Frame i of the batch of n: true with its first byte and size, or false with an error bit. An offset is
// suspect when it lies past n_frame_bytes or stands in a descending pair (either side may be the wrong
// one); a frame with a suspect offset — its own pair descends or reaches past the end, or a neighbour's
// does at the offset they share — cannot be told from its neighbours: bit 0. 2^32 bytes or more: bit 1.
// Only fo[i - 1 .. i + 2], clipped to [0, n], are read.
WQ_DEC_HD bool dec_frame_span(const uint64_t* __restrict__ fo, uint64_t i, uint64_t n, uint64_t n_frame_bytes,
                              uint64_t* lo, uint64_t* size, uint32_t* err) {
    const uint64_t a = fo[i], b = fo[i + 1];
    *lo = 0;
    *size = 0;
    bool suspect = a > b || b > n_frame_bytes;  // a <= b <= n_frame_bytes below
    if (!suspect && i > 0) suspect = fo[i - 1] > a;
    if (!suspect && i + 1 < n) suspect = b > fo[i + 2];
    if (suspect) {
        *err |= kDecErrOffsets;
        return false;
    }
    if (b - a >= (1ull << 32)) {
        *err |= kDecErrHuge;
        return false;
    }
    *lo = a;
    *size = b - a;
    return true;
}

// ---- worlds -------------------------------------------------------------------------------------
constexpr uint64_t kDecFnvBasis = 0xCBF29CE484222325ull, kDecFnvPrime = 0x100000001B3ull;
WQ_DEC_HD uint64_t dec_fnv(uint64_t h, uint8_t c) { return (h ^ c) * kDecFnvPrime; }

// The bytes wq_sanitize_world_name writes for one accepted byte: out[0 .. return value)
WQ_DEC_HD uint32_t dec_san_expand(uint8_t c, uint8_t out[4]) {
    const uint8_t mid0 = c == '/' ? 'f' : c == '\\' ? 'b' : c == ':' ? 'c' : 'a';
    const uint8_t mid1 = c == '/' ? 's' : c == '\\' ? 's' : c == ':' ? 'l' : 't';
    if (c == '/' || c == '\\' || c == ':' || c == '@') {
        out[0] = '_', out[1] = mid0, out[2] = mid1, out[3] = '_';
        return 4;
    }
    out[0] = c == ' ' ? (uint8_t)'_' : c;
    return 1;
}

WQ_DEC_HD bool dec_san_alpha(uint8_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }

// wq_sanitize_world_name's verdict on name[0 .. len) without its output: 0 with the sanitized length
// and hash, or the WQ_SAN_* error, in its order of checks.
WQ_DEC_HD int dec_sanitize(const uint8_t* name, uint32_t len, uint32_t* out_len, uint64_t* hash) {
    if (len == 7 && name[0] == '@' && name[1] == 'g' && name[2] == 'l' && name[3] == 'o' && name[4] == 'b' &&
        name[5] == 'a' && name[6] == 'l')
        return WQ_SAN_IS_GLOBAL_WORLD;
    if (len == 0) return WQ_SAN_ZERO_LENGTH;
    if (!dec_san_alpha(name[0])) return WQ_SAN_INVALID_START;
    // an accepted byte gives at least one output byte: above 63 input bytes the host answers InvalidChars
    // or TooLong, the table is not asked either way, and the name (it may be megabytes) is not scanned
    if (len > 63) return WQ_SAN_TOO_LONG;
    uint32_t outn = 0;
    uint64_t h = kDecFnvBasis;
    for (uint32_t i = 0; i < len; ++i) {
        const uint8_t c = name[i];
        if (!(dec_san_alpha(c) || (c >= '0' && c <= '9') || c == '_' || c == ' ' || c == '/' || c == '\\' || c == ':' ||
              c == '@'))
            return WQ_SAN_INVALID_CHARS;
        uint8_t e[4];
        const uint32_t k = dec_san_expand(c, e);
        for (uint32_t j = 0; j < k; ++j) h = dec_fnv(h, e[j]);
        outn += k;
    }
    if (outn > 63) return WQ_SAN_TOO_LONG;
    *out_len = outn;
    *hash = h;
    return 0;
}

// Does the sanitized form of name[0 .. len) equal want[0 .. want_len)? (want_len is its length already.)
WQ_DEC_HD bool dec_san_equals(const uint8_t* name, uint32_t len, const uint8_t* want) {
    uint32_t k = 0;
    for (uint32_t i = 0; i < len; ++i) {
        uint8_t e[4];
        const uint32_t m = dec_san_expand(name[i], e);
        for (uint32_t j = 0; j < m; ++j)
            if (want[k++] != e[j]) return false;
    }
    return true;
}

// The world id of a decoded name: WQ_WORLD_GLOBAL for "@global", the lowest id whose table name is the
// sanitized name, else WQ_WORLD_INVALID. *bits gets kDecGlobal or kDecWorldKnown.
WQ_DEC_HD uint32_t dec_world(const uint8_t* name, uint32_t len, const DecTables& t, uint32_t* bits) {
    uint32_t outn = 0;
    uint64_t h = 0;
    const int rc = dec_sanitize(name, len, &outn, &h);
    if (rc == WQ_SAN_IS_GLOBAL_WORLD) {
        *bits |= kDecGlobal;
        return WQ_WORLD_GLOBAL;
    }
    if (rc != 0 || t.n_worlds == 0) return WQ_WORLD_INVALID;
    uint32_t lo = 0, hi = t.n_worlds;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t.world_hash[mid] < h) lo = mid + 1;
        else hi = mid;
    }
    for (uint32_t j = lo; j < t.n_worlds && t.world_hash[j] == h; ++j) {  // ids ascend inside one hash
        const uint32_t w = t.world_id[j];
        const uint32_t a = t.world_off[w], b = t.world_off[w + 1];
        if (b - a == outn && dec_san_equals(name, len, t.world_bytes + a)) {
            *bits |= kDecWorldKnown;
            return w;
        }
    }
    return WQ_WORLD_INVALID;
}

// ---- senders ------------------------------------------------------------------------------------
WQ_DEC_HD uint64_t dec_be64(const uint8_t* p) {
    uint64_t v = 0;
    for (int k = 0; k < 8; ++k) v = (v << 8) | p[k];
    return v;
}

WQ_DEC_HD uint32_t dec_sender(const uint8_t u[16], const DecTables& t, uint32_t* bits) {
    const uint64_t kh = dec_be64(u), kl = dec_be64(u + 8);
    uint32_t lo = 0, hi = t.n_peers;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint64_t mh = t.peer_hi[mid], ml = t.peer_lo[mid];
        if (mh < kh || (mh == kh && ml < kl)) lo = mid + 1;
        else hi = mid;
    }
    if (lo < t.n_peers && t.peer_hi[lo] == kh && t.peer_lo[lo] == kl) {
        *bits |= kDecSenderKnown;
        return t.peer_id[lo];
    }
    return kDecNoPeer;
}

// ---- the passes, one frame or one chunk at a time ---------------------------------------------------
// Writes frame i's outputs (each nullable) from its struct: the frame's own fields for an OK frame,
// zeros with world WQ_WORLD_INVALID and sender kDecNoPeer otherwise.
WQ_DEC_HD void dec_store(const wq_ingest_out& out, uint64_t i, const DecFrame& f, uint32_t world, uint32_t sender,
                         uint32_t flags) {
    if (out.msg) out.msg[i] = f.m;
    if (out.pos)
        for (int k = 0; k < 3; ++k) out.pos[3 * i + k] = f.m.position[k];
    if (out.world) out.world[i] = world;
    if (out.sender) out.sender[i] = sender;
    if (out.repl) out.repl[i] = f.m.replication;
    if (out.instruction) out.instruction[i] = f.m.instruction;
    if (out.sender_uuid)
        for (int k = 0; k < 16; ++k) out.sender_uuid[16 * i + k] = f.m.sender_uuid[k];
    if (out.flex_range) out.flex_range[2 * i] = f.flex_off, out.flex_range[2 * i + 1] = f.flex_len;
    if (out.flags) out.flags[i] = (uint8_t)flags;
}

// The walk of frame i. Returns the frame's word for the later passes; *err gets the offset error bits.
WQ_DEC_HD uint32_t dec_walk(const uint8_t* __restrict__ frames, const uint64_t* __restrict__ fo, uint64_t i, uint64_t n,
                            uint64_t n_frame_bytes, const DecList& list, const DecTables& t, const wq_ingest_out& out,
                            uint32_t* err) {
    DecFrame f;
    uint64_t lo, size;
    if (dec_frame_span(fo, i, n, n_frame_bytes, &lo, &size, err)) {
        dec_frame(frames + lo, size, list, lo, (uint32_t)i, &f);
    } else {
        memset(&f, 0, sizeof(f));
        f.m.status = WQ_DEC_INVALID_FLATBUFFER;
    }
    uint32_t flags = 0, world = WQ_WORLD_INVALID, sender = kDecNoPeer;
    if (f.m.status == WQ_DEC_OK) {
        flags = kDecOk | (f.m.has_position ? kDecHasPos : 0u) | (f.m.has_parameter ? kDecHasParam : 0u) |
                (f.has_flex ? kDecHasFlex : 0u);
        world = dec_world(frames + lo + f.m.world_off, f.m.world_len, t, &flags);
        sender = dec_sender(f.m.sender_uuid, t, &flags);
    }
    dec_store(out, i, f, world, sender, flags);
    return flags | ((uint32_t)f.m.status << 8);
}

// The strings pass on chunk [c0, c0 + kDecChunk) of one listed string.
WQ_DEC_HD bool dec_entry_chunk_ok(const uint8_t* __restrict__ frames, const DecEntry& e, uint64_t c0) {
    const uint64_t c1 = e.len - c0 > kDecChunk ? c0 + kDecChunk : e.len;
    return dec_utf8_chunk(frames + e.start, e.len, c0, c1);
}

// The finish of frame i from its word: a frame the strings pass refused becomes the verifier's failure.
// Returns the final word (flags, status).
WQ_DEC_HD uint32_t dec_finish(uint32_t word, uint64_t i, const wq_ingest_out& out) {
    if (!(word & kDecTentBad)) return word;
    DecFrame f;
    memset(&f, 0, sizeof(f));
    f.m.status = WQ_DEC_INVALID_FLATBUFFER;
    dec_store(out, i, f, WQ_WORLD_INVALID, kDecNoPeer, 0);
    return (uint32_t)WQ_DEC_INVALID_FLATBUFFER << 8;
}

// The six counters a final word adds to: {ok, invalid, missing, bad uuid, world unresolved, sender unknown}
WQ_DEC_HD void dec_count(uint32_t word, uint32_t c[6]) {
    const uint32_t status = (word >> 8) & 3u;
    c[status] += 1;
    if (status == WQ_DEC_OK) {
        if (!(word & (kDecGlobal | kDecWorldKnown))) c[4] += 1;
        if (!(word & kDecSenderKnown)) c[5] += 1;
    }
}

// ---- the tables' host side ----------------------------------------------------------------------------
inline uint64_t dec_hash_name(const uint8_t* s, size_t n) {
    uint64_t h = kDecFnvBasis;
    for (size_t i = 0; i < n; ++i) h = dec_fnv(h, s[i]);
    return h;
}

// The lookup order of a world table: ids by (hash of the name, id).
inline void dec_world_index(const uint8_t* names, const uint32_t* off, uint32_t n, std::vector<uint64_t>* hash,
                            std::vector<uint32_t>* id) {
    std::vector<uint64_t> h(n);
    for (uint32_t w = 0; w < n; ++w) h[w] = dec_hash_name(names + off[w], off[w + 1] - off[w]);
    id->resize(n);
    std::iota(id->begin(), id->end(), 0u);
    std::sort(id->begin(), id->end(), [&](uint32_t a, uint32_t b) { return h[a] != h[b] ? h[a] < h[b] : a < b; });
    hash->resize(n);
    for (uint32_t k = 0; k < n; ++k) (*hash)[k] = h[(*id)[k]];
}

// The sorted sender table; false when a uuid occurs twice. ids == nullptr: id = index.
inline bool dec_peer_index(const uint8_t* uuids, const uint32_t* ids, uint32_t n, std::vector<uint64_t>* hi,
                           std::vector<uint64_t>* lo, std::vector<uint32_t>* id) {
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    auto key = [&](uint32_t k, int half) { return dec_be64(uuids + 16 * (size_t)k + 8 * half); };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const uint64_t ah = key(a, 0), bh = key(b, 0);
        return ah != bh ? ah < bh : key(a, 1) < key(b, 1);
    });
    hi->resize(n), lo->resize(n), id->resize(n);
    for (uint32_t k = 0; k < n; ++k) {
        (*hi)[k] = key(order[k], 0), (*lo)[k] = key(order[k], 1);
        (*id)[k] = ids ? ids[order[k]] : order[k];
        if (k && (*hi)[k] == (*hi)[k - 1] && (*lo)[k] == (*lo)[k - 1]) return false;
    }
    return true;
}

}  // namespace wq
