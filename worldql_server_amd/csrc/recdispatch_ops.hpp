// recdispatch_ops.hpp — the arithmetic of the record dispatch (include/wq_router.h, "record dispatch";
// kernels: wq_recdispatch.hip). Everything the kernels compute is here, in functions that are
// __host__ __device__, so tests/cpp/records_dispatch_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/ingest.py (records_dispatch_np), which is the definition.
//
//   rd_parse_after      Rust's u64::from_str and chrono's range check (utils/time.rs:6-16), digit by digit.
//   rd_frame_eval       a listed frame's class, its `after`, and where its records vector lies: the bounded
//                       reader of decode_ops.hpp from the root table to the vector's length word.
//   rd_record           one record of an APPLY frame: the walk over its table, the drop rules of
//                       database/client.rs:86-111 / :365-379, the world lookup and rec_pack_position.
//   rd_frame_of         the listed frame whose records hold ordinal q: a search in the exclusive prefix of
//                       the frames' record counts.
//   rd_before           the accepted (or deferred) records before an ordinal, from the granules' prefix
//                       and flag words.
//   RdSum, RdCombine    what a stretch of listed frames adds up to: ops, query rows, deferred entries, its
//                       first deferred frame, and what it does to RecordProcessor.process's two batches: the
//                       kinds it closes before its first effective frame, that frame's kind, the run left
//                       open and the run starts behind it. Associative: one scan carries rows and runs
//                       together, as the dispatch's DspSum does.
//   rd_emit_op, rd_emit_frame, rd_finish   an op and its reference, a frame's query row, deferred entry
//                       and run entry, the closing run and the counters.
#pragma once

#include "decode_ops.hpp"
#include "dispatch_ops.hpp"
#include "record_ops.hpp"

namespace wq {

#define WQ_RD_HD __host__ __device__ __forceinline__

constexpr uint32_t kRdGranule = 64;                // records per flag word: one wave
constexpr uint64_t kRdMaxRecords = 0xFFFFFFC0ull;  // max_records stays below: an ordinal is a u32
constexpr uint32_t kRdErrWalk = 1u, kRdErrList = 2u;  // wq_recdisp_counters.error bits 0 and 1
constexpr uint32_t kRdOvOps = 1u, kRdOvDefer = 2u, kRdOvRuns = 4u, kRdOvRecords = 8u;  // .overflow bits
constexpr uint64_t kRdMaxSeconds = 8210298412799ull;  // chrono 0.4 NaiveDateTime::from_timestamp_opt's last second
constexpr uint32_t kRdNone = 0xFFFFFFFFu;
constexpr uint32_t kRdWords = 3;  // flag words per granule: accepted, deferred, accepted creates

// What a record comes to; the first four are the counters' drop reasons in their order.
enum : uint32_t { kRdFail = 0, kRdNoPos = 1, kRdBadWorld = 2, kRdUnpackable = 3, kRdDefer = 4, kRdAccept = 5 };

// u64::from_str: an optional '+', then digits only, below 2^64; then ms / 1000 within chrono's range.
// The leading zeros are the only long walk (s is bounded by the frame); the significant digits stop at 20.
WQ_RD_HD bool rd_parse_after(const uint8_t* s, uint32_t len, int64_t* out) {
    uint32_t i = (len && s[0] == '+') ? 1u : 0u;
    if (i == len) return false;
    while (i < len && s[i] == '0') ++i;
    uint64_t v = 0;
    uint32_t digits = 0;
    for (; i < len; ++i) {
        const uint32_t d = (uint32_t)s[i] - (uint32_t)'0';
        if (d > 9 || ++digits > 20) return false;
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    if (v / 1000 > kRdMaxSeconds) return false;
    *out = (int64_t)(v * 1000);
    return true;
}

WQ_RD_HD DecV rd_reader(const uint8_t* b, uint64_t n) { return DecV{b, n, 0, 0, 0, true, DecList{nullptr, nullptr, 0}, 0, 0}; }

// Listed entry j: its frame index, and with true the frame's first byte and size. A frame index that is
// not above its predecessor's or not below n_frames raises kRdErrList, offsets the decoder would refuse
// kRdErrWalk. Reads db_src[j - 1 .. j] and frame_offsets[f - 1 .. f + 2], clipped.
WQ_RD_HD bool rd_frame_span(const wq_recdisp_in& in, uint64_t j, uint32_t* f, uint64_t* lo, uint64_t* size, uint32_t* err) {
    *f = in.db_src ? in.db_src[j] : (uint32_t)j;
    *lo = *size = 0;
    if (in.db_src && j > 0 && in.db_src[j - 1] >= *f) *err |= kRdErrList;
    if (*f >= in.n_frames) {
        *err |= kRdErrList;
        return false;
    }
    uint32_t e = 0;
    if (!dec_frame_span(in.frame_offsets, *f, in.n_frames, in.n_frame_bytes, lo, size, &e)) {
        *err |= kRdErrWalk;
        return false;
    }
    return true;
}

// Where Message.records lies in the frame b[0 .. n): the first slot and the count, 0, 0 when absent.
WQ_RD_HD bool rd_records_vector(const uint8_t* b, uint64_t n, uint32_t* start, uint32_t* count) {
    DecV v = rd_reader(b, n);
    DecTable t;
    uint64_t root, fp, vp, s, len;
    *start = *count = 0;
    if (!(v.follow(0, &root) && dec_visit_table(v, root, &t) && dec_field(v, t, kDmRecords, &fp))) return false;
    if (!fp) return true;
    if (!(v.follow(fp, &vp) && v.aligned(vp, 4) && v.vec_range(vp, 4, &s, &len))) return false;
    *start = (uint32_t)s;
    *count = (uint32_t)len;
    return true;
}

struct RdFrameRes {
    uint32_t cls, f, count, vec;  // WQ_RCLS_*, the frame index, an APPLY frame's records and their first slot
    int64_t after;                // a READ frame's `after`
    uint32_t err;
};

// Listed entry j (the header's frame rules, in their order).
WQ_RD_HD RdFrameRes rd_frame_eval(const wq_recdisp_in& in, uint64_t j) {
    RdFrameRes r{WQ_RCLS_SKIP, 0, 0, 0, INT64_MIN, 0};
    uint64_t lo, size;
    if (!rd_frame_span(in, j, &r.f, &lo, &size, &r.err)) return r;
    const uint32_t flags = in.flags[r.f];
    if (!(flags & kDecOk) || (flags & kDecGlobal)) return r;
    const wq_decoded_msg& m = in.msg[r.f];
    const uint32_t ins = m.instruction;
    const uint8_t* b = in.frames + lo;
    if (ins == kInsRecordCreate || ins == kInsRecordDelete) {
        r.cls = WQ_RCLS_APPLY;
        if (!rd_records_vector(b, size, &r.vec, &r.count)) r.err |= kRdErrWalk;
        return r;
    }
    if (ins != kInsRecordRead) return r;
    r.cls = WQ_RCLS_READ_DROPPED;
    if (!(flags & kDecHasPos)) return r;
    if (flags & kDecHasParam) {
        if ((uint64_t)m.param_off + m.param_len > size) {
            r.err |= kRdErrWalk;
            return r;
        }
        if (!rd_parse_after(b + m.param_off, m.param_len, &r.after)) return r;
    }
    if ((uint64_t)m.world_off + m.world_len > size) {
        r.err |= kRdErrWalk;
        return r;
    }
    uint32_t outn;
    uint64_t hash;
    if (dec_sanitize(b + m.world_off, m.world_len, &outn, &hash) != 0) return r;
    r.cls = (flags & kDecWorldKnown) && in.world[r.f] < WQ_WORLD_GLOBAL ? WQ_RCLS_READ : WQ_RCLS_READ_DEFERRED;
    return r;
}

struct RdRec {
    uint32_t status, world;
    uint64_t pos[3], uuid_hi, uuid_lo;  // the position's bits as they lie
    uint32_t data_off, data_len, flex_off, flex_len, bits;  // bits: 1 data present, 2 flex present
};

// Record r of the vector at `vec` in the frame b[0 .. n).
WQ_RD_HD RdRec rd_record(const uint8_t* b, uint64_t n, uint32_t vec, uint32_t r, const DecTables& tables, const RecCfg& cfg) {
    RdRec o;
    memset(&o, 0, sizeof(o));
    o.status = kRdFail;
    DecV v = rd_reader(b, n);
    DecTable t;
    uint64_t rp, at;
    DecStr uuid{false, 0, 0}, world{false, 0, 0}, data{false, 0, 0}, flex{false, 0, 0};
    bool has_pos;
    if (!(v.follow((uint64_t)vec + 4ull * r, &rp) && dec_visit_table(v, rp, &t) && dec_field_bytes(v, t, kDrUuid, &uuid) &&
          dec_field_vec3(v, t, kDrPos, &has_pos, &at) && dec_field_bytes(v, t, kDrWorld, &world) &&
          dec_field_bytes(v, t, kDrData, &data) && dec_field_bytes(v, t, kDrFlex, &flex)))
        return o;
    uint8_t u[16];
    if (!uuid.present || !world.present || !dec_parse_uuid(b + uuid.off, uuid.len, u)) return o;
    o.uuid_hi = dec_be64(u), o.uuid_lo = dec_be64(u + 8);
    o.data_off = data.off, o.data_len = data.len, o.flex_off = flex.off, o.flex_len = flex.len;
    o.bits = (data.present ? 1u : 0u) | (flex.present ? 2u : 0u);
    if (!has_pos) {  // insert_records / delete_records: no position, no row
        o.status = kRdNoPos;
        return o;
    }
    uint32_t outn, found = 0;
    uint64_t hash;
    if (dec_sanitize(b + world.off, world.len, &outn, &hash) != 0) {  // "@global" is IsGlobalWorld here
        o.status = kRdBadWorld;
        return o;
    }
    o.world = dec_world(b + world.off, world.len, tables, &found);
    if (!(found & kDecWorldKnown)) {
        o.status = kRdDefer;
        return o;
    }
    double p[3];
    for (int k = 0; k < 3; ++k) {
        o.pos[k] = v.rd64(at + 8 * k);
        memcpy(&p[k], &o.pos[k], 8);
    }
    RecPacked region, table;
    o.status = rec_pack_position(cfg, o.world, p, &region, &table) ? kRdAccept : kRdUnpackable;
    return o;
}

// The listed entry in [lo, hi] whose records hold ordinal q: the last j with pre[j] <= q (pre: the exclusive
// prefix of the counts, pre[lo] <= q < pre[hi + 1]).
WQ_RD_HD uint32_t rd_frame_of(const uint64_t* __restrict__ pre, uint32_t lo, uint32_t hi, uint32_t q) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (pre[mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The records examined: the listed frames' total, cut at max_records.
WQ_RD_HD uint32_t rd_examined(uint64_t total, uint64_t max_records) { return (uint32_t)(total < max_records ? total : max_records); }

// The granules' prefix packs accepted << 32 | deferred (both stay below 2^32: they count ordinals).
WQ_RD_HD uint64_t rd_granule_term(const uint64_t* words, uint64_t g) {
    return (uint64_t)dsp_popc(words[kRdWords * g]) << 32 | dsp_popc(words[kRdWords * g + 1]);
}

// The accepted (which 0) or deferred (which 1) records before ordinal q <= the examined total.
WQ_RD_HD uint32_t rd_before(const uint64_t* __restrict__ base, const uint64_t* __restrict__ words, uint32_t which, uint32_t q) {
    const uint32_t g = q / kRdGranule, l = q % kRdGranule;
    uint32_t n = which ? (uint32_t)base[g] : (uint32_t)(base[g] >> 32);
    if (l) n += dsp_popc(words[(uint64_t)kRdWords * g + which] & dsp_below(l));
    return n;
}

struct RdSum {
    uint32_t ops, q, defs;   // accepted ops, query rows, entries of the deferred list
    uint32_t first;          // the kind of the first effective frame, WQ_RRUN_END: none
    uint32_t last;           // with an effective frame: the kind of the run open behind the stretch, WQ_RRUN_END: none
    uint32_t clear;          // bit k: a run of kind k open before the stretch is closed ahead of `first` (or by the end)
    uint32_t starts;         // run starts behind the first effective frame
    uint32_t first_def;      // the first deferred frame, kRdNone: none
};
static_assert(sizeof(RdSum) == 32, "8 words");

WQ_RD_HD RdSum rd_zero() { return RdSum{0, 0, 0, WQ_RRUN_END, WQ_RRUN_END, 0, 0, kRdNone}; }

// The run of kind `open` (or none) after barriers that close the kinds of `clear`.
WQ_RD_HD uint32_t rd_cleared(uint32_t open, uint32_t clear) { return (clear >> open) & 1u ? (uint32_t)WQ_RRUN_END : open; }

// a then b, in list order. RecordProcessor.process keeps one batch of each kind: a barrier of the other kind
// flushes it, an effective frame joins its kind's open batch or starts one. A stretch is that machine's
// function of the run open before it; behind its first effective frame nothing depends on the past.
struct RdCombine {
    WQ_RD_HD RdSum operator()(const RdSum& a, const RdSum& b) const {
        RdSum s;
        s.ops = a.ops + b.ops, s.q = a.q + b.q, s.defs = a.defs + b.defs;
        s.first_def = a.first_def < b.first_def ? a.first_def : b.first_def;
        s.first = a.first != WQ_RRUN_END ? a.first : b.first;
        s.clear = a.first != WQ_RRUN_END ? a.clear : a.clear | b.clear;
        if (a.first == WQ_RRUN_END) {
            s.last = b.last, s.starts = b.starts;
        } else if (b.first == WQ_RRUN_END) {
            s.last = rd_cleared(a.last, b.clear), s.starts = a.starts;
        } else {
            s.last = b.last;
            s.starts = a.starts + b.starts + (rd_cleared(a.last, b.clear) != b.first ? 1u : 0u);
        }
        return s;
    }
};

// The run open before a frame whose predecessors add up to p (none is open before the first frame).
WQ_RD_HD uint32_t rd_open_before(const RdSum& p) { return p.first != WQ_RRUN_END ? p.last : (uint32_t)WQ_RRUN_END; }
// The runs that have started before it.
WQ_RD_HD uint32_t rd_runs_before(const RdSum& p) { return p.first != WQ_RRUN_END ? p.starts + 1u : 0u; }

// A listed frame's own sum: its class, its frame index and the accepted and deferred records it holds.
WQ_RD_HD RdSum rd_frame_sum(uint32_t cls, uint32_t f, uint32_t accepted, uint32_t deferred) {
    RdSum s = rd_zero();
    if (cls == WQ_RCLS_SKIP) return s;
    const uint32_t kind = cls == WQ_RCLS_APPLY ? WQ_RRUN_APPLY : WQ_RRUN_READ;
    s.clear = 1u << (kind == WQ_RRUN_APPLY ? WQ_RRUN_READ : WQ_RRUN_APPLY);  // a barrier flushes the other kind's batch
    s.ops = accepted;
    s.q = cls == WQ_RCLS_READ ? 1u : 0u;
    s.defs = deferred + (cls == WQ_RCLS_READ_DEFERRED ? 1u : 0u);
    if (s.ops || s.q) s.first = s.last = kind;  // effective
    if (s.defs) s.first_def = f;
    return s;
}

// The call's scratch, carved per call.
struct RdWs {
    uint64_t* pre;     // [n_db + 1] the exclusive prefix of cnt
    int64_t* after;    // [n_db]
    RdSum* ex;         // [n_db + 1] the exclusive scan of the frames' sums; the last entry is the total
    uint32_t* cnt;     // [n_db] records of an APPLY frame
    uint32_t* vec;     // [n_db] where its vector's first slot lies in the frame
    uint8_t* cls;      // [n_db]
    uint64_t* words;   // [3 nG] per granule: accepted, deferred, accepted creates
    uint64_t* base;    // [nG] accepted << 32 | deferred before the granule
    uint64_t* cbase;   // [nG] accepted creates before the granule
};

// The scans' terms.
struct RdCountTerm {
    const uint32_t* cnt;
    uint64_t n_db;
    WQ_RD_HD uint64_t operator()(uint64_t j) const { return j < n_db ? cnt[j] : 0u; }
};

// A granule's packed counts (creates: its accepted creates), 0 behind the examined ordinals.
struct RdGranuleTerm {
    const uint64_t* words;
    const uint64_t* total;
    uint64_t max_records;
    bool creates;
    WQ_RD_HD uint64_t operator()(uint64_t g) const {
        if (g * kRdGranule >= rd_examined(*total, max_records)) return 0;
        return creates ? dsp_popc(words[kRdWords * g + 2]) : rd_granule_term(words, g);
    }
};

// Listed entry j's own sum, from the granules' prefix; the zero sum behind the list.
struct RdFrameTerm {
    RdWs ws;
    const uint32_t* db_src;
    uint64_t n_db, max_records;
    WQ_RD_HD RdSum operator()(uint64_t j) const {
        if (j >= n_db) return rd_zero();
        const uint32_t T = rd_examined(ws.pre[n_db], max_records);
        const uint32_t lo = ws.pre[j] < T ? (uint32_t)ws.pre[j] : T, hi = ws.pre[j + 1] < T ? (uint32_t)ws.pre[j + 1] : T;
        uint32_t acc = 0, def = 0;
        if (hi > lo) {
            acc = rd_before(ws.base, ws.words, 0, hi) - rd_before(ws.base, ws.words, 0, lo);
            def = rd_before(ws.base, ws.words, 1, hi) - rd_before(ws.base, ws.words, 1, lo);
        }
        return rd_frame_sum(ws.cls[j], db_src ? db_src[j] : (uint32_t)j, acc, def);
    }
};

// The last ordinal of the granule that starts at q0 < T.
WQ_RD_HD uint32_t rd_granule_last(uint32_t T, uint32_t q0) { return T - q0 > kRdGranule ? q0 + kRdGranule - 1 : T - 1; }

// Ordinal q's record: its listed entry (in [rlo, rhi]), frame and index; the record as rd_record leaves it.
WQ_RD_HD RdRec rd_ordinal_record(const wq_recdisp_in& in, const RdWs& ws, const DecTables& tables, const RecCfg& cfg,
                                 uint32_t rlo, uint32_t rhi, uint32_t q, uint32_t* j, uint32_t* f, uint32_t* r) {
    *j = rd_frame_of(ws.pre, rlo, rhi, q);
    *r = q - (uint32_t)ws.pre[*j];
    uint64_t lo, size;
    uint32_t err = 0;
    if (!rd_frame_span(in, *j, f, &lo, &size, &err)) {  // the frame pass gave such an entry no records
        RdRec o;
        memset(&o, 0, sizeof(o));
        return o;
    }
    return rd_record(in.frames + lo, size, ws.vec[*j], *r, tables, cfg);
}

// The handle of the k-th accepted create of the call.
WQ_RD_HD uint32_t rd_handle(const wq_recdisp_in& in, uint32_t k) {
    return k < in.n_free ? in.free_handles[k] : in.handle_next + (k - in.n_free);
}

// An accepted record's op and reference at row `row`; create_rank: the accepted creates before it.
WQ_RD_HD void rd_emit_op(const wq_recdisp_in& in, const wq_recdisp_out& out, uint32_t f, uint32_t r, bool create,
                         const RdRec& rec, uint32_t row, uint32_t create_rank) {
    if (row >= out.ops_capacity) return;
    if (out.ops) {  // the 64 bytes whole
        uint64_t* d = reinterpret_cast<uint64_t*>(out.ops + row);
        d[0] = (uint64_t)(create ? WQ_RECORD_CREATE : WQ_RECORD_DELETE) | (uint64_t)rec.world << 32;
        d[1] = rec.pos[0], d[2] = rec.pos[1], d[3] = rec.pos[2];
        d[4] = rec.uuid_hi, d[5] = rec.uuid_lo;
        d[6] = (uint64_t)in.now_us;
        d[7] = create ? rd_handle(in, create_rank) : 0u;
    }
    if (out.op_ref) {
        wq_rec_op_ref e;
        e.frame = f, e.record = r, e.data_off = rec.data_off, e.data_len = rec.data_len;
        e.flex_off = rec.flex_off, e.flex_len = rec.flex_len, e.bits = rec.bits, e.pad_ = 0;
        out.op_ref[row] = e;
    }
}

WQ_RD_HD void rd_emit_defer(const wq_recdisp_out& out, uint32_t at, uint32_t f, uint32_t r) {
    if (out.defer && at < out.defer_capacity) out.defer[at] = wq_recdisp_defer{f, r};
}

// Lane `lane` of granule g in the emit: an accepted record is walked again and its op stored at the granule's
// prefix + the accepted lanes below (consecutive rows: one contiguous run per wave); a deferred one is listed
// behind its frame's earlier entries.
WQ_RD_HD void rd_emit_ordinal(const wq_recdisp_in& in, const RdWs& ws, const DecTables& tables, const RecCfg& cfg,
                              const wq_recdisp_out& out, uint32_t g, uint32_t lane, uint32_t rlo, uint32_t rhi) {
    const uint64_t acc = ws.words[(uint64_t)kRdWords * g], def = ws.words[(uint64_t)kRdWords * g + 1];
    const uint64_t crw = ws.words[(uint64_t)kRdWords * g + 2];
    const uint32_t q = g * kRdGranule + lane;
    uint32_t j, f, r;
    if ((acc >> lane) & 1ull) {
        const RdRec rec = rd_ordinal_record(in, ws, tables, cfg, rlo, rhi, q, &j, &f, &r);
        const uint32_t row = (uint32_t)(ws.base[g] >> 32) + dsp_popc(acc & dsp_below(lane));
        const uint32_t crank = (uint32_t)ws.cbase[g] + dsp_popc(crw & dsp_below(lane));
        rd_emit_op(in, out, f, r, (crw >> lane) & 1ull, rec, row, crank);
    } else if ((def >> lane) & 1ull) {
        j = rd_frame_of(ws.pre, rlo, rhi, q);
        const uint32_t first = (uint32_t)ws.pre[j];  // below the examined total: the entry holds ordinal q
        const uint32_t at = ws.ex[j].defs + rd_before(ws.base, ws.words, 1, q) - rd_before(ws.base, ws.words, 1, first);
        rd_emit_defer(out, at, in.db_src ? in.db_src[j] : j, q - first);
    }
}

// Listed frame f of class cls: its query row, its deferred entry and, when it starts a run, its run entry.
// ex: the sum of the entries before it; own: its own sum.
WQ_RD_HD void rd_emit_frame(const wq_recdisp_in& in, const wq_recdisp_out& out, uint32_t f, uint32_t cls, int64_t after,
                            const RdSum& ex, const RdSum& own) {
    if (cls == WQ_RCLS_READ) {
        if (out.q_src) out.q_src[ex.q] = f;
        if (out.q_world) out.q_world[ex.q] = in.world[f];
        if (out.q_pos) {  // bits, not values
            const uint64_t* s = reinterpret_cast<const uint64_t*>(in.msg[f].position);
            uint64_t* d = reinterpret_cast<uint64_t*>(out.q_pos) + 3ull * ex.q;
            d[0] = s[0], d[1] = s[1], d[2] = s[2];
        }
        if (out.q_after) out.q_after[ex.q] = after;
    }
    if (cls == WQ_RCLS_READ_DEFERRED) rd_emit_defer(out, ex.defs, f, WQ_RDEFER_READ);
    const uint32_t run = rd_runs_before(ex);
    if (own.first != WQ_RRUN_END && rd_open_before(ex) != own.first && out.runs && run < out.runs_capacity)
        out.runs[run] = wq_recdisp_run{own.first, f, ex.ops, ex.q};
}

// The closing run and what the counters take from the whole call's sum (the class counts, the drop
// reasons and the error bits were added pass by pass).
WQ_RD_HD void rd_finish(const wq_recdisp_in& in, const wq_recdisp_out& out, const RdSum& t, uint64_t records_total,
                        wq_recdisp_counters* c) {
    const uint32_t n_runs = rd_runs_before(t);
    if (out.runs && n_runs < out.runs_capacity) out.runs[n_runs] = wq_recdisp_run{WQ_RRUN_END, (uint32_t)in.n_frames, t.ops, t.q};
    c->n_db = in.n_db;
    c->n_records_total = records_total;
    c->n_records = rd_examined(records_total, in.max_records);
    c->n_runs = n_runs;
    c->first_deferred = t.first_def == kRdNone ? in.n_frames : t.first_def;
    c->overflow = (t.ops > out.ops_capacity ? kRdOvOps : 0u) | (t.defs > out.defer_capacity ? kRdOvDefer : 0u) |
                  ((uint64_t)n_runs + 1 > out.runs_capacity ? kRdOvRuns : 0u) |
                  (records_total > in.max_records ? kRdOvRecords : 0u);
}

}  // namespace wq
