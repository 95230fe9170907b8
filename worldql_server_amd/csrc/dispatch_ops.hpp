// dispatch_ops.hpp — the arithmetic of the ingest dispatch (include/wq_router.h, "ingest dispatch";
// kernels: wq_dispatch.hip). Everything the kernels compute is here, in functions that are
// __host__ __device__, so tests/cpp/ingest_dispatch_host_shim.hip runs the same code on the CPU against
// worldql_server_amd/ingest.py (dispatch_np), which is the definition.
//
//   dsp_classify        a frame's class from its 10 bytes of instruction, flags, world and sender: the
//                       reference's drop rules (local_message.rs:17-56, global_message.rs:18-54,
//                       area_subscribe.rs:17-46, area_unsubscribe.rs) and the three channels of
//                       thread.rs:72-108.
//   DspSum, dsp_combine what a stretch of frames adds up to: the count of every class, the kind of its
//                       first and of its last effective frame, the run starts inside it, its first
//                       deferred frame and its error bits. dsp_combine is associative ("right if not
//                       none, else left" for the last kind; a run starts between two stretches when the
//                       left one's last kind and the right one's first kind both exist and differ), so
//                       one scan carries counts and runs together.
//   dsp_granule_sum     the DspSum of a granule of 64 frames from its ten class ballots.
//   dsp_prev_kind       the kind of the last effective frame before a lane, inside the granule or
//                       inherited: what decides whether the lane starts a run.
//   dsp_lane_before, dsp_starts_run, dsp_lane_run   a lane's ranks from its granule's ballots.
//   dsp_emit            a frame's row, list entry, stamp or run entry at its ranks.
#pragma once
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/wq_codec.h"
#include "../../include/wq_router.h"

namespace wq {

#define WQ_DSP_HD __host__ __device__ __forceinline__

constexpr uint32_t kDspGranule = 64;               // frames per ballot word: one wave
constexpr uint32_t kDspBlock = 1024;               // frames per block: 16 granules, one DspSum
constexpr uint32_t kDspGranules = kDspBlock / kDspGranule;
constexpr uint32_t kDspScanBlock = 256;            // lanes of the one scanning block
constexpr uint32_t kDspNone = 0xFFFFFFFFu;
constexpr uint32_t kDspNoPeer = 0xFFFFFFFFu;
constexpr uint32_t kDspErrDisagree = 1;            // wq_dispatch_counters.error bit 0

// wq_ingest_out.flags
constexpr uint32_t kDspOk = 1, kDspPos = 2, kDspAtGlobal = 16, kDspWorldKnown = 32, kDspSenderKnown = 64;

constexpr uint32_t kInsHeartbeat = 0, kInsRecordCreate = 8, kInsRecordRead = 9, kInsRecordDelete = 11;

struct DspSum {
    uint32_t cnt[WQ_CLS_COUNT];
    uint32_t first, last;  // WQ_RUN_END (none) / WQ_RUN_TABLE / WQ_RUN_READ
    uint32_t starts;       // run starts among the effective frames, the stretch's first one not counted
    uint32_t first_def;    // kDspNone: no deferred frame
    uint32_t err;
};
static_assert(sizeof(DspSum) == 60, "15 words");

WQ_DSP_HD DspSum dsp_zero() {
    DspSum s;
    for (uint32_t c = 0; c < WQ_CLS_COUNT; ++c) s.cnt[c] = 0;
    s.first = s.last = WQ_RUN_END;
    s.starts = 0;
    s.first_def = kDspNone;
    s.err = 0;
    return s;
}

// a then b, in arrival order
WQ_DSP_HD DspSum dsp_combine(const DspSum& a, const DspSum& b) {
    DspSum s;
    for (uint32_t c = 0; c < WQ_CLS_COUNT; ++c) s.cnt[c] = a.cnt[c] + b.cnt[c];
    s.first = a.first != WQ_RUN_END ? a.first : b.first;
    s.last = b.last != WQ_RUN_END ? b.last : a.last;
    s.starts = a.starts + b.starts + (a.last != WQ_RUN_END && b.first != WQ_RUN_END && a.last != b.first ? 1u : 0u);
    s.first_def = a.first_def < b.first_def ? a.first_def : b.first_def;
    s.err = a.err | b.err;
    return s;
}

// The runs that have started before a frame whose predecessors add up to p.
WQ_DSP_HD uint32_t dsp_runs_before(const DspSum& p) { return p.starts + (p.first != WQ_RUN_END ? 1u : 0u); }

WQ_DSP_HD bool dsp_world_resolved(uint32_t flags, uint32_t world) {
    return (flags & kDspWorldKnown) && world < WQ_WORLD_GLOBAL;
}
WQ_DSP_HD bool dsp_sender_known(uint32_t flags, uint32_t sender) {
    return (flags & kDspSenderKnown) && sender != kDspNoPeer;
}
// The sender a row carries: the id, or the no-peer id when it is not known.
WQ_DSP_HD uint32_t dsp_row_sender(uint32_t flags, uint32_t sender) {
    return dsp_sender_known(flags, sender) ? sender : kDspNoPeer;
}

// The class of a frame; *err receives the error bits it raises.
WQ_DSP_HD uint32_t dsp_classify(uint32_t ins, uint32_t flags, uint32_t world, uint32_t sender, uint32_t* err) {
    if (!(flags & kDspOk)) return WQ_CLS_BAD;
    const bool at_global = (flags & kDspAtGlobal) != 0;
    if (((flags & kDspWorldKnown) != 0) != (world < WQ_WORLD_GLOBAL) || at_global != (world == WQ_WORLD_GLOBAL) ||
        ((flags & kDspSenderKnown) != 0) != (sender != kDspNoPeer))
        *err |= kDspErrDisagree;
    const bool has_pos = (flags & kDspPos) != 0;
    const bool world_ok = dsp_world_resolved(flags, world);
    const bool sender_ok = dsp_sender_known(flags, sender);
    switch (ins) {
    case kInsHeartbeat:
        return WQ_CLS_HEARTBEAT;
    case WQ_INSTR_LOCAL_MESSAGE:  // local_message.rs:17-56
        return !at_global && has_pos && world_ok ? WQ_CLS_LOCAL : WQ_CLS_DROPPED;
    case WQ_INSTR_GLOBAL_MESSAGE:  // global_message.rs:18-54
        return at_global ? WQ_CLS_BCAST : world_ok ? WQ_CLS_GLOBAL : WQ_CLS_DROPPED;
    case WQ_INSTR_AREA_SUBSCRIBE:  // area_subscribe.rs:17-46; an unresolved world or sender is a join
        if (at_global || !has_pos) return WQ_CLS_DROPPED;
        return world_ok && sender_ok ? WQ_CLS_OP : WQ_CLS_DEFERRED;
    case WQ_INSTR_AREA_UNSUBSCRIBE:  // area_unsubscribe.rs; a peer without an id holds nothing
        return !at_global && has_pos && world_ok && sender_ok ? WQ_CLS_OP : WQ_CLS_DROPPED;
    case kInsRecordCreate:
    case kInsRecordRead:
    case kInsRecordDelete:
        return WQ_CLS_DB;
    default:
        return WQ_CLS_OTHER;
    }
}

WQ_DSP_HD uint32_t dsp_kind_of(uint32_t cls) {
    return cls == WQ_CLS_OP ? WQ_RUN_TABLE : cls == WQ_CLS_LOCAL || cls == WQ_CLS_GLOBAL ? WQ_RUN_READ : WQ_RUN_END;
}

WQ_DSP_HD uint32_t dsp_popc(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(v);
#else
    return (uint32_t)__builtin_popcountll(v);
#endif
}
WQ_DSP_HD uint32_t dsp_lowest(uint64_t v) {  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__ffsll((unsigned long long)v) - 1u;
#else
    return (uint32_t)__builtin_ctzll(v);
#endif
}
WQ_DSP_HD uint32_t dsp_highest(uint64_t v) {  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 63u - (uint32_t)__clzll((long long)v);
#else
    return 63u - (uint32_t)__builtin_clzll(v);
#endif
}
WQ_DSP_HD uint64_t dsp_below(uint32_t lane) { return lane ? ~0ull >> (64 - lane) : 0ull; }

// The kind of the last effective frame before `lane`: inside the granule (table / read are the ballots
// of the table and the read frames), else `inherited`.
WQ_DSP_HD uint32_t dsp_prev_kind(uint64_t table, uint64_t read, uint32_t lane, uint32_t inherited) {
    const uint64_t below = (table | read) & dsp_below(lane);
    if (!below) return inherited;
    return (table >> dsp_highest(below)) & 1 ? WQ_RUN_TABLE : WQ_RUN_READ;
}

// Whether a lane of kind `kind` starts a run inside its granule: its predecessor there exists and differs.
WQ_DSP_HD bool dsp_inner_start(uint64_t table, uint64_t read, uint32_t lane, uint32_t kind) {
    if (kind == WQ_RUN_END) return false;
    const uint32_t prev = dsp_prev_kind(table, read, lane, WQ_RUN_END);
    return prev != WQ_RUN_END && prev != kind;
}

// A granule's sum from its class ballots m[WQ_CLS_COUNT], the ballot of its inner starts, its first
// frame's index and whether a lane raised an error.
WQ_DSP_HD DspSum dsp_granule_sum(const uint64_t* m, uint64_t inner_starts, uint32_t base, uint32_t err) {
    DspSum s;
    for (uint32_t c = 0; c < WQ_CLS_COUNT; ++c) s.cnt[c] = dsp_popc(m[c]);
    const uint64_t table = m[WQ_CLS_OP], read = m[WQ_CLS_LOCAL] | m[WQ_CLS_GLOBAL], eff = table | read;
    s.first = s.last = WQ_RUN_END;
    if (eff) {
        s.first = (table >> dsp_lowest(eff)) & 1 ? WQ_RUN_TABLE : WQ_RUN_READ;
        s.last = (table >> dsp_highest(eff)) & 1 ? WQ_RUN_TABLE : WQ_RUN_READ;
    }
    s.starts = dsp_popc(inner_starts);
    s.first_def = m[WQ_CLS_DEFERRED] ? base + dsp_lowest(m[WQ_CLS_DEFERRED]) : kDspNone;
    s.err = err;
    return s;
}

// Where the five side lists begin inside side_src, and the end (the counters' side_begin).
WQ_DSP_HD void dsp_side_begin(const uint32_t* cnt, uint64_t* sb) {
    sb[0] = 0;
    sb[1] = sb[0] + cnt[WQ_CLS_HEARTBEAT];
    sb[2] = sb[1] + cnt[WQ_CLS_BCAST];
    sb[3] = sb[2] + cnt[WQ_CLS_DB];
    sb[4] = sb[3] + cnt[WQ_CLS_OTHER];
    sb[5] = sb[4] + cnt[WQ_CLS_DEFERRED];
}
// The list of side_src a class goes to, -1: none.
WQ_DSP_HD int dsp_side_list(uint32_t cls) {
    switch (cls) {
    case WQ_CLS_HEARTBEAT: return 0;
    case WQ_CLS_BCAST: return 1;
    case WQ_CLS_DB: return 2;
    case WQ_CLS_OTHER: return 3;
    case WQ_CLS_DEFERRED: return 4;
    default: return -1;
    }
}

// The counters and the closing run from the whole tick's sum.
WQ_DSP_HD void dsp_finish(const DspSum& t, uint64_t n, const wq_dispatch_out& out, wq_dispatch_counters* c) {
    const uint32_t n_runs = dsp_runs_before(t);
    if (out.runs && n_runs < out.runs_capacity) {
        wq_dispatch_run e;
        e.kind = WQ_RUN_END, e.first_frame = (uint32_t)n;
        e.l_begin = t.cnt[WQ_CLS_LOCAL], e.g_begin = t.cnt[WQ_CLS_GLOBAL], e.op_begin = t.cnt[WQ_CLS_OP];
        out.runs[n_runs] = e;
    }
    if (!c) return;
    c->n_frames = n;
    uint64_t* per = &c->n_bad;
    for (uint32_t k = 0; k < WQ_CLS_COUNT; ++k) per[k] = t.cnt[k];
    c->n_runs = n_runs;
    dsp_side_begin(t.cnt, c->side_begin);
    c->first_deferred = t.first_def == kDspNone ? n : t.first_def;
    c->overflow = (uint64_t)n_runs + 1 > out.runs_capacity ? 1 : 0;
    c->error = t.err;
}

// What lies before lane `lane` of a granule whose predecessors add up to gp: the count of every class
// (m = the granule's class ballots).
WQ_DSP_HD void dsp_lane_before(const DspSum& gp, const uint64_t* m, uint32_t lane, uint32_t* before) {
    const uint64_t below = dsp_below(lane);
    for (uint32_t c = 0; c < WQ_CLS_COUNT; ++c) before[c] = gp.cnt[c] + dsp_popc(m[c] & below);
}
// Whether a lane of kind `kind` starts a run: the last effective frame before it, in the granule or
// before it (gp.last), is of another kind or does not exist.
WQ_DSP_HD bool dsp_starts_run(const DspSum& gp, uint64_t table, uint64_t read, uint32_t lane, uint32_t kind) {
    return kind != WQ_RUN_END && dsp_prev_kind(table, read, lane, gp.last) != kind;
}
// The runs that have started before a lane (starts = the granule's ballot of dsp_starts_run).
WQ_DSP_HD uint32_t dsp_lane_run(const DspSum& gp, uint64_t starts, uint32_t lane) {
    return dsp_runs_before(gp) + dsp_popc(starts & dsp_below(lane));
}

// Frame i of class cls: its row, list entry or op at before[cls] (before = the class counts of the
// frames before it, total = the whole tick's sum), its stamp, and with starts_run its run entry at `run`.
WQ_DSP_HD void dsp_emit(const wq_dispatch_in& in, const wq_dispatch_out& out, uint32_t i, uint32_t cls,
                        const uint32_t* before, const DspSum& total, bool starts_run, uint32_t run) {
    const uint32_t flags = in.flags[i];
    const uint32_t r = before[cls];
    const uint64_t* pos = reinterpret_cast<const uint64_t*>(in.pos) + 3 * (uint64_t)i;  // bits, not values
    switch (cls) {
    case WQ_CLS_LOCAL:
        if (out.l_src) out.l_src[r] = i;
        if (out.l_pos) {
            uint64_t* d = reinterpret_cast<uint64_t*>(out.l_pos) + 3 * (uint64_t)r;
            d[0] = pos[0], d[1] = pos[1], d[2] = pos[2];
        }
        if (out.l_world) out.l_world[r] = in.world[i];
        if (out.l_sender) out.l_sender[r] = dsp_row_sender(flags, in.sender[i]);
        if (out.l_repl) out.l_repl[r] = in.repl[i];
        break;
    case WQ_CLS_GLOBAL:
        if (out.g_src) out.g_src[r] = i;
        if (out.g_world) out.g_world[r] = in.world[i];
        if (out.g_sender) out.g_sender[r] = dsp_row_sender(flags, in.sender[i]);
        if (out.g_repl) out.g_repl[r] = in.repl[i];
        break;
    case WQ_CLS_OP:
        if (out.op_src) out.op_src[r] = i;
        if (out.ops) {  // the 40 bytes whole, padding zeroed
            uint64_t* d = reinterpret_cast<uint64_t*>(out.ops + r);
            d[0] = (uint64_t)in.world[i] | (uint64_t)in.sender[i] << 32;
            d[1] = in.instruction[i] == WQ_INSTR_AREA_SUBSCRIBE ? WQ_OP_SUBSCRIBE : WQ_OP_UNSUBSCRIBE;
            d[2] = pos[0], d[3] = pos[1], d[4] = pos[2];
        }
        break;
    case WQ_CLS_HEARTBEAT: {
        const uint32_t s = dsp_row_sender(flags, in.sender[i]);
        if (in.last_seen && s < in.n_last_seen) in.last_seen[s] = in.now;
        break;
    }
    default:
        break;
    }
    const int list = dsp_side_list(cls);
    if (list >= 0 && out.side_src) {
        uint64_t sb[6];
        dsp_side_begin(total.cnt, sb);
        out.side_src[sb[list] + r] = i;
    }
    if (starts_run && out.runs && run < out.runs_capacity) {
        wq_dispatch_run e;
        e.kind = dsp_kind_of(cls), e.first_frame = i;
        e.l_begin = before[WQ_CLS_LOCAL], e.g_begin = before[WQ_CLS_GLOBAL], e.op_begin = before[WQ_CLS_OP];
        out.runs[run] = e;
    }
}

}  // namespace wq
