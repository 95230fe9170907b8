// join_ops.hpp — the arithmetic of the ingest joins (include/wq_router.h, "ingest joins"; kernels:
// wq_join.hip). Everything the kernels compute is here, in functions that are __host__ __device__, so
// tests/cpp/ingest_join_host_shim.hip runs the same code on the CPU in the kernels' passes against
// worldql_server_amd/ingest.py (join_peers_np, drop_peers_np), which is the definition.
//
//   jn_flags        a frame's two bits: candidate (a subscribe the dispatch would defer for its sender
//                   alone) and unknown (decoded, sender not known: a frame the patch may touch)
//   jn_check_new    a candidate whose uuid the table already holds is none: the flags and the table disagree
//   jn_compact      the candidates in frame order from the granules' ballots: key halves and frame index
//                   at the candidate's rank; every slot behind the last candidate is padded with the
//                   all-ones key, which a stable sort leaves behind the real candidates
//   jn_head         the sorted candidates: position s opens a group of equal keys. The sort is stable and
//                   the candidates were in frame order, so a head's frame is its uuid's first_frame
//   jn_decide       the joins' count against the three limits, and the counters
//   jn_join_id      the id of join k: the free list in pop order, then id_next upwards
//   jn_emit         a head's row in j_* at its join rank (its rank among the heads in candidate order)
//   jn_patch        an unknown frame looks its key up among the sorted candidates (the lower bound is the
//                   group's head) and takes the id when it does not precede first_frame
//   jn_merge_old, jn_merge_new   where an old entry and a new key land in the merged table: each adds to
//                   its own rank the count of the other list's keys below it
//   jn_drop_*       the leave side: membership of an entry's id in the sorted id list, and the kept
//                   entries' ranks from the granules' ballots
#pragma once
#include "dispatch_ops.hpp"

namespace wq {

#define WQ_JN_HD __host__ __device__ __forceinline__

constexpr uint32_t kJnGranule = 64;                  // frames / entries per ballot word: one wave
constexpr uint32_t kJnErrDisagree = 1, kJnErrNoTable = 2;       // wq_join_counters.error
constexpr uint32_t kJnOvIds = 1, kJnOvTable = 2, kJnOvOut = 4;  // wq_join_counters.overflow
constexpr uint32_t kJnCand = 1, kJnUnknown = 2;      // jn_flags
constexpr uint64_t kJnPad = ~0ull;

// The control block between the passes: the counters, then what the later passes read on the device.
struct JnCtrl {
    wq_join_counters c;
    uint32_t ok;      // the joins go ahead (no overflow)
    uint32_t k;       // joins
    uint32_t n_cand;  // candidates
    uint32_t live;    // the table's live count when the call began
};
static_assert(sizeof(JnCtrl) == 96, "80 bytes of counters and four words");

// The handle's sender table, keys ascending over [0, *live), room for cap entries.
struct JnTable {
    uint64_t* hi;
    uint64_t* lo;
    uint32_t* id;
    uint32_t* live;
    uint32_t cap;
};

WQ_JN_HD uint64_t jn_be64(const uint8_t* p) {
    uint64_t v = 0;
    for (int k = 0; k < 8; ++k) v = (v << 8) | p[k];
    return v;
}
WQ_JN_HD bool jn_less(uint64_t ah, uint64_t al, uint64_t bh, uint64_t bl) { return ah < bh || (ah == bh && al < bl); }

// The first position in [0, n) whose key is not below (kh, kl).
WQ_JN_HD uint32_t jn_lower_bound(const uint64_t* hi, const uint64_t* lo, uint32_t n, uint64_t kh, uint64_t kl) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (jn_less(hi[mid], lo[mid], kh, kl)) a = mid + 1;
        else b = mid;
    }
    return a;
}

// kJnCand | kJnUnknown of a frame; *err receives kJnErrDisagree (dsp_classify's rule).
WQ_JN_HD uint32_t jn_flags(uint32_t ins, uint32_t flags, uint32_t world, uint32_t sender, uint32_t* err) {
    if (!(flags & kDspOk)) return 0;
    const bool at_global = (flags & kDspAtGlobal) != 0;
    if (((flags & kDspWorldKnown) != 0) != (world < WQ_WORLD_GLOBAL) || at_global != (world == WQ_WORLD_GLOBAL) ||
        ((flags & kDspSenderKnown) != 0) != (sender != kDspNoPeer))
        *err |= kJnErrDisagree;
    if (dsp_sender_known(flags, sender)) return 0;
    const bool cand = ins == WQ_INSTR_AREA_SUBSCRIBE && !at_global && (flags & kDspPos) && dsp_world_resolved(flags, world);
    return kJnUnknown | (cand ? kJnCand : 0u);
}

// A candidate's uuid must be new to the table: one the table holds means the caller's flags and the
// handle's table disagree (kJnErrDisagree), and the frame is left to the host.
WQ_JN_HD uint32_t jn_check_new(const JnTable& t, const uint8_t* uuid, uint32_t i, uint32_t f, uint32_t* err) {
    if (!(f & kJnCand)) return f;
    const uint64_t kh = jn_be64(uuid + 16 * (uint64_t)i), kl = jn_be64(uuid + 16 * (uint64_t)i + 8);
    const uint32_t live = *t.live, pos = jn_lower_bound(t.hi, t.lo, live, kh, kl);
    if (pos >= live || t.hi[pos] != kh || t.lo[pos] != kl) return f;
    *err |= kJnErrDisagree;
    return f & ~kJnCand;
}

// The compacted candidates (n slots each) and the sort's identity permutation.
struct JnCand {
    uint64_t* hi;
    uint64_t* lo;
    uint32_t* frame;
    uint32_t* iota;
};

// Frame i of n: a candidate goes to its rank (base = the candidates in the granules before its own, word =
// its granule's ballot); slot i is padded when it lies behind the c candidates.
WQ_JN_HD void jn_compact(const JnCand& w, const uint8_t* uuid, uint32_t i, bool cand, uint64_t word, uint32_t base,
                         uint32_t c) {
    w.iota[i] = i;
    if (cand) {
        const uint32_t r = base + dsp_popc(word & dsp_below(i % kJnGranule));
        w.hi[r] = jn_be64(uuid + 16 * (uint64_t)i);
        w.lo[r] = jn_be64(uuid + 16 * (uint64_t)i + 8);
        w.frame[r] = i;
    }
    if (i >= c) w.hi[i] = kJnPad, w.lo[i] = kJnPad, w.frame[i] = 0xFFFFFFFFu;
}

// The sorted candidates: keys ascending over [0, c), equal keys in frame order; perm[s] is the rank the
// candidate at s had in frame order.
struct JnSorted {
    const uint64_t* hi;
    const uint64_t* lo;
    const uint32_t* frame;
    const uint32_t* perm;
};

WQ_JN_HD bool jn_head(const JnSorted& s, uint32_t pos, uint32_t c) {
    return pos < c && (pos == 0 || s.hi[pos] != s.hi[pos - 1] || s.lo[pos] != s.lo[pos - 1]);
}

// The counters and the go-ahead from the candidates' count c, the joins' count k and the live count.
WQ_JN_HD void jn_decide(JnCtrl* ctrl, const wq_join_in& in, const wq_join_out& out, uint64_t n, uint32_t c, uint32_t k,
                        uint32_t live, uint32_t cap) {
    uint64_t ov = 0;
    if ((uint64_t)k > (uint64_t)in.n_free + (in.id_limit - in.id_next)) ov |= kJnOvIds;
    if ((uint64_t)live + k > cap) ov |= kJnOvTable;
    if ((out.j_uuid || out.j_id || out.j_frame) && k > out.joined_capacity) ov |= kJnOvOut;
    const bool ok = ov == 0;
    const uint32_t used = k < in.n_free ? k : in.n_free;
    ctrl->ok = ok ? 1u : 0u, ctrl->k = k, ctrl->n_cand = c, ctrl->live = live;
    ctrl->c.n_frames = n, ctrl->c.n_candidates = c, ctrl->c.n_joined = k, ctrl->c.n_patched = 0;
    ctrl->c.n_free_used = ok ? used : 0;
    ctrl->c.id_next = (uint64_t)in.id_next + (ok ? k - used : 0u);
    ctrl->c.n_table = (uint64_t)live + (ok ? k : 0u);
    ctrl->c.first_join = n;
    ctrl->c.overflow = ov;
}

WQ_JN_HD uint32_t jn_join_id(const wq_join_in& in, uint32_t rank) {
    return rank < in.n_free ? in.free_ids[rank] : in.id_next + (rank - in.n_free);
}

// The head at sorted position pos, join number rank: its row in j_*, and the first join's frame.
WQ_JN_HD void jn_emit(const wq_join_in& in, const wq_join_out& out, const JnSorted& s, uint32_t pos, uint32_t rank,
                      JnCtrl* ctrl) {
    const uint32_t f = s.frame[pos];
    if (out.j_uuid)
        for (int b = 0; b < 16; ++b) out.j_uuid[16 * (uint64_t)rank + b] = in.sender_uuid[16 * (uint64_t)f + b];
    if (out.j_id) out.j_id[rank] = jn_join_id(in, rank);
    if (out.j_frame) out.j_frame[rank] = f;
    if (rank == 0) ctrl->c.first_join = f;
}

// Frame i, unknown: patched when its uuid joined at or before it. rank[r] = the joins before candidate r
// in frame order.
WQ_JN_HD bool jn_patch(const wq_join_in& in, const JnSorted& s, const uint32_t* rank, uint32_t c, uint32_t i) {
    const uint64_t kh = jn_be64(in.sender_uuid + 16 * (uint64_t)i), kl = jn_be64(in.sender_uuid + 16 * (uint64_t)i + 8);
    const uint32_t pos = jn_lower_bound(s.hi, s.lo, c, kh, kl);
    if (pos >= c || s.hi[pos] != kh || s.lo[pos] != kl || i < s.frame[pos]) return false;
    in.sender[i] = jn_join_id(in, rank[s.perm[pos]]);
    in.flags[i] = (uint8_t)(in.flags[i] | kDspSenderKnown);
    return true;
}

// The merge. old = the table's copy (n_old entries); heads_before[pos] = the heads below sorted position pos.
// An old entry e moves up by the new keys below it.
WQ_JN_HD void jn_merge_old(const JnTable& t, const uint64_t* ohi, const uint64_t* olo, const uint32_t* oid, uint32_t e,
                           const JnSorted& s, const uint32_t* heads_before, uint32_t c) {
    const uint32_t d = e + heads_before[jn_lower_bound(s.hi, s.lo, c, ohi[e], olo[e])];
    t.hi[d] = ohi[e], t.lo[d] = olo[e], t.id[d] = oid[e];
}
// The head at sorted position pos lands behind the heads and the old entries below it.
WQ_JN_HD void jn_merge_new(const JnTable& t, const uint64_t* ohi, const uint64_t* olo, uint32_t n_old, const JnSorted& s,
                           const uint32_t* heads_before, uint32_t pos, uint32_t id) {
    const uint32_t d = heads_before[pos] + jn_lower_bound(ohi, olo, n_old, s.hi[pos], s.lo[pos]);
    t.hi[d] = s.hi[pos], t.lo[d] = s.lo[pos], t.id[d] = id;
}

// ---- the leave side ----
// Is `id` among the n ascending ids?
WQ_JN_HD bool jn_drop_has(const uint32_t* sorted, uint32_t n, uint32_t id) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (sorted[mid] < id) a = mid + 1;
        else b = mid;
    }
    return a < n && sorted[a] == id;
}
// Entry e stays: it is live and its id is not listed.
WQ_JN_HD bool jn_drop_keep(const uint32_t* ids, const uint32_t* sorted, uint32_t n, uint32_t live, uint32_t e) {
    return e < live && !jn_drop_has(sorted, n, ids[e]);
}
// The counters of a drop of n ids that left `kept` of `live` entries.
WQ_JN_HD void jn_drop_finish(JnCtrl* ctrl, uint64_t n, uint32_t live, uint32_t kept) {
    ctrl->c.n_frames = n, ctrl->c.n_candidates = 0, ctrl->c.n_joined = 0, ctrl->c.n_patched = live - kept;
    ctrl->c.n_free_used = 0, ctrl->c.id_next = 0, ctrl->c.n_table = kept, ctrl->c.first_join = n;
    ctrl->c.overflow = 0;
}
// A handle without a reserved table: the counters of the no-op.
WQ_JN_HD void jn_no_table(JnCtrl* ctrl, uint64_t n, uint32_t id_next) {
    ctrl->c.n_frames = n, ctrl->c.n_candidates = 0, ctrl->c.n_joined = 0, ctrl->c.n_patched = 0;
    ctrl->c.n_free_used = 0, ctrl->c.id_next = id_next, ctrl->c.n_table = 0, ctrl->c.first_join = n;
    ctrl->c.overflow = 0, ctrl->c.error = kJnErrNoTable;
}

}  // namespace wq
