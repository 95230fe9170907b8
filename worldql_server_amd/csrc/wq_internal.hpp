// wq_internal.hpp — host-side state of one router handle (one GPU, one owner thread).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/wq_router.h"
#include "wq_device.hpp"

namespace wq {

// wq_route_health error bit 16: a device op batch held an invalid op and was not applied.
constexpr uint32_t kErrBadBatch = 16u;

// Grow-only device buffer.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    // hipExtMallocWithFlags flags for the next allocation (0: hipMalloc); a flagged allocation that
    // fails falls back to hipMalloc
    unsigned flags = 0;
    bool flagged = false;  // the current allocation came from hipExtMallocWithFlags
    hipError_t ensure(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);
            if (e != hipSuccess) return e;
            p = nullptr;
            bytes = 0;
        }
        size_t cap = need < 4096 ? 4096 : need + need / 4;
        hipError_t e = flags ? hipExtMallocWithFlags(&p, cap, flags) : hipMalloc(&p, cap);
        flagged = flags && e == hipSuccess;
        if (e != hipSuccess && flags) {
            (void)hipGetLastError();
            p = nullptr;
            e = hipMalloc(&p, cap);
        }
        if (e == hipSuccess) bytes = cap;
        return e;
    }
    template <typename T>
    T* as() const { return static_cast<T*>(p); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// A device buffer that is all zero between the calls that use it. The select of the send budgets
// (wq_budget.hip) needs every bin of its histograms zero when a call starts. Every pick pass zeroes
// the bins it read, so a call that launched all its passes leaves them zero: `clean` is the number of
// bytes known to be zero. It is 0 for a new allocation (decided from the capacity, not the address:
// a freed block's address can come back) and between begin() and end(), while a call's passes are
// being launched, so a call that failed between a histogram pass and its pick makes the next one
// clear the buffer.
struct ZeroedBuf {
    DevBuf b;
    size_t clean = 0;
    // Room for `need` bytes, all zero once the stream reaches this point (defined below the handle).
    int prepare(wq_router* h, size_t need, hipStream_t stream);
    void begin() { clean = 0; }
    void end() { clean = b.bytes; }
    void release() {
        b.release();
        clean = 0;
    }
};

// The live subscription set, sorted by (hash, world, key, peer): one entry per
// (world, cube, peer) triple. Everything the route kernel reads is derived from it.
struct State {
    DevBuf h, w, kx, ky, kz, p;  // u64, u32, i64 x3, u32
    uint64_t n = 0;
};

struct Table {
    DevBuf recs;      // Record[rec_cap]: regular cubes (wq_device.hpp), load <= 0.3
    DevBuf rclaim;    // u32[rec_cap] (build scratch)
    uint64_t rec_cap = 0;
    int rec_shift = 64;
    DevBuf slots;     // Slot[cap]: cubes without a packed key
    DevBuf claim;     // u32[cap] (build scratch)
    DevBuf list;      // u32 words: per cube [count, peers...] (+ room for relocated lists)
    DevBuf any;       // u64[n_any] sorted (world << 32 | peer)
    uint64_t cap = 0;
    int shift = 64;
    uint64_t n_cubes = 0, n_any = 0;
    // incremental updates (wq_delta.hip): list words in use (lists are bump-allocated past the
    // build's dense region when they outgrow their capacity) and record slots in use (including
    // records whose cube emptied: they keep their key, count 0)
    uint64_t list_used = 0, list_cap = 0, n_recs = 0;
    // per-peer boxes (wq_device.hpp PeerBox): kBoxWords words per peer, then the valid word
    DevBuf pbox;
    uint32_t n_pbox = 0;
    // u32: non-zero while the last incremental batch could not be applied on the device (the
    // next host call re-applies it); route kernels report error bit 8 meanwhile
    DevBuf stale;
    // dense record headers (TableView::hdr): 32 B per record slot, refreshed by every full build;
    // off (hdr_ok false) from the first in-place change until the next build
    DevBuf hdr;
    bool hdr_ok = false;
    // compact headers (round 6, default): their own open-addressed table at load <= 1/2 (hdr_cap
    // slots), each header's cap word replaced by its record slot; hdr_cap == 0: the round-4 layout
    // (header i = record i's first 32 bytes, WQ_HDR_COMPACT=0)
    uint64_t hdr_cap = 0;
    int hdr_shift = 64;
    uint32_t hdr_blk = 0;  // wq_device.hpp hdr_home (WQ_HDR_BLOCK)
};

// The last incremental batch (wq_delta.hip), in flight: its status and stat deltas arrive in
// pinned memory; the next host call folds them in (and re-applies the batch if it was not
// applied) — the update itself never waits for the GPU.
struct PendingDelta {
    bool active = false;
    hipEvent_t ev = nullptr;
    void* pinned = nullptr;     // DeltaStatus (32 B) + i64 {entries, live cubes} deltas
    const wq_op* ops = nullptr; // the batch (h->d_ops or the caller's device array)
    size_t n = 0;
    uint64_t list_room = 0;
};

// Scratch of the incremental update (wq_delta.hip).
struct DeltaWs {
    DevBuf part, summ;      // REMOVE_PEER per-block partial sums; a batch's DeltaStatus
    DevBuf dstat;           // i64 x2: entry / live-cube deltas of batches not yet read back
    DevBuf rm_bits;         // REMOVE_PEER from every world: bitmap over peer ids
    DevBuf sort_cnt;        // bucket sort: per (digit, tile) key counts, then their row prefixes
    DevBuf sort_tot;        // bucket sort: per digit key totals
};

// Route workspace, persistent across calls so a tick needs no memset: two counter slots (each
// call's count pass zeroes the next call's) and the per-message state the count pass hands to
// the scan and emit passes.
struct RouteWs {
    DevBuf buf;    // [pad 64][wq_route_counters x2]
    DevBuf info;   // uint2[M]: locators, count pass -> emit pass
    DevBuf e;      // u32[M]: filtered counts
    DevBuf tiles;  // u32[2 * n_count_blocks]: block totals, then their exclusive prefix
    DevBuf spill;  // per-block output images of the count+spill tick (route config 7)
    DevBuf agg;    // u64[2 * blocks]: look-back and candidate granules of the single-launch tick
    DevBuf scan_tmp;  // rocPRIM temporary storage of the many-tile scan (WQ_SCAN_MULTI=0)
    DevBuf sgran;     // u64[2 * blocks]: the multi-block tile scan's tagged block aggregates {E, F}
    uint64_t sgran_zeroed = 0;  // granules zeroed so far (a fresh one never matches a tag)
    uint64_t scan_calls = 0;    // multi-block scans so far (their tags)
    uint64_t agg_zeroed = 0;
    uint64_t agg_epoch = 0;  // calls / kTickTagPeriod when agg was last zeroed (zeroed again when the tags wrap)
    uint64_t* stamps = nullptr;  // wq_debug_set_timeline
    // the pipelined heavy tick (wq_route.hip, short ticks): count chunks on `side` while the launch
    // stream scans and emits the previous chunk; {P, F} carried across the chunks' scans
    hipStream_t side = nullptr;
    hipEvent_t ev_in = nullptr;
    std::vector<hipEvent_t> cev;
    DevBuf carry;
    uint64_t calls = 0;
    wq_route_counters* last = nullptr;  // counters of the most recent call (device)
    // wq_route_tick_device's caller counters: the three-launch tick's scan writes them itself when it
    // can (out_done), instead of a copy launch after the tick
    wq_route_counters* out = nullptr;
    bool out_done = false;
};

struct ProfileEvents {
    std::vector<hipEvent_t> start, stop;
    // the three-launch shape (count / tile scan / emit) also records an event after the count and
    // one after the scan, so wq_profile_read_phases can split a launch's time per kernel
    std::vector<hipEvent_t> mid1, mid2;
    std::vector<char> phased;
    size_t used = 0;
    bool enabled = false;
};

// Scratch of the table export (wq_table_export.hip), grow-only: per table slot the live flag and its
// prefix; per live cube the sort words, count and table slot, then count, slot and row base in
// canonical order; per granule of 64 rows the filter's flag word, count and prefix; the peer bitmap;
// the totals; the host form's (and a multi-GPU merge's) device image of the rows.
struct ExportWs {
    DevBuf flag, pos, keys, cnt, src, ocnt, osrc, base, gword, gcnt, gbase, bits, tot, stage, merge;
    void* pinned = nullptr;
};

struct ShardCtx;  // shard_ctx.hpp: the exchange a sharded tick uses, and its workspace
struct MultiCtx;  // wq_multi.hip: a handle over G GPUs (wq_router_create_multi)
struct RecStore;  // wq_records.hip: the record store (wq_records_open)
struct RecCfg;    // record_ops.hpp: a store's configuration
struct DecTables; // decode_ops.hpp: the handle's world and sender tables as the kernels take them

}  // namespace wq

struct wq_router {
    int device = 0;
    uint16_t cube_size = 16;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    uint64_t hash_mask = ~0ull;
    uint32_t rec_slack = 8;  // record slots per cube at build (load <= 1/rec_slack)
    bool rec_slack_set = false;  // set by wq_debug_set_record_slack (then no footprint cap)
    uint64_t hash_fallbacks = 0;
    std::string err;

    wq::State st, st_next;
    wq::Table tab;
    // After incremental updates the sorted state `st` and the any-keys are stale; they are
    // regenerated from the records on demand (table_materialize / table_ensure_any).
    bool st_stale = false, any_stale = false;
    wq::DeltaWs dws;
    wq::PendingDelta pend;
    // incremental batches applied, batches that fell back to the rebuild, applied batches in which
    // some cube took the wave path (lists longer than kLaneList)
    uint64_t n_delta_applies = 0, n_delta_fallbacks = 0, n_delta_wave_batches = 0;
    uint64_t n_delta_batches = 0;  // batch tags of the record claims (wq_delta.hip)
    bool dstat_pending = false;
    // bumped by every change of the table (an op batch, a removal, a re-applied device batch):
    // results that point into the table (the slot tick's kept rows) are valid for one generation
    uint64_t table_gen = 0;

    // build scratch
    wq::DevBuf ev_h, ev_w, ev_kx, ev_ky, ev_kz, ev_p, ev_kind, d_ops;
    const wq_op* cur_ops = nullptr;  // the batch being applied (h->d_ops, or the caller's device array)
    wq::DevBuf idx_a, idx_b, key32_a, key32_b, key64_a, key64_b, flags, scan, sort_tmp, small;
    wq::DevBuf cube_id, cube_start;

    wq::RouteWs rws;
    // sharded ticks (wq_shard.hip): owner histograms, unpacked received records
    wq::DevBuf shard_hist, rec_keys, rec_w, rec_s, rec_r;
    // the one-pass slot grouping (wq_shard.hip slot_group_kernel): tagged look-back granules per
    // (owner, block), zeroed once per allocation (tag 0 never matches), and the launches so far
    wq::DevBuf shard_look;
    uint64_t shard_look_zeroed = 0, shard_look_calls = 0, shard_look_epoch = 0;
    int route_cfg = 0;  // route kernel shapes (wq_route.hip kCfgs)
    uint32_t route_chunks = 0;  // wq_debug_set_route_chunks: chunks of the pipelined heavy tick (0 = default)
    bool heavy_fanout = false;  // wq_set_fanout_hint: default shape -> kCfgHeavy
    bool fanout_auto = true;    // until wq_set_fanout_hint: wq_route_tick sets heavy_fanout from its P / M
    // host-pointer convenience buffers
    wq::DevBuf h_in, h_out;
    // C5 radius filter (wq_set_radius / wq_set_peer_positions)
    wq::DevBuf ppos;
    wq::DevBuf ppos4;  // f32 copy (float4 per peer) for the radius filter's second test
    wq::DevBuf pcode;  // 4-byte position codes (the first test) and their box (wq_device.hpp)
    wq::DevBuf qbox;   // u64 box keys [0, 6), then {lo, step} doubles [6, 12), the second box slot [12, 18)
    int qbox_phase = -1;  // the box slot the next wq_set_peer_positions accumulates into (-1: not reset yet)
    uint64_t n_ppos = 0;
    double radius = 0.0;
    wq::ProfileEvents prof;
    wq::ShardCtx* shard = nullptr;  // wq_shard_attach_*: this handle is one shard of G
    bool shard_expanded = false;    // wq_debug_set_shard_form: expanded pairs back instead of row references
    int shard_inject = 0;           // wq_debug_inject_shard_failure: fail the next sharded tick's step 1 or 3
    wq::MultiCtx* multi = nullptr;  // wq_router_create_multi: this handle drives G shard handles
    // follow (wq_follow.hip): per peer id the world (WQ_WORLD_INVALID: not followed) and position it
    // was last followed at — separate from the radius filter's ppos — and the scratch of a call: op
    // counts, their exclusive prefix, the packed axis masks, the totals (device / pinned), the op
    // buffer of the latest call (a pending batch may be re-applied from it) and the host form's staging
    wq::DevBuf fol_world, fol_pos, fol_cnt, fol_off, fol_mask, fol_tot, fol_ops, fol_in;
    void* fol_pinned = nullptr;
    uint64_t fol_cap = 0;    // peers the state covers
    uint64_t fol_n = 0;      // peers followed now
    uint64_t fol_n_ops = 0;  // ops of the latest call
    uint64_t fol_len = 0;    // peers wq_follow_state_read reports: the largest n a call or a load covered
    uint32_t fol_reach = 1;
    // interest diff (wq_csr_diff.hip): per row the clamped lengths of both sides and their prefix,
    // per granule the counts and their prefix, the granules' flag words, and two error slots (each
    // call zeroes the next call's) followed by the host form's counters
    wq::DevBuf diff_len, diff_pre, diff_cnt, diff_base, diff_flags, diff_err;
    uint64_t diff_calls = 0;
    // the send side's ordinal space (send_rows.hpp rows_alloc / rows_view), shared by the budgets, the
    // fair share and the send buffers: per peer the clamped lengths (then the kept or chosen counts),
    // their saturating prefix and the prefix clamped to n_in
    wq::DevBuf bud_len, bud_sum, bud_pre;
    // send budgets (wq_budget.hip): per ordinal the key, row and class; per slot of kBudShort ordinals
    // the select's state and u32 histogram; per granule of 64 the tie and keep flag words, counts and
    // prefixes; {rows_cut, error}
    wq::DevBuf bud_key, bud_row, bud_cls, bud_sel, bud_words, bud_cnt, bud_base, bud_ctrl;
    wq::ZeroedBuf bud_hist;
    // byte budgets (wq_budget.hip): they run on the buffers above and add, per ordinal, the size and
    // one u64 scan entry, and per slot the weighted select's state and u64 histogram: a zeroed buffer
    // of its own, so the two calls alternate on one handle
    wq::DevBuf byt_size, byt_scan, byt_sel;
    wq::ZeroedBuf byt_hist;
    // fair share (wq_rotate.hip): it runs on the buffers above (the full CSR's ordinal space, the
    // per-ordinal row and size, the u64 scan, the flag words, ctrl) and adds the kept CSR's ordinal
    // space and, per peer, the folded scan terms of its row (RotRow), and the slots the counters' adds
    // are spread over
    wq::DevBuf rot_len, rot_sum, rot_pre, rot_rows, rot_part;
    // send buffers (wq_pack.hip): the rows run on the shared ordinal space above; per ordinal the
    // frame's size, where it starts and one u64 scan entry; {unused, error}
    wq::DevBuf pack_size, pack_src, pack_scan, pack_ctrl;
    // frame builder (wq_frames.hip): per message the frame's size; {unused, error}; the world table
    // (wq_frames_set_worlds): the names back to back and their n_worlds + 1 offsets
    wq::DevBuf frm_size, frm_ctrl, frm_world_bytes, frm_world_off;
    uint32_t frm_n_worlds = 0;
    uint64_t frm_world_total = 0;
    // ingest decoder (wq_decode.hip): per frame the word between the passes; the long-string work list;
    // the counters and behind them the list's count; the world table's lookup order (hashes ascending,
    // their ids), built by wq_frames_set_worlds; the sender table (wq_ingest_set_peers): keys ascending
    wq::DevBuf ing_word, ing_list, ing_ctrl, ing_whash, ing_wid, ing_phi, ing_plo, ing_pid;
    uint32_t ing_n_peers = 0;
    int64_t ing_list_cap = -1;  // wq_debug_set_ingest_list (negative: the default)
    // ingest joins (wq_join.hip). wq_ingest_peers_reserve: ing_cap > 0 is the sender table's room in
    // entries and ing_live holds its live count, one device u32 the decode reads in place of ing_n_peers.
    // A call's scratch (per frame and per table entry), the table's copy during a merge or a compaction,
    // and the control block between the passes.
    wq::DevBuf ing_live, join_ws, join_tab, join_ctrl;
    uint32_t ing_cap = 0;
    // ingest leaves (wq_leave.hip): a call's scratch (per reserved table entry and per 32 ids) and the
    // control block between the passes; the table's second buffer is join_tab
    wq::DevBuf leave_ws, leave_ctrl;
    // ingest dispatch (wq_dispatch.hip): per frame its class between the passes; one DspSum per 1,024
    // frames and the total behind them
    wq::DevBuf dsp_cls, dsp_sum;
    // record dispatch (wq_recdispatch.hip): per listed frame its class, record count, vector, `after`, the
    // counts' prefix and the frames' scanned sums; per granule of 64 records the flag words and the two
    // prefixes; the counters
    wq::DevBuf rdp, rdp_ctrl;
    // record payload slab (wq_slab.hip): per op two elements (data, flex) with their size, source and one
    // u64 scan entry; the control block between the passes
    wq::DevBuf slab_ws, slab_ctrl;
    // slab compaction (wq_slab_compact.hip): per source entry its term, the scan's pair and one element of the
    // dense list of live entries; the control block between the passes
    wq::DevBuf cmp_ws, cmp_ctrl;
    // record reply builder (wq_reply.hip): per handle the scan state, term, size and two u64 prefixes; per
    // message the first occurrence of each record shape; sizes and the error word are the frame builder's
    wq::DevBuf rp_ws;
    // tick sends (wq_sends.hip): the regions and their prefixes on the device, the counters, and the pinned
    // buffer the regions are uploaded from with the event of the latest copy out of it
    wq::DevBuf snd_tab, snd_ctrl;
    void* snd_pinned = nullptr;
    size_t snd_pinned_bytes = 0;
    hipEvent_t snd_ev = nullptr;
    bool snd_pending = false;
    wq::RecStore* rec = nullptr;  // wq_records_open: rows, views, dead list and a call's scratch
    wq::ExportWs exp;             // wq_table_export*
};

namespace wq {
inline TableView table_view(const wq_router* h) {
    TableView v;
    v.recs = h->tab.recs.as<Record>();
    v.rec_mask = h->tab.rec_cap - 1;
    v.rec_shift = h->tab.rec_shift;
    v.slots = h->tab.slots.as<Slot>();
    v.slot_mask = h->tab.cap - 1;
    v.slot_shift = h->tab.shift;
    v.hash_mask = h->hash_mask;
    v.list = h->tab.list.as<uint32_t>();
    v.sf = (double)h->cube_size;
    v.ppos = h->ppos.as<double>();
    v.ppos4 = h->ppos4.as<float4>();
    v.pcode = h->n_ppos ? h->pcode.as<uint32_t>() : nullptr;
    v.qbox = h->qbox.p ? reinterpret_cast<const double*>(h->qbox.as<uint64_t>() + 6) : nullptr;
    v.n_ppos = (uint32_t)h->n_ppos;
    v.r2 = h->radius > 0.0 ? h->radius * h->radius : -1.0;
    v.n_pbox = h->tab.n_pbox;
    v.pbox = h->tab.n_pbox ? h->tab.pbox.as<uint32_t>() : nullptr;
    v.pbox_valid = h->tab.n_pbox ? h->tab.pbox.as<uint32_t>() + (uint64_t)kBoxWords * h->tab.n_pbox : nullptr;
    v.stale = h->tab.stale.as<uint32_t>();
    v.hdr = h->tab.hdr_ok ? h->tab.hdr.as<uint4>() : nullptr;
    v.hdr_mask = h->tab.hdr_cap ? h->tab.hdr_cap - 1 : 0;
    v.hdr_shift = h->tab.hdr_shift;
    v.hdr_blk = h->tab.hdr_blk;
    return v;
}
// Sticky {error OR, overflow OR} words of every route / global call since the last
// wq_route_health: the first 8 bytes of the route workspace (route_counters allocates it).
inline uint32_t* route_health(wq_router* h) { return h->rws.buf.as<uint32_t>(); }
// wq_route.hip
int route_config_count();
// 256-message tiles per block of a count or emit pass over `tiles` tiles: one for a short tick, two
// otherwise (the grid strides over the rest) — launch_route's shapes, shared with the sharded passes
uint32_t route_tiles_per_block(uint32_t tiles);
// The tick's counter slots (this call's, the next call's); *cur == nullptr when M == 0 (offsets[0]
// and both slots zeroed, nothing left to launch).
int route_counters(wq_router* h, size_t M, uint32_t* d_offsets, wq_route_counters** cur, wq_route_counters** nxt);
int launch_route(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                 const uint32_t* d_sender, const uint8_t* d_repl, size_t M, uint32_t* d_offsets,
                 uint32_t* d_peers, uint32_t* d_msgs, size_t capacity);
// wq_shard.hip (what each computes: at its definition)
struct SlotLayout;  // route_common.hpp
int launch_shard_messages(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                          const uint32_t* d_sender, const uint8_t* d_repl, size_t M, uint32_t G, wq_msg_rec* d_out,
                          uint32_t* d_counts);
int launch_budget_slots(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                        const uint32_t* d_sender, const uint8_t* d_repl, size_t M, uint32_t G, uint32_t me,
                        const SlotLayout& L, uint32_t* d_slots, uint32_t* d_perm, uint32_t* d_a, int phases,
                        bool hist_ready = false, bool own_too = false, uint32_t* own_slots = nullptr,
                        uint32_t* own_perm = nullptr, uint32_t* zero_e = nullptr, bool row_any = false,
                        uint32_t own_budget = 0xFFFFFFFFu, uint32_t* a_self = nullptr);
uint32_t budget_slot_tile();
int launch_route_records(wq_router* h, const wq_msg_rec* d_recs, size_t M, uint32_t* d_offsets, uint32_t* d_peers,
                         uint32_t* d_msgs, size_t capacity);
int launch_op_owner(wq_router* h, const wq_op* d_ops, size_t n, uint32_t G, uint32_t* d_owner);
// wq_table.hip
// ops on the host (copied to h->d_ops) or, with on_device, a device array the batch is read from
// (validated on the device: no REMOVE_PEER, no reserved world id).
int table_apply_segment(wq_router* h, const wq_op* ops, size_t n, bool on_device = false);
// keys: sorted unique (world << 32 | peer); world == WQ_WORLD_INVALID removes the peer everywhere.
int table_remove_peers(wq_router* h, const uint64_t* keys_sorted_unique, size_t n);
// The same for the peers whose bit is set in a device bitmap of n_ids bits, removed from every world;
// nothing is uploaded or waited for. d_count (nullable): a device word, 0 = no bit is set.
int table_remove_peers_device(wq_router* h, const uint32_t* d_bits, uint32_t n_ids, const uint64_t* d_count);
int table_rebuild_derived(wq_router* h);
// wq_delta.hip. Applies n subscribe / unsubscribe ops (h->cur_ops) to the records and lists in
// place; *applied = false (and nothing changed) when the batch needs the full rebuild.
int table_apply_delta(wq_router* h, size_t n, bool* applied);
// REMOVE_PEER in place: keys sorted unique (world << 32 | peer), world WQ_WORLD_INVALID = every
// world; one pass over every cube's list (wq_delta.hip).
int table_remove_peers_inplace(wq_router* h, const uint64_t* keys, size_t n);
// The same pass for a bitmap already on the device (n_ids bits): asynchronous, nothing uploaded. With
// d_count given and *d_count == 0 every block returns before it touches the table.
int table_remove_peers_bits(wq_router* h, const uint32_t* d_bits, uint32_t n_ids, const uint64_t* d_count);
// Folds the device-side entry / live-cube deltas of incremental batches into st.n / tab.n_cubes
// (synchronises the stream).
int table_sync_delta_stats(wq_router* h);
// Folds in the in-flight incremental batch (blocking: waits for it; otherwise only if it has
// finished) and re-applies it through the rebuild if the device could not apply it.
int table_resolve(wq_router* h, bool blocking);
// Regenerates `st` (grouped by cube, peers ascending) from the records, slots and lists.
int table_materialize(wq_router* h);
// Rebuilds the any-keys if incremental updates left them stale.
int table_ensure_any(wq_router* h);
int set_error(wq_router* h, int code, const char* what, hipError_t e = hipSuccess);
// wq_shard_exchange.hip: frees the exchange and its workspace (destroys an RCCL communicator).
void shard_release(wq_router* h);
// wq_follow.hip: frees the follow state and its scratch.
void follow_release(wq_router* h);
// wq_csr_diff.hip: the diff of two ticks' CSRs on device arrays (asynchronous; own: the counters
// also go to the handle's scratch, after the two error slots of diff_err), and its scratch's release.
int launch_csr_diff(wq_router* h, size_t n_rows, const uint32_t* d_old_offsets, const uint32_t* d_old_peers,
                    size_t old_capacity, const uint32_t* d_new_offsets, const uint32_t* d_new_peers,
                    size_t new_capacity, uint32_t* d_ent_offsets, uint32_t* d_ent_peers, size_t ent_capacity,
                    uint32_t* d_left_offsets, uint32_t* d_left_peers, size_t left_capacity,
                    wq_diff_counters* d_counters, bool own);
void csr_diff_release(wq_router* h);
// wq_budget.hip: the send budgets on device arrays (asynchronous; the positions already resolved),
// and its scratch's release.
int launch_peer_budget(wq_router* h, const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers,
                       size_t n_in, const double* d_msg_pos, size_t n_msgs, const double* d_peer_pos,
                       size_t n_peer_pos, uint32_t k, const uint32_t* d_budget, uint32_t* d_out_offsets,
                       uint32_t* d_out_msgs, wq_budget_counters* d_counters);
int launch_peer_budget_bytes(wq_router* h, const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers,
                             size_t n_in, const double* d_msg_pos, const uint32_t* d_msg_size, size_t n_msgs,
                             const double* d_peer_pos, size_t n_peer_pos, uint64_t w, const uint64_t* d_budget_bytes,
                             uint32_t* d_out_offsets, uint32_t* d_out_msgs, uint64_t* d_out_bytes,
                             wq_budget_bytes_counters* d_counters);
void budget_release(wq_router* h);
// wq_rotate.hip: the fair share on device arrays (asynchronous), and its scratch's release.
int launch_peer_rotate(wq_router* h, const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers,
                       size_t n_in, const uint32_t* d_kept_offsets, const uint32_t* d_kept_msgs, size_t n_kept_in,
                       const uint32_t* d_msg_size, size_t n_msgs, uint32_t r, const uint32_t* d_extra, uint64_t v,
                       const uint64_t* d_extra_bytes, uint32_t* d_cursor, uint32_t* d_out_offsets,
                       uint32_t* d_out_msgs, uint64_t* d_out_bytes, wq_rotate_counters* d_counters);
void rotate_release(wq_router* h);
// wq_pack.hip: the send buffers on device arrays (asynchronous), and its scratch's release.
int launch_peer_pack(wq_router* h, const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers, size_t n_in,
                     const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n_msgs, size_t n_frame_bytes,
                     uint32_t flags, uint8_t* d_out, size_t capacity_bytes, uint64_t* d_out_peer_bytes,
                     uint64_t* d_out_elem_bytes, wq_pack_counters* d_counters);
void pack_release(wq_router* h);
// wq_frames.hip: the world table's check and upload, the frame builder on device arrays (asynchronous),
// and the release of both.
bool frames_worlds_valid(const char* names, const uint32_t* name_offsets, uint32_t n_worlds);
int frames_set_worlds(wq_router* h, const char* names, const uint32_t* name_offsets, uint32_t n_worlds);
int launch_frames_build(wq_router* h, const wq_frames_src* src, size_t n_msgs, uint8_t* d_frames, size_t capacity_bytes,
                        uint64_t* d_frame_offsets, uint32_t* d_frame_size, wq_frames_counters* d_counters);
void frames_release(wq_router* h);
// wq_decode.hip: the world table's lookup order (enqueued on the stream by frames_set_worlds between its
// two waits; off is rebased to 0), the sender table, the decoder on device arrays (asynchronous), and
// the release of all three.
int ingest_set_world_index(wq_router* h, const uint8_t* names, const uint32_t* off, uint32_t n_worlds);
int ingest_set_peers(wq_router* h, const uint8_t* uuids, const uint32_t* ids, uint32_t n);
int launch_frames_decode(wq_router* h, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n_frames,
                         size_t n_frame_bytes, const wq_ingest_out* out, wq_ingest_counters* d_counters);
void ingest_release(wq_router* h);
// wq_join.hip: the sender table's reserve and read (both wait for the stream), the join and the drop on
// device arrays (asynchronous; arguments validated), and the release of their scratch.
int ingest_peers_reserve(wq_router* h, size_t capacity);
int ingest_peers_read(wq_router* h, uint8_t* uuids, uint32_t* ids, size_t capacity, size_t* n);
int launch_ingest_join(wq_router* h, const wq_join_in* in, size_t n_frames, const wq_join_out* out,
                       wq_join_counters* d_counters);
int launch_ingest_drop(wq_router* h, const uint32_t* d_ids, size_t n, wq_join_counters* d_counters);
void join_release(wq_router* h);
// wq_leave.hip: the leaves on device arrays (asynchronous; arguments validated) and the release of their
// scratch.
int launch_ingest_leave(wq_router* h, const wq_leave_in* in, const wq_leave_out* out, wq_leave_counters* d_counters);
void leave_release(wq_router* h);
// wq_dispatch.hip: the dispatch on device arrays (asynchronous) and the release of its scratch.
int launch_ingest_dispatch(wq_router* h, const wq_dispatch_in* in, size_t n_frames, const wq_dispatch_out* out,
                           wq_dispatch_counters* d_counters);
void dispatch_release(wq_router* h);
// wq_recdispatch.hip: the record dispatch on device arrays (asynchronous; arguments validated, a store is
// open) and the release of its scratch. It takes the tables from wq_decode.hip (ingest_tables) and the
// open store's configuration from wq_records.hip (records_config: false without a store).
int launch_records_dispatch(wq_router* h, const wq_recdisp_in* in, const wq_recdisp_out* out,
                            wq_recdisp_counters* d_counters);
void recdispatch_release(wq_router* h);
// wq_slab.hip: the slab store on device arrays (asynchronous; arguments validated) and its scratch's release.
int launch_slab_store(wq_router* h, const wq_rec_op* d_ops, const wq_rec_op_ref* d_op_ref, size_t n_ops,
                      const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n_frames, const wq_slab_view* view,
                      uint64_t* d_cursor, wq_slab_counters* d_counters);
void slab_release(wq_router* h);
// wq_slab_compact.hip: the slab's compaction on device arrays (asynchronous; arguments validated) and its release.
int launch_slab_compact(wq_router* h, const wq_slab_view* src, const wq_slab_view* dst, uint64_t* d_dst_cursor,
                        wq_slab_compact_counters* d_counters);
void slab_compact_release(wq_router* h);
// wq_reply.hip: the record reply builder on device arrays (asynchronous; arguments validated) and its release.
int launch_frames_build_records(wq_router* h, const wq_frames_src* src, const wq_frames_rec_src* rec, size_t n_msgs,
                                uint8_t* d_frames, size_t capacity_bytes, uint64_t* d_frame_offsets, uint32_t* d_frame_size,
                                wq_frames_counters* d_counters);
void reply_release(wq_router* h);
// wq_sends.hip: the tick sends on device arrays (asynchronous; the regions are checked there) and the
// release of its scratch, staging buffer and event.
int launch_tick_sends(wq_router* h, const wq_tick_sends_in* in, uint32_t* d_peer_offsets, uint32_t* d_frames_out,
                      size_t n_elems, wq_tick_sends_counters* d_counters);
void sends_release(wq_router* h);
void ingest_tables(const wq_router* h, DecTables* t);
bool records_config(const wq_router* h, RecCfg* cfg);
// wq_records.hip: frees the record store.
void records_release(wq_router* h);
// wq_table_export.hip: frees the export's scratch.
void export_release(wq_router* h);
// wq_multi.hip: the sub-handles of a multi-GPU handle (the export walks them itself)
uint32_t multi_subs(wq_router* h, wq_router*** sub, const int** dev, int* mode);
// wq_multi.hip: the multi-GPU handle's side of the entry points (h->multi != nullptr)
int multi_merge_any(wq_router* h);
int multi_apply_ops(wq_router* h, const wq_op* ops, size_t n);
int multi_apply_ops_device(wq_router* h, const wq_op* d_ops, size_t n);
int multi_remove_peers(wq_router* h, const uint32_t* peers, size_t n);
int multi_route_tick(wq_router* h, const double* pos, const int64_t* keys, const uint32_t* world,
                     const uint32_t* sender, const uint8_t* repl, size_t M, uint32_t* offsets, uint32_t* peers,
                     uint32_t* msgs, size_t capacity, size_t* n_pairs, bool on_device);
int multi_route_slices(wq_router* h, const wq_msg_slice* in, int with_msgs, wq_slice_view* out);
int multi_is_subscribed(wq_router* h, size_t n, const uint32_t* world, const uint32_t* peer, int raw,
                        const void* kp, uint8_t* out);
int multi_stats(wq_router* h, wq_stats* out);
int multi_health(wq_router* h, uint32_t* error_bits, uint32_t* overflow);
int multi_set_positions(wq_router* h, const double* pos, size_t n, bool on_device);
int multi_set_radius(wq_router* h, double radius);
int multi_set_hint(wq_router* h, double pairs_per_message);
void multi_release(wq_router* h);
}  // namespace wq

#define WQ_HIP(h, call)                                                    \
    do {                                                                   \
        hipError_t e_ = (call);                                            \
        if (e_ != hipSuccess) return wq::set_error((h), WQ_E_HIP, #call, e_); \
    } while (0)

#define WQ_ALLOC(h, buf, bytes)                                                     \
    do {                                                                            \
        hipError_t e_ = (buf).ensure(bytes);                                        \
        if (e_ != hipSuccess) return wq::set_error((h), WQ_E_OOM, "hipMalloc " #buf, e_); \
    } while (0)

inline int wq::ZeroedBuf::prepare(wq_router* h, size_t need, hipStream_t stream) {
    const size_t cap = b.bytes;
    WQ_ALLOC(h, b, need);
    if (b.bytes != cap) clean = 0;
    if (clean < b.bytes) {
        WQ_HIP(h, hipMemsetAsync(b.p, 0, b.bytes, stream));
        clean = b.bytes;
    }
    return WQ_OK;
}
