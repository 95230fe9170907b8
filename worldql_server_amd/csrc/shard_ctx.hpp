// shard_ctx.hpp — what the sharded tick's translation units share: the exchange a handle is
// attached to with its workspace (ShardCtx), one exchange's description (Xfer), and the helpers of
//   wq_shard_exchange.hip  the transports (hub, RCCL, the caller's callback), attach / release
//   wq_sharded.hip         the expanded-record tick, wq_sharded_copy_out
//   wq_sharded_slots.hip   the slot tick and the owner form on slots
// Internal to the library: nothing here is part of the C ABI (include/wq_router.h).
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "route_async.hpp"

namespace wq {

constexpr int kXNone = 0, kXHub = 1, kXRccl = 2, kXCallback = 3;

// Record index bounds of each source shard's segment of the received records (kernel argument).
struct SegBounds {
    uint32_t b[WQ_MAX_SHARDS + 1];
};

// One exchange of n buffers: buffer k sends sbytes[k][d] bytes to rank d (segments contiguous in
// rank order from send[k]) and receives rbytes[k][s] from rank s into recv[k].
struct Xfer {
    const void* send[3];
    const size_t* sbytes[3];
    void* recv[3];
    const size_t* rbytes[3];
    int n;
    // buffer k's self segment is already in place in recv[k] (RCCL and hub exchanges only): not copied
    bool skip_self[3] = {false, false, false};
};

struct ShardCtx {
    uint32_t G = 1, rank = 0;
    int kind = kXNone;
    wq_hub* hub = nullptr;
    ncclComm_t comm = nullptr;
    wq_exchange_fn fn = nullptr;
    void* fn_ctx = nullptr;
    // workspace of the expanded-return tick (radius filter on) and the owner form
    DevBuf recs, recv, own_off, own_peers, own_e, ret_e, ret_off, ret_peers, by_msg, tmp, small;
    uint64_t own_cap = 0;
    std::vector<uint32_t> sc, rc;
    // workspace of the slot tick (compact slots out, row references + cube-list pools back)
    DevBuf slots, perm, rslots, ocnt, hslot, plen, poff, claim, lead, ref_send, ref_recv, pool_send, pool_recv,
        desc_fill, e_msg, info_msg, mtiles, otiles, blk;
    // own slots (the default with G > 1, no radius): this shard's own messages as slots of a segment
    // that is never exchanged, its slot -> message map, and the scratch tile sums of their count
    DevBuf own_slots, own_perm, own_tiles;
    // every DevBuf above, for shard_release: a buffer added to the lists above is added here
    std::vector<DevBuf*> bufs() {
        return {&recs,     &recv,      &own_off,   &own_peers, &own_e,     &ret_e,     &ret_off,   &ret_peers,
                &by_msg,   &tmp,       &small,     &slots,     &perm,      &rslots,    &ocnt,      &hslot,
                &plen,     &poff,      &claim,     &lead,      &ref_send,  &ref_recv,  &pool_send, &pool_recv,
                &desc_fill, &e_msg,    &info_msg,  &mtiles,    &otiles,    &blk,       &own_slots, &own_perm,
                &own_tiles};
    }
    // which form the budgets above were derived from (0 the slot tick, 1 wq_sharded_route_owner_slots)
    int budget_form = 0;
    uint64_t claim_cap = 0;  // claim table entries (power of two); 0 = not allocated
    uint64_t ticks = 0;      // slot ticks run: the claim table's tag
    // exchange budgets of the slot tick, identical on both ends of every pair: slots me -> d and
    // s -> me (whole 256-slot blocks; 0 for this shard itself), pool words me -> s and o -> me. Set
    // from the previous tick's true sizes with headroom; without them (first tick, or after a tick
    // whose sizes outgrew them) the tick runs exact, reading the sizes back twice.
    std::vector<uint32_t> b1_out, b1_in;
    std::vector<uint64_t> b2_out, b2_in;
    bool budgets = false;
    uint64_t n_exact = 0, n_budget = 0;  // slot ticks of each kind (wq_shard_tick_stats)
    void* hsmall = nullptr;              // pinned copy of the small vectors at the end of a tick
    hipStream_t side = nullptr;          // the own-cube count pass, beside the exchanges
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_ready = nullptr, ev_done = nullptr;
    // bytes this shard sent to / received from OTHER shards in its latest tick (xGMI volume)
    uint64_t last_sent = 0, last_recv = 0;
    // the latest tick, kept for wq_sharded_copy_out after WQ_E_CAPACITY
    uint64_t last_M = 0, last_P = 0;
    bool last_ready = false;
    bool last_slots = false;  // the latest tick was a slot tick (copy_out = scan + emit of its rows)
    uint64_t last_gen = 0;    // its table generation: its own-cube rows point into the table
    const uint32_t* last_sender = nullptr;  // its d_sender (OnlySelf rows read the sender)
    const double* last_pos = nullptr;       // radius filter on: its positions and replication codes
    const uint8_t* last_repl = nullptr;     // (the emit re-filters list and pool rows)
    bool last_radius = false;
    // wq_sharded_route_tick_async: pinned snapshots of the small vectors of ticks not read back yet,
    // oldest first (a ring); every call drains them in the same order on every shard, so the budgets
    // derived from them stay identical on both ends of every pair
    // (mapped pinned memory the tick's last kernel writes itself, then a sequence word: no copy
    // launch and no event, each of which costs the stream a ~7 us bubble)
    static constexpr uint32_t kRing = 4;
    void* asnap[kRing] = {};
    uint64_t aseq[kRing] = {};  // the sequence number snapshot k completes with
    uint32_t ahead = 0, acount = 0;
    uint64_t n_async = 0;
    bool small_zeroed = false;  // the last tick's k_async_result left the small vectors zero
};

// A tick's local failure. Every rank makes the same exchanges whether its own steps failed or not
// (no peer is left waiting), so a failed step is only noted — the first one, with its message —
// and reported once the tick's exchanges are complete.
struct Late {
    int code = WQ_OK;
    std::string msg;
    explicit operator bool() const { return code != WQ_OK; }
    int fail(wq_router* h, int rc) {
        if (rc && !code) {
            code = rc;
            msg = h->err;
        }
        return rc;
    }
    int report(wq_router* h) const {
        h->err = msg;
        return code;
    }
};

// What every tick entry point checks of its message arrays.
inline int check_tick_msgs(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                           const uint32_t* d_sender, const uint8_t* d_repl, size_t n_msgs) {
    if (!h || (n_msgs && (!d_world || !d_sender || !d_repl || (!d_pos && !d_keys)))) return WQ_E_INVALID;
    if (n_msgs >= 0xFFFFFC00ull) return set_error(h, WQ_E_INVALID, "n_msgs must be < 2^32 - 1024 per tick");
    return WQ_OK;
}
// ... and of its output buffers (the two CSR forms)
inline int check_csr_tick(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                          const uint32_t* d_sender, const uint8_t* d_repl, size_t n_msgs, const uint32_t* d_offsets,
                          const uint32_t* d_peers, size_t capacity) {
    if (!d_offsets || (capacity && !d_peers)) return WQ_E_INVALID;
    return check_tick_msgs(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs);
}
// ... or of its view, zeroed, on an attached handle (the three owner forms)
template <class View>
inline int begin_owner_tick(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                            const uint32_t* d_sender, const uint8_t* d_repl, size_t n_msgs, View* out) {
    if (!out) return WQ_E_INVALID;
    if (int rc = check_tick_msgs(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs)) return rc;
    WQ_HIP(h, hipSetDevice(h->device));
    if (!h->shard) return set_error(h, WQ_E_INVALID, "no exchange attached (wq_shard_attach_*)");
    memset(out, 0, sizeof(*out));
    return WQ_OK;
}

#pragma GCC visibility push(hidden)
// wq_shard_exchange.hip
int exchange(wq_router* h, const Xfer& x);
int scan_excl(wq_router* h, DevBuf& tmp, const uint32_t* in, uint32_t* out, size_t n);
// Blocks of a sharded count or emit pass over n tiles, shaped as launch_route's (WQ_DEBUG_SHARD_TPB:
// tiles per block, diagnostics)
uint32_t pass_blocks(uint32_t n);
// A receive buffer could not be allocated after the peers were told what they will send: the
// collective cannot complete. The hub is marked broken (its peers fail at their next wait instead
// of timing out); an RCCL or callback caller has to abandon its communicator.
int fatal_receive(wq_router* h, const char* what);
// Status word of a failed local step as the exchanges carry it (the negated WQ_E_* code).
inline uint32_t status_of(int rc) { return (uint32_t)(-rc); }
// The error a shard reports for a status word it received (its own or a peer's): counter bits
// << 32 (4 spin, 2 > 2^32 pairs, 8 stale table) or a negated WQ_E_* code.
int status_error(wq_router* h, uint64_t st, uint32_t from);
// wq_sharded_slots.hip: the slot tick's CSR from its kept rows (ar: an asynchronous tick's end)
int slots_copy_out(wq_router* h, uint32_t* d_offsets, uint32_t* d_peers, uint32_t* d_msgs, size_t capacity,
                   const AsyncResultParams* ar = nullptr, bool* ar_done = nullptr);
// wq_sharded.hip: the latest tick into the caller's buffers (message order), either form
int copy_out(wq_router* h, uint32_t* d_offsets, uint32_t* d_peers, uint32_t* d_msgs, size_t capacity);
// wq_sharded_slots.hip: the slot tick behind wq_sharded_route_tick_device (async: ..._tick_async)
int sharded_tick_slots(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                       const uint32_t* d_sender, const uint8_t* d_repl, size_t M, uint32_t* d_offsets,
                       uint32_t* d_peers, uint32_t* d_msgs, size_t capacity, size_t* n_pairs, bool async = false,
                       wq_route_counters* d_result = nullptr);
#pragma GCC visibility pop

}  // namespace wq
