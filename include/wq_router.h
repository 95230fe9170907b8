/*
 * wq_router.h — C ABI of the MI355X-native WorldQL spatial message-routing path.
 *
 * This is the drop-in boundary for the reference server's subscription table
 * (worldql_server/src/subscriptions/{world_map,area_map,cube_area}.rs) and the
 * LocalMessage / AreaSubscribe / AreaUnsubscribe handlers that drive it
 * (worldql_server/src/processing/{local_message,area_subscribe,area_unsubscribe}.rs).
 * The reference has no FFI for this path (it is plain Rust methods);
 * each entry point below names the Rust method(s) it replaces, and INTEGRATION.md shows
 * the `extern "C"` block a `worldql_gpu` crate would declare to bind them.
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns an int status (WQ_OK = 0,
 *     negative WQ_E_* on failure). No exception or panic crosses the ABI.
 *   - peers are dense uint32 ids (the Rust side keeps the Uuid <-> u32 map);
 *     worlds are dense uint32 ids interned on the host from the *sanitized* world name
 *     (worldql_server/src/utils/world_names.rs:54-87). WQ_WORLD_INVALID is reserved.
 *   - a handle is owned by one thread (Send, not Sync), mirroring the single owner task of
 *     WorldMap in worldql_server/src/processing/thread.rs:113-148.
 *   - functions without the `_device` suffix take HOST pointers and are synchronous;
 *     `_device` variants take DEVICE pointers and are asynchronous on the handle's stream.
 */
#ifndef WQ_ROUTER_H
#define WQ_ROUTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define WQ_OK 0
#define WQ_E_INVALID (-1)  /* bad argument (null handle, cube_size 0, reserved world id ...) */
#define WQ_E_OOM (-2)      /* device allocation failed */
#define WQ_E_HIP (-3)      /* HIP runtime error (message in wq_last_error) */
#define WQ_E_RCCL (-4)     /* the multi-GPU exchange failed (RCCL, hub timeout, caller callback) */
#define WQ_E_CAPACITY (-5) /* caller's output buffer too small; required size reported */
#define WQ_E_NODEV (-6)    /* no usable gfx950 device: the path never falls back to the CPU */
#define WQ_E_TIMEOUT (-7)  /* a bounded in-kernel spin gave up (must never happen) */

/* ---- op kinds (wq_op.kind) ---- */
#define WQ_OP_SUBSCRIBE 0   /* AreaMap::add_subscription, area_map.rs:72-85 */
#define WQ_OP_UNSUBSCRIBE 1 /* AreaMap::remove_subscription, area_map.rs:88-119 */
#define WQ_OP_REMOVE_PEER 2 /* world == WQ_WORLD_INVALID: WorldMap::remove_peer (world_map.rs:41-61);
                             otherwise that world only: AreaMap::remove_peer (area_map.rs:124-135) */

/* ---- replication codes, wire values of WorldQLFB_generated.rs:176-188 ---- */
#define WQ_REPL_EXCEPT_SELF 0    /* default; also every unknown code (replication.rs:40) */
#define WQ_REPL_INCLUDING_SELF 1
#define WQ_REPL_ONLY_SELF 2

#define WQ_WORLD_INVALID 0xFFFFFFFFu
#define WQ_WORLD_GLOBAL 0xFFFFFFFEu /* reserved: the "@global" world as wq_frames_decode_device reports it;
                                       never an id of the subscription table or of wq_frames_set_worlds */

typedef struct wq_router wq_router;

/* One subscription-table op (40 bytes). key_is_raw = 1 means `key` is a CubeArea used as-is
 * (impl ToCubeArea for CubeArea, cube_area.rs:65-70); 0 means `pos` is a Vector3 quantised
 * by CubeArea::from_vector3 (cube_area.rs:50-56). */
typedef struct wq_op {
    uint32_t world;
    uint32_t peer;
    uint8_t kind;
    uint8_t key_is_raw;
    uint8_t pad_[6];
    union {
        double pos[3];
        int64_t key[3];
    } u;
} wq_op;

typedef struct wq_stats {
    uint64_t n_entries;     /* live (world, cube, peer) subscriptions */
    uint64_t n_cubes;       /* occupied (world, cube) buckets */
    uint64_t n_any;         /* distinct (world, peer) pairs = sum of |subscribed_peers| */
    uint64_t table_slots;   /* open-addressed slot count (power of two) */
    uint64_t hash_fallbacks;/* builds that hit a 64-bit hash collision and took the exact path */
    uint32_t cube_size;
    int32_t device;
} wq_stats;

/* Per-call route counters written by the route kernel (device memory, see wq_route_tick_device). */
typedef struct wq_route_counters {
    uint64_t n_pairs;      /* P: (message, peer) pairs after the replication filter */
    uint64_t n_candidates; /* F: peers read from the probed buckets before the filter */
    uint32_t overflow;     /* 1 if P exceeded the caller's capacity (outputs truncated) */
    uint32_t error;        /* 4: a bounded spin gave up (WQ_E_TIMEOUT); 2: P > 2^32-1 (WQ_E_CAPACITY);
                              8: the table is missing an incremental batch the device could not
                              apply (re-applied by the next wq_apply* / query call) */
} wq_route_counters;

/* ---- pinned host memory for the host-array entry points: buffers from wq_host_alloc move over
 * PCIe by DMA without a staging copy (pageable buffers work too, at a fraction of the rate). */
int wq_host_alloc(size_t bytes, void** out);
int wq_host_free(void* p);

/* ---- lifetime: replaces WorldMap::new (world_map.rs:17-22) ---- */
int wq_router_create(uint16_t cube_size, int device, wq_router** out);
/* The same table over n_gpus GPUs behind ONE handle (SURVEY.md §8(b) wq_router_create(cube_size,
 * n_gpus, devices, out)); the reference's single owner (thread.rs:119) keeps its one WorldMap.
 * Inside: one cube-hash shard per device (devices may repeat), attached to an in-process exchange,
 * driven by one worker thread each; every call below gives the one-table result:
 *   wq_apply_ops[_device], wq_remove_peers   the whole op stream to every shard (each keeps its cubes)
 *   wq_route_tick[_device]                   the sharded tick over G slices of the messages, CSR
 *                                            concatenated in message order (n_candidates = P)
 *   wq_is_subscribed[_any], wq_world_peers,  shard answers combined (any-keys merged on devices[0])
 *   wq_route_global[_device], wq_get_stats
 *   wq_set_radius, wq_set_peer_positions[_device], wq_set_fanout_hint, wq_route_health: every shard
 * Device-pointer calls take arrays on devices[0], ordered after the handle's stream (wq_set_stream),
 * and are synchronous on return — except wq_apply_ops_device, which keeps the single-GPU contract:
 * an invalid batch is not applied and shows as error bit 16 of wq_route_health (the call returns
 * WQ_OK); on the replicate layout it is also asynchronous. The cube-hash layout partitions a device
 * batch by owner on devices[0] (one read-back of the per-shard counts). The sharded entry points
 * (wq_shard_*, wq_sharded_*) and the instrumentation hooks are for single-device handles. */
int wq_router_create_multi(uint16_t cube_size, int n_gpus, const int* devices, wq_router** out);
/* The same with the layout chosen (wq_router_create_multi = WQ_MULTI_CUBE_HASH):
 *   WQ_MULTI_CUBE_HASH  the table partitioned by cube hash, as above (tables beyond one GPU's HBM);
 *   WQ_MULTI_REPLICATE  every device holds the WHOLE table and routes its own slice of a tick with
 *                       the single-GPU tick — no exchange at all (C3's table is ~10 GB of 288 GB).
 *                       Every op is applied on every device (the op stream is the only thing all
 *                       devices see); wq_apply_ops_device stays asynchronous; queries go to device 0.
 * Results are the one-table results either way. */
#define WQ_MULTI_CUBE_HASH 0
#define WQ_MULTI_REPLICATE 1
int wq_router_create_multi_mode(uint16_t cube_size, int n_gpus, const int* devices, int mode, wq_router** out);
/* Sub-handles behind a handle (1 for wq_router_create), and the layout (-1 for a single-GPU handle). */
int wq_multi_info(wq_router* h, uint32_t* n_gpus);
int wq_multi_mode(wq_router* h, int* mode);
/* The scaling form of a multi-GPU tick: every device routes the messages it ingested and keeps its
 * CSR (no pair crosses to devices[0]). in[g] = the messages on devices[g] (device pointers there,
 * complete before the call; keys or positions as wq_route_tick); out[g] = views into the handle's
 * workspace on devices[g] (a staging of their own), valid until the next wq_route_tick_slices_device
 * call on the handle or its destruction — every other call (routes, queries, op batches) leaves
 * them intact: offsets[n_msgs + 1] (from 0),
 * peers[n_pairs], msgs[n_pairs] (the index within the slice; NULL unless with_msgs). Per message
 * the recipients are exactly wq_route_tick's for the same message on one table. Synchronous. */
typedef struct wq_msg_slice {
    const double* d_pos;
    const int64_t* d_keys;
    const uint32_t* d_world;
    const uint32_t* d_sender;
    const uint8_t* d_repl;
    uint64_t n_msgs;
} wq_msg_slice;
typedef struct wq_slice_view {
    int32_t device;
    uint32_t pad_;
    uint64_t n_msgs;
    uint64_t n_pairs;
    const uint32_t* offsets;
    const uint32_t* peers;
    const uint32_t* msgs;
} wq_slice_view;
int wq_route_tick_slices_device(wq_router* h, const wq_msg_slice* in, int with_msgs, wq_slice_view* out);
int wq_router_destroy(wq_router* h);
const char* wq_last_error(const wq_router* h);
/* Use the caller's HIP stream (hipStream_t as void*); NULL restores the handle's own stream. */
int wq_set_stream(wq_router* h, void* hip_stream);
int wq_get_stats(wq_router* h, wq_stats* out);

/* ---- table mutation: AreaSubscribe / AreaUnsubscribe / disconnect ----
 * Ops are applied in ARRAY ORDER with the reference's sequential semantics
 * (processing/thread.rs:122-146): for each (world, cube, peer) the last op wins, and a
 * REMOVE_PEER op removes every subscription its peer holds at that point.
 * Replaces area_subscribe.rs:137-138 / area_unsubscribe.rs:189-190 -> AreaMap::{add,remove}_subscription
 * and thread.rs:124-125 -> WorldMap::remove_peer. */
int wq_apply_ops(wq_router* h, const wq_op* ops, size_t n);
/* The same for a batch already in device memory (e.g. assembled by the caller's own kernels):
 * subscribe / unsubscribe ops only — a REMOVE_PEER op or the reserved world id fails the whole
 * batch with WQ_E_INVALID before anything changes (use wq_remove_peers for disconnects).
 * Asynchronous: an incremental batch (up to 1/4 of the table's entries) is enqueued on the
 * handle's stream, before any later tick, and the call returns without waiting for the GPU; the
 * NEXT call on the handle folds its status in (waiting only for that batch, not for later work).
 * Keep d_ops unchanged until that next call has returned: a batch the device could not apply
 * (an op whose key has no packed form — NaN / huge coordinates, off-grid raw keys, world ids
 * >= 2^24 - 1 — or list space exhausted) is re-applied from it by the rebuild then, and routes
 * issued in between report error bit 8 (WQ stale table) in their counters and in
 * wq_route_health. A batch holding an invalid op (REMOVE_PEER kind, reserved world) is not applied at
 * all (the table stays as before it); the next call on the handle still does its own work in full
 * and leaves the rejection in wq_last_error and as error bit 16 of wq_route_health. */
int wq_apply_ops_device(wq_router* h, const wq_op* d_ops, size_t n);
/* WorldMap::remove_peer for n peers (every world), world_map.rs:41-61. */
int wq_remove_peers(wq_router* h, const uint32_t* peers, size_t n);

/* ---- the hot path: one tick of LocalMessages ----
 * Replaces the per-message body of handle_local_message (local_message.rs:52-86):
 * world lookup -> Vector3::to_cube_area -> AreaMap::get_subscribed_peers -> replication filter.
 * Validation (@global, missing position, bad world name: local_message.rs:17-50) stays on the
 * host, before the call. Output: message-major CSR, offsets[M+1] and peers[P]; msgs[P]
 * (nullable) repeats the message index of each pair. Pair order inside one message is
 * ascending peer id (the reference's AHashSet order is random per process: compare sets).
 * keys (nullable, M x 3 int64) replaces pos with raw CubeArea keys (ToCubeArea for CubeArea). */
int wq_route_tick(wq_router* h, const double* pos, const int64_t* keys, const uint32_t* world,
                  const uint32_t* sender, const uint8_t* repl, size_t n_msgs, uint32_t* offsets,
                  uint32_t* peers, uint32_t* msgs, size_t capacity, size_t* n_pairs);
/* Asynchronous form on device pointers; nothing is read back. counters (device pointer to a
 * wq_route_counters) receives P, F and the overflow / error flags (also kept sticky for
 * wq_route_health). Pairs beyond `capacity` are not written.
 * A tick whose P exceeds `capacity` still completes (tests/test_gpu_truncation.py):
 *   - d_offsets[0 .. n_msgs] are complete: d_offsets[n_msgs] = P, not clipped to `capacity`;
 *   - d_peers / d_msgs hold exactly the first `capacity` pairs of the full result (the last message
 *     kept may be cut inside its recipients); nothing at index >= capacity is written, and with
 *     P < capacity nothing at index >= P either;
 *   - the counters carry the full P and F, overflow = 1, error = 0; wq_route_tick returns
 *     WQ_E_CAPACITY with *n_pairs = P after copying the same offsets and prefix;
 *   - capacity = 0 asks for offsets and counters only (d_peers and d_msgs are not touched);
 *   - wq_csr_diff* reads such a tick as it is, with new_capacity = `capacity`.
 * A tick whose P exceeds 2^32 - 1, the most that u32 offsets address, is reported, never mistaken for a
 * smaller one — in every tick shape, with or without the radius filter, wq_route_global* included
 * (tests/test_gpu_pair_limit.py):
 *   - counters.n_pairs is the exact P for P < 2^40 (beyond that some value >= 2^40 - 1: the
 *     single-launch tick carries 40 bits of it from block to block); n_candidates is the exact F;
 *   - counters.error has bit 2 and overflow = (P > capacity), i.e. 1 (capacities count as at most
 *     2^32 - 1); wq_route_health reports bit 2 once, then (0, 0);
 *   - d_offsets[0 .. n_msgs] are written and nothing behind them; their values are unspecified (they
 *     are the true offsets modulo 2^32);
 *   - the contents of d_peers / d_msgs are unspecified; nothing at index >= capacity is written, and
 *     with capacity 0 they are not touched;
 *   - wq_route_tick and wq_route_global return WQ_E_CAPACITY with *n_pairs = P and leave offsets,
 *     peers and msgs untouched; a multi-GPU handle (wq_router_create_multi*) returns WQ_E_CAPACITY
 *     from the host and the device form, with *n_pairs / counters.n_pairs >= 2^32;
 *   - the next tick on the handle is exact.
 * P = 2^32 - 1 is an ordinary tick: offsets[n_msgs] = 0xFFFFFFFF, error 0.
 * d_peers and d_msgs are expected 16-byte aligned, as every hipMalloc result is: the kernels store
 * 16-byte quads at pair indices that are multiples of four. */
int wq_route_tick_device(wq_router* h, const double* d_pos, const int64_t* d_keys,
                         const uint32_t* d_world, const uint32_t* d_sender, const uint8_t* d_repl,
                         size_t n_msgs, uint32_t* d_offsets, uint32_t* d_peers, uint32_t* d_msgs,
                         size_t capacity, wq_route_counters* d_counters);

/* ---- C5: exact radius filter after the cube broadphase ----
 * An extension the reference does not have (it stores no peer positions). With a radius > 0 set,
 * every subsequent tick keeps a (message, peer) pair only if additionally
 *     dx = mx - px; dy = my - py; dz = mz - pz;   (dx*dx + dy*dy) + dz*dz <= radius*radius
 * evaluated left to right in f64 without FMA contraction, m = the message position, p = the
 * peer's position from the latest wq_set_peer_positions; a peer id >= n_peers has no position and
 * is dropped. Ticks with the filter on take message positions (keys must be NULL).
 * radius <= 0 or NaN turns the filter off. The handle keeps the positions (24 B per peer) and an
 * f32 copy (16 B per peer) that decides every pair whose f64 result it can bound; the rest read
 * the f64 copy, so results are exactly the f64 predicate's. The _device form reads d_pos on the
 * handle's stream (asynchronous). */
int wq_set_peer_positions(wq_router* h, const double* pos, size_t n_peers);
int wq_set_peer_positions_device(wq_router* h, const double* d_pos, size_t n_peers);
int wq_set_radius(wq_router* h, double radius);

/* ---- follow moving peers: the subscription deltas generated on the GPU ----
 * An extension the reference does not have: there every client works out its own AreaSubscribe /
 * AreaUnsubscribe messages (area_subscribe.rs / area_unsubscribe.rs), and a host driving this table
 * would have to produce and upload one 40-byte wq_op per changed cube. Here the host hands over one
 * world id and one position per peer and the handle derives the ops itself.
 *   neighbourhood  of (world w, position p), cube size s, reach r: the cubes
 *                  CubeArea::from_vector3(p + s*d) for d in {-r..r}^3 — one f64 add per axis, no
 *                  contraction, the table's own quantiser; it can hold fewer than (2r+1)^3 cubes.
 *   follow state   per peer id the world and position it was last followed at (28 B per peer;
 *                  WQ_WORLD_INVALID = not followed). It is separate from the radius filter's
 *                  positions: wq_set_peer_positions* and the filter neither read nor write it.
 *   one call       world[n] and pos[n x 3], indexed by peer id. For every peer i < n, with O = the
 *                  neighbourhood of its stored state (empty if not followed) and N = the one of
 *                  (world[i], pos[i]) (empty if world[i] == WQ_WORLD_INVALID: stop following), the
 *                  call applies UNSUBSCRIBE for every cube of O \ N and SUBSCRIBE for every cube of
 *                  N \ O — an exact set difference, cell edges included — and then stores the new
 *                  state. Peers >= n are untouched.
 * The ops depend on the old and new follow state only, never on what the table holds:
 * subscriptions made through wq_apply_ops are not touched, and wq_remove_peers does NOT clear the
 * follow state of the peers it removes (stop following them with WQ_WORLD_INVALID, or
 * wq_follow_reset).
 * The op stream is deterministic, byte for byte: ascending peer id; within a peer the unsubscribes,
 * then the subscribes; each group in lexicographic (dx, dy, dz) order over the first offset that
 * yields each distinct cube. Ops carry key_is_raw = 0 and the offset position p + s*d — what a host
 * handler would send — so keys without a packed form (NaN, huge coordinates, world ids >= 2^24 - 1)
 * take the rebuild path they take through wq_apply_ops_device. Padding bytes are zero.
 * A call counts the ops (one lane per peer), reads the totals back (its only host read), sizes the
 * handle's op buffer exactly — WQ_E_OOM, or WQ_E_CAPACITY at more than 2^32-1 ops, is returned
 * before any follow state changes — writes the ops and the new state, and applies the ops as
 * wq_apply_ops_device does (incremental or rebuild, the same pending-batch protocol; the previous
 * batch is folded in first). The _device form reads its arrays on the handle's stream and is
 * asynchronous after the read-back: keep the arrays unchanged until the stream has passed the call;
 * a wq_route_tick_device issued right after it sees the updated table. Multi-GPU handles generate on
 * devices[0] and distribute the ops as wq_apply_ops_device does, in both layouts; the sharded
 * entry points (wq_shard_*, wq_sharded_*) have no follow form. */
typedef struct wq_follow_result {
    uint64_t n_unsubscribe; /* ops of this call */
    uint64_t n_subscribe;
    uint64_t n_followed;    /* peers followed after the call (the whole handle) */
} wq_follow_result;
/* Reach r of the neighbourhood, 0..2 (default 1: 3x3x3). Only while no peer is followed
 * (WQ_E_INVALID otherwise; reach > 2: WQ_E_INVALID). */
int wq_follow_set_reach(wq_router* h, uint32_t reach);
/* Drops all follow state; emits no op (the table keeps its subscriptions). */
int wq_follow_reset(wq_router* h);
/* out is nullable. A null array with n > 0: WQ_E_INVALID. */
int wq_follow_peers(wq_router* h, const uint32_t* world, const double* pos, size_t n, wq_follow_result* out);
int wq_follow_peers_device(wq_router* h, const uint32_t* d_world, const double* d_pos, size_t n,
                           wq_follow_result* out);
/* The ops of the latest follow call: a device pointer into the handle's op buffer (NULL when the
 * call had none), valid until the next follow call on the handle. */
int wq_follow_last_ops(wq_router* h, const wq_op** d_ops, size_t* n);
/* The same copied to host memory (synchronous); *n = the op count, WQ_E_CAPACITY if it exceeds
 * `capacity` (nothing copied). */
int wq_follow_read_ops(wq_router* h, wq_op* out, size_t capacity, size_t* n);

/* The follow state itself, so a restarted server goes on where the old one stopped (a restored table
 * with an empty follow state would subscribe every peer's whole neighbourhood again and never
 * unsubscribe the cubes it has left since).
 * wq_follow_state_read: world[n] and pos[n x 3] for the n peers the state covers (the largest n a
 * follow call or a load was given since the last reset). A peer that is not followed reads
 * WQ_WORLD_INVALID and +0.0 three times. *n is always the full count; peers at index >= capacity are
 * not written and the call returns WQ_E_CAPACITY; null arrays with capacity 0 ask for the count.
 * wq_follow_state_load: installs world[n], pos[n x 3] as the state and emits no op; n_followed
 * counts from it. Only while no peer is followed (WQ_E_INVALID otherwise, as wq_follow_set_reach).
 * The reach is not part of the state: set it first. Both are synchronous; a multi-GPU handle keeps
 * the state on devices[0]. */
int wq_follow_state_read(wq_router* h, uint32_t* world, double* pos, size_t capacity, size_t* n);
int wq_follow_state_load(wq_router* h, const uint32_t* world, const double* pos, size_t n);

/* ---- table snapshots: the subscriptions as a canonical op stream ----
 * An extension: the reference keeps its WorldMap in memory only and cannot list it.
 * Every live (world, cube, peer) that passes the filter becomes one wq_op: kind WQ_OP_SUBSCRIBE,
 * key_is_raw = 1, u.key = the CubeArea exactly as the table holds it, pad_ zero. Import is
 * wq_apply_ops[_device] of those rows into an empty handle (wq_sharded_apply_ops with the same
 * rows on every shard; the ordinary apply on a multi-GPU handle): there is no import entry point.
 * Rows ascend by (world as u32, key x, y, z as i64, peer as u32), so two handles holding the same
 * subscription set export the same bytes whatever their history (rebuilds, in-place batches,
 * relocated lists, wq_remove_peers, truncated hash bits, record slack, header layout, one GPU or
 * several). A cube whose list has been emptied yields nothing.
 *   - The pending incremental batch is folded in first: an export right after wq_apply_ops_device
 *     sees that batch.
 *   - *n is always the full row count. Rows at index >= capacity are not written and the call then
 *     returns WQ_E_CAPACITY; a null array with capacity 0 asks for the count.
 *   - Both forms are synchronous (they wait for the totals). The _device form leaves the rows in
 *     device memory (8-byte aligned) on the handle's device, devices[0] for a multi-GPU handle.
 *   - Multi-GPU: the replicate layout exports replica 0; the cube-hash layout exports every shard
 *     and merges on devices[0]. A single handle with an exchange attached (wq_shard_attach_*)
 *     exports the buckets it owns, without communication.
 * The filter: `peers` is a HOST array in both forms. */
typedef struct wq_export_filter {
    uint32_t world;        /* WQ_WORLD_INVALID: every world */
    uint32_t n_peers;
    const uint32_t* peers; /* NULL: every peer; else exactly these ids (any order, duplicates and ids
                              nobody holds allowed; n_peers may be 0) */
} wq_export_filter;        /* a NULL filter = everything */
int wq_table_export(wq_router* h, const wq_export_filter* f, wq_op* out, size_t capacity, size_t* n);
int wq_table_export_device(wq_router* h, const wq_export_filter* f, wq_op* d_out, size_t capacity, size_t* n);

/* ---- tick shape: the caller's expected recipients per message (e.g. its previous tick's
 * n_pairs / M; no reference counterpart — the Rust loop routes one message at a time,
 * thread.rs:125-146). At >= WQ_HEAVY_FANOUT the tick runs as count / scan / emit launches, whose
 * emit writes each block's outputs straight to HBM without holding a block that waits on its
 * predecessors (C3: 2.18 -> 1.76 ms); below it, the single launch (C2). Results are identical
 * either way. Until the caller sets a hint, the host-array wq_route_tick sets it itself from each
 * tick's n_pairs / M (device-pointer ticks never read their counters back, so they keep the last
 * value; the initial one is the single launch). */
#define WQ_HEAVY_FANOUT 16.0
/* A negative or NaN hint hands the choice back to the automatic rule (host-array ticks of >= 256
 * messages set the next tick's shape from their own n_pairs / M). */
int wq_set_fanout_hint(wq_router* h, double pairs_per_message);

/* ---- F1: GlobalMessage to a named world (worldql_server/src/processing/global_message.rs:36-84)
 * Message m goes to every peer subscribed to at least one cube of world[m]
 * (AreaMap::get_subscribed_any_peers, area_map.rs:65-67), in ascending peer order, filtered by
 * repl[m] like LocalMessage: ExceptSelf drops sender[m], OnlySelf keeps only sender[m] (if it is
 * subscribed in that world), IncludingSelf keeps every peer. A world with no subscriptions yields
 * nothing (global_message.rs:50-54). Output, capacity and counters as wq_route_tick. The host-array
 * form rejects WQ_WORLD_INVALID (WQ_E_INVALID); the device form routes it to nobody. The "@global"
 * broadcast to every connected peer (global_message.rs:18-35) is a peer-map operation and has no
 * table entry point. */
int wq_route_global(wq_router* h, const uint32_t* world, const uint32_t* sender, const uint8_t* repl,
                    size_t n_msgs, uint32_t* offsets, uint32_t* peers, uint32_t* msgs, size_t capacity,
                    size_t* n_pairs);
int wq_route_global_device(wq_router* h, const uint32_t* d_world, const uint32_t* d_sender,
                           const uint8_t* d_repl, size_t n_msgs, uint32_t* d_offsets, uint32_t* d_peers,
                           uint32_t* d_msgs, size_t capacity, wq_route_counters* d_counters);

/* ---- queries (the reference uses these in its unit tests, area_map.rs:33-67) ---- */
/* AreaMap::is_peer_subscribed(uuid, cube), batched; key_or_pos is n x 3 (int64 if key_is_raw). */
int wq_is_subscribed(wq_router* h, size_t n, const uint32_t* world, const uint32_t* peer,
                     int key_is_raw, const void* key_or_pos, uint8_t* out);
/* AreaMap::is_peer_subscribed_any(uuid), batched. */
int wq_is_subscribed_any(wq_router* h, size_t n, const uint32_t* world, const uint32_t* peer,
                         uint8_t* out);
/* AreaMap::get_subscribed_any_peers() for one world (ascending ids). */
int wq_world_peers(wq_router* h, uint32_t world, uint32_t* out, size_t capacity, size_t* n_out);

/* ---- kernel (1) alone: CubeArea::coord_clamp over n coordinates (cube_area.rs:23-44) ---- */
int wq_quantize(const double* coords, size_t n, uint16_t cube_size, int64_t* out);
int wq_quantize_device(wq_router* h, const double* d_coords, size_t n, int64_t* d_out);

/* ---- multi-GPU: cube-hash ownership ----
 * The reference is single-process (one WorldMap owned by one task, thread.rs:113-148); these
 * entry points partition that one table over G GPUs without changing any result. Each (world,
 * cube) bucket has one owner shard in [0, G) computed from the QUANTISED key, so the owner
 * holds every subscription a message to that cube can reach. A sharded tick is
 *   wq_shard_messages_device -> all-to-all of the records (RCCL) -> wq_route_records_device on
 *   the owner -> all-to-all of per-message counts and peers back to the ingesting GPU.
 * These are the building blocks; the whole tick behind one call is wq_sharded_route_tick_device
 * (below), over RCCL, the in-process hub, or the caller's transport (wq_shard_attach_exchange;
 * tests/test_distributed.py and tests/test_gpu_sharded_native.py drive it over gloo). */
#define WQ_MAX_SHARDS 64
#define WQ_SHARD_ALL 0xFFFFFFFFu /* owner of a REMOVE_PEER op: every shard */

/* One message on the wire between GPUs (40 bytes): its quantised CubeArea (or, with flags &
 * WQ_REC_POS, the bits of its f64 position — what the owner's radius filter needs), world,
 * sender, index in the ingesting GPU's batch, and replication code. */
typedef struct wq_msg_rec {
    int64_t key[3];
    uint32_t world;
    uint32_t sender;
    uint32_t msg;
    uint8_t repl;
    uint8_t flags;
    uint8_t pad_[2];
} wq_msg_rec;
#define WQ_REC_POS 1u /* key[] holds the message position (double[3] bits); the owner quantises */

/* Owner shard of each op (host arrays); REMOVE_PEER ops get WQ_SHARD_ALL. Each shard applies,
 * in array order, the ops it owns plus every REMOVE_PEER (area_subscribe.rs / area_unsubscribe.rs
 * / thread.rs:124-125 on the owner). */
int wq_shard_ops(wq_router* h, const wq_op* ops, size_t n, uint32_t n_shards, uint32_t* owner);
/* Quantise (or take raw keys), compute owners and write the records grouped by owner, stable in
 * message order: d_out[M] and d_counts[n_shards] (device). Asynchronous on the handle's stream.
 * With the radius filter on (wq_set_radius) and positions given, the records carry the positions
 * (WQ_REC_POS) so the owner can filter; every shard then needs the peer positions. */
int wq_shard_messages_device(wq_router* h, const double* d_pos, const int64_t* d_keys,
                             const uint32_t* d_world, const uint32_t* d_sender, const uint8_t* d_repl,
                             size_t n_msgs, uint32_t n_shards, wq_msg_rec* d_out, uint32_t* d_counts);
/* wq_route_tick_device on received records (the owner side of a sharded tick). With the radius
 * filter on, records without WQ_REC_POS have no position and route to nobody. */
int wq_route_records_device(wq_router* h, const wq_msg_rec* d_recs, size_t n_msgs, uint32_t* d_offsets,
                            uint32_t* d_peers, uint32_t* d_msgs, size_t capacity,
                            wq_route_counters* d_counters);

/* ---- multi-GPU: sharded ticks behind the ABI ----
 * A handle becomes shard `rank` of G by attaching an exchange; afterwards
 *   wq_sharded_apply_ops            every shard is given the SAME op stream (the reference's one
 *                                   subscription task, thread.rs:122-146) and keeps the ops of the
 *                                   buckets it owns plus every REMOVE_PEER;
 *   wq_sharded_route_tick_device    every shard is given its OWN ingested messages; the call runs
 *                                   shard -> exchange -> route on the owners -> exchange back and
 *                                   returns, on each shard, exactly the CSR wq_route_tick_device would
 *                                   return for those messages on one GPU holding the whole table
 *                                   (offsets[M+1] and peers[P] in message order, msgs[P] optional).
 * The tick is collective: all G shards call it (M may be 0), each on its own thread or process.
 * Its exchanges are sized by budgets every shard derives from the previous tick's sizes (both ends
 * of a pair agree without a read-back), so it reads the device once, at its end, and is synchronous
 * on return; *n_pairs = P. The first tick, and a tick whose sizes outgrew a budget (every shard
 * learns it from the exchanged status words and all redo the tick), read the sizes back first. If
 * P > capacity the tick still completes (its peers are not left waiting), returns WQ_E_CAPACITY
 * with offsets written, and wq_sharded_copy_out re-copies the kept result into a larger buffer
 * without another exchange — as long as the table is unchanged since (WQ_E_INVALID otherwise).
 * Exchange failures return WQ_E_RCCL.
 * Exchanges: RCCL (one process per GPU, or several handles of one process), an in-process hub
 * (G handles of one process, peer copies over xGMI), or the caller's own all-to-all. */
#define WQ_RCCL_ID_BYTES 128
/* The caller's all-to-all: send_bytes[d] bytes to shard d from d_send (segments contiguous in
 * shard order), recv_bytes[s] bytes from shard s into d_recv (likewise); device pointers, ordered
 * after the work already queued on hip_stream. Returns 0 on success. */
typedef int (*wq_exchange_fn)(void* ctx, const void* d_send, const size_t* send_bytes, void* d_recv,
                              const size_t* recv_bytes, void* hip_stream);
typedef struct wq_hub wq_hub;
int wq_hub_create(uint32_t n_shards, wq_hub** out);
int wq_hub_destroy(wq_hub* hub);
int wq_shard_attach_hub(wq_router* h, wq_hub* hub, uint32_t rank);
/* RCCL: rank 0 makes the id (wq_rccl_unique_id), the caller distributes the 128 bytes, every rank
 * attaches (collective, blocks until all G have joined). librccl is loaded at run time. */
int wq_rccl_unique_id(uint8_t* id_out);
int wq_shard_attach_rccl(wq_router* h, uint32_t n_shards, uint32_t rank, const uint8_t* id);
int wq_shard_attach_exchange(wq_router* h, uint32_t n_shards, uint32_t rank, wq_exchange_fn fn, void* ctx);
int wq_shard_detach(wq_router* h);
int wq_shard_info(wq_router* h, uint32_t* n_shards, uint32_t* rank);
int wq_sharded_apply_ops(wq_router* h, const wq_op* ops, size_t n);
int wq_sharded_route_tick_device(wq_router* h, const double* d_pos, const int64_t* d_keys,
                                 const uint32_t* d_world, const uint32_t* d_sender, const uint8_t* d_repl,
                                 size_t n_msgs, uint32_t* d_offsets, uint32_t* d_peers, uint32_t* d_msgs,
                                 size_t capacity, size_t* n_pairs);
int wq_sharded_copy_out(wq_router* h, uint32_t* d_offsets, uint32_t* d_peers, uint32_t* d_msgs, size_t capacity);
/* The same tick without its end-of-tick read: it returns as soon as its work is enqueued (the GPU
 * never idles between back-to-back ticks) and writes its result to d_counters (device memory,
 * nullable) and the sticky wq_route_health words, as wq_route_tick_device does: n_pairs = P,
 * overflow = P > capacity (outputs truncated), error = the device bits of every shard's counters
 * and statuses (2, 4, 8 as for a single-GPU tick), 32 when some shard's local step failed, 64 when a
 * budget was too small — the tick's outputs are then NOT valid and the caller routes it again; every
 * shard sees the same bits. The budgets of a tick come from the tick two calls back: each call first
 * folds in the read-back of every earlier asynchronous tick but the latest (all shards fold the same
 * ticks, so both ends of every pair agree). A tick that must run exact (the first, or after a bit
 * 64) runs synchronously, as wq_sharded_route_tick_device does. A shard whose local step fails on a
 * budgeted tick still ends it asynchronously (its snapshot queued like every other shard's, so all
 * shards keep folding the same ticks) and returns its error code; the others see bit 32. Collective:
 * all G shards make the same sequence of sharded calls. wq_sharded_copy_out does not apply to an
 * asynchronous tick. The slot form only (not wq_debug_set_shard_form's expanded form). A result that
 * never arrives (60 s) returns WQ_E_TIMEOUT naming the tick, its ring slot and the sequence words. */
int wq_sharded_route_tick_async(wq_router* h, const double* d_pos, const int64_t* d_keys,
                                const uint32_t* d_world, const uint32_t* d_sender, const uint8_t* d_repl,
                                size_t n_msgs, uint32_t* d_offsets, uint32_t* d_peers, uint32_t* d_msgs,
                                size_t capacity, wq_route_counters* d_counters);
/* What crosses between GPUs in a sharded tick: each message as one 20-byte slot to its owner (two
 * for a key without a packed form), and back a 12-byte row reference per slot plus, per (owner,
 * ingesting shard), ONE copy of every cube list those messages hit — not the expanded (message,
 * peer) pairs (C3: a hotspot list of ~500 peers is hit by thousands of messages a tick). The
 * ingesting GPU expands the rows itself; with the radius filter on it also filters them there, where
 * the message positions are (every shard holds every peer position), so a hot cube costs its owner
 * one list copy per ingesting shard, however many messages hit it.
 * wq_shard_last_bytes: bytes this shard sent to / received from OTHER shards in its latest sharded
 * tick (the xGMI volume; the self segment is not counted). */
int wq_shard_last_bytes(wq_router* h, uint64_t* sent, uint64_t* received);
/* Slot ticks run exactly (the sizes read back twice: the first tick, or a redo after a tick outgrew
 * its budgets) and on budgets (one host read per tick, at its end), on this shard so far. */
int wq_shard_tick_stats(wq_router* h, uint64_t* exact, uint64_t* budgeted);
/* Test / tuning hook: 1 = the sharded tick sends 40-byte records and returns expanded pairs (the
 * earlier form; the owner filters by radius), 0 = slots, row references and pools (default).
 * Results are identical. */
int wq_debug_set_shard_form(wq_router* h, int expanded);
/* Test hook: the next sharded tick on this handle fails locally at step 1 (grouping its messages)
 * or 3 (routing what it owns) with WQ_E_INVALID, as a real local failure would: it still completes
 * every exchange of the tick, and every shard of the tick returns an error. 0 = off. */
int wq_debug_inject_shard_failure(wq_router* h, int step);

/* The owner-side form of the sharded tick ("pairs stay on the owner"):
 * the same collective shard -> exchange -> route, but the (message, peer) pairs are not sent back.
 * On return, *out describes what THIS shard routed — the R messages it owns, as the records it
 * received (recs[i].msg = the message's index in its ingesting shard's batch; records from source
 * shard s are recs[seg[s] .. seg[s+1])) with their recipients as a CSR (offsets[R + 1], peers[P]),
 * each message's peers ascending. Device pointers into the handle's workspace, valid until the
 * next sharded call on it. A transport that sends from the owner (or re-partitions by peer) needs
 * no return exchange: across the shards every message appears exactly once. */
typedef struct wq_owner_view {
    const wq_msg_rec* recs;
    const uint32_t* offsets;
    const uint32_t* peers;
    uint64_t n_recs;
    uint64_t n_pairs;
    uint32_t seg[WQ_MAX_SHARDS + 1];
} wq_owner_view;
int wq_sharded_route_owner_device(wq_router* h, const double* d_pos, const int64_t* d_keys,
                                  const uint32_t* d_world, const uint32_t* d_sender, const uint8_t* d_repl,
                                  size_t n_msgs, wq_owner_view* out);

/* The owner form on budgeted 20-byte slots (first option; the per-slot
 * lookup is area_map.rs:52-60 / local_message.rs:52-86): every message goes to the shard owning its
 * cube as one slot (two for a key without a packed form), this shard's own messages through the
 * self segment. The slot exchange is the tick's only collective step. Each owner routes the slots it
 * received and keeps the pairs. The exchange sizes are budgets from the previous tick (the first
 * tick, or one after a short budget anywhere, runs exact), so only the end of the tick reads back.
 * Collective: every shard calls it. Received segment of source s: slots [seg[s], seg[s+1]), in
 * the order of s's sent segment for this shard, [send_seg[me], send_seg[me+1]) on s. So slot
 * seg[s] + k carries the message send_perm[send_seg[me] + k] of shard s (UINT32_MAX: padding, or
 * the second slot of a wide key). Padding and second slots route to nobody. The pairs are a CSR
 * over the received slots: slot i's recipients are peers[offsets[i] .. offsets[i+1]). Device
 * pointers into the handle's workspace stay valid until the next sharded call. No radius filter
 * here (wq_sharded_route_owner_device has it). */
#define WQ_SLOT_WORDS 5
typedef struct wq_owner_slot_view {
    const uint32_t* slots;      /* n_slots x WQ_SLOT_WORDS words, as received */
    const uint32_t* offsets;    /* [n_slots + 1] */
    const uint32_t* peers;      /* [n_pairs] */
    const uint32_t* send_perm;  /* this shard's sent slots -> its message index */
    uint64_t n_slots;
    uint64_t n_pairs;
    uint32_t seg[WQ_MAX_SHARDS + 1];       /* received segments, per source shard */
    uint32_t send_seg[WQ_MAX_SHARDS + 1];  /* sent segments, per owner shard */
} wq_owner_slot_view;
int wq_sharded_route_owner_slots(wq_router* h, const double* d_pos, const int64_t* d_keys,
                                 const uint32_t* d_world, const uint32_t* d_sender, const uint8_t* d_repl,
                                 size_t n_msgs, wq_owner_slot_view* out);
/* The same without the end-of-tick read (as wq_sharded_route_tick_async): a budgeted tick returns
 * once enqueued, with out->n_pairs = UINT64_MAX; P and the status bits land in d_counters (device;
 * nullable) and the sticky health words (error bit 64: a budget was too small, the tick's outputs
 * are not valid and the next call runs exact; overflow: the handle's pair buffer was short, the
 * outputs are truncated and the buffer grows for the tick after next). A tick that must run exact
 * (the first, one after a short budget, one after the slot tick) runs synchronously and fills
 * n_pairs. A local failure on a budgeted tick ends it asynchronously all the same and returns the
 * error. The view's arrays are rewritten by the next tick on the handle's stream. */
int wq_sharded_route_owner_slots_async(wq_router* h, const double* d_pos, const int64_t* d_keys,
                                       const uint32_t* d_world, const uint32_t* d_sender, const uint8_t* d_repl,
                                       size_t n_msgs, wq_route_counters* d_counters, wq_owner_slot_view* out);

/* ---- F2: per-peer send lists (PeerMap::broadcast_to, worldql_server/src/transport/peer_map.rs:151-163)
 * The transpose of a tick's message-major CSR for a transport that batches per peer: for every
 * peer p < n_peers whose bit is set in d_connected (bit p % 32 of word p / 32; NULL = every peer
 * connected) the messages it must receive, ascending — the reference's "recipients intersected
 * with the connected peers". d_peer_offsets[n_peers + 1]; d_msgs_out[n_pairs] (the kept ones
 * first: d_peer_offsets[n_peers] of them). Asynchronous: nothing is read back, so the call can
 * follow wq_route_tick_device on the same stream without the host knowing the tick's pair count.
 *
 * Inputs
 *   - n_pairs is the element count of d_peers and d_msgs_out, i.e. the `capacity` the tick was
 *     given. It need not equal d_offsets[n_msgs]: a cut tick's offsets reach past it, a buffer
 *     larger than the tick's pairs ends behind them.
 *   - Row m is the part of [offsets[m], offsets[m + 1]) inside [0, n_pairs). It is empty when
 *     offsets[m + 1] < offsets[m]. Elements of [0, n_pairs) that no row covers belong to nobody
 *     and are dropped, whatever they hold.
 *   - No input is dereferenced outside [0, n_pairs), [0, n_msgs] or the ceil(n_peers / 32) bitmap
 *     words, whatever the arrays hold. d_offsets is not read at all with n_msgs == 0.
 * Outputs
 *   - Nothing is written outside d_peer_offsets[0 .. n_peers] and d_msgs_out[0 .. n_pairs).
 *   - For ascending offsets the result is exactly the transpose of the clamped rows: a peer's
 *     messages ascend, and a peer repeated within a row keeps its repeats. A tick always writes
 *     ascending offsets, cut or not, below the 2^32-pair limit.
 *   - For other offsets (wrapped, descending, junk) the result is unspecified but well formed:
 *     d_peer_offsets ascends from 0, d_peer_offsets[n_peers] <= n_pairs, every written message
 *     index is < n_msgs, and two calls on the same input give the same bytes.
 *   - d_msgs_out[d_peer_offsets[n_peers] .. n_pairs) is scratch: it holds the rows of the dropped
 *     elements, 0 for an element no row covers.
 *   - d_peer_offsets is always written in full, including n_msgs == 0, n_pairs == 0 and
 *     n_peers == 0.
 * Scratch lives in the handle, grow-only (12 n_pairs bytes and the sort's): a steady-state call
 * does no hipMalloc. */
int wq_peer_major_device(wq_router* h, const uint32_t* d_offsets, const uint32_t* d_peers, size_t n_msgs,
                         size_t n_pairs, const uint32_t* d_connected, uint32_t n_peers,
                         uint32_t* d_peer_offsets, uint32_t* d_msgs_out);

/* ---- tick sends: one per-peer frame list from all of a tick's read runs ----
 * A received tick is routed run by run (wq_ingest_dispatch_device): every read run leaves a CSR region
 * for its LocalMessage rows, one for its GlobalMessage rows, or both, and row k of a region is frame
 * l_src[l_begin + k] or g_src[g_begin + k] of the tick. wq_peer_major_device transposes one CSR and
 * names rows; this call transposes all regions of a tick at once and names frames: for every peer the
 * received frames it must be sent, ascending by frame index — the order in which the reference's
 * sequential loop (PeerMap::broadcast_to per message, in arrival order) would have sent them, whatever
 * run or kind a frame came from. Its output is what wq_peer_budget*_device, wq_peer_rotate_device and
 * wq_peer_pack_device take, with the tick's received frames as the frames.
 *
 * Regions (a HOST array, validated and copied before the call returns)
 *   - The element space is the regions' [0, capacity) laid end to end in region order; n_elems is its
 *     length, the sum of the capacities. Region g's elements are d_peers[peers_at .. peers_at + capacity).
 *   - Inside a region a row and its clamping are wq_peer_major_device's with n_pairs = capacity, on the
 *     region's own n_rows + 1 offsets d_offsets[off_at ..] (region-local, as a route call writes them).
 *     off_at == WQ_SEND_UNIT_ROWS: row r is element r, for r < min(n_rows, capacity), and d_offsets is
 *     not read. An element no row covers belongs to nobody. d_offsets is not read for n_rows == 0.
 *   - The frame of an element of row r is frame_base + (src_at == WQ_SEND_NO_SRC ? r :
 *     d_src[src_sel][src_at + r]), computed in 64 bits. Nothing assumes that the src entries ascend, and
 *     the same frame in two rows or two regions is no error: the element is kept twice.
 *   - A region with n_rows == 0 or capacity == 0 is legal and empty.
 * Drops and errors (wq_tick_sends_counters.error)
 *   - An element whose frame is >= n_frames is dropped and counted in n_drop_frame; error bit 1.
 *   - Of the others, an element whose peer is >= n_peers or not set in d_connected (as
 *     wq_peer_major_device; NULL = every peer connected) is dropped and counted in n_drop_peer.
 *   - A cut route call is a legal input: its offsets reach past `capacity`. It sets error bit 0, and so do
 *     descending offsets; for those the result is well formed but unspecified, as in wq_peer_major_device.
 *   - n_covered = n_kept + n_drop_peer + n_drop_frame: the elements a row covers.
 * Outputs
 *   - d_frames_out[d_peer_offsets[p] .. d_peer_offsets[p + 1]) holds peer p's frames ascending by frame
 *     index, equal frames in element order. d_peer_offsets[n_peers + 1] is always written in full.
 *   - All n_elems words of d_frames_out are written on every call: the d_peer_offsets[n_peers] kept ones,
 *     then zeros. Nothing is written outside the two arrays and the counters, and two calls on the same
 *     input give the same bytes.
 * Execution
 *   - Asynchronous on the handle's stream; nothing is read back. Scratch lives in the handle, grow-only
 *     (8 or 12 bytes per element, the sort's, 44 bytes per region): a steady-state call does no hipMalloc.
 *     The regions go through a pinned buffer of the handle's; the call waits for the previous call's copy
 *     out of that buffer, not for the stream. `regions` is free to reuse when the call returns.
 *   - Like wq_peer_major_device the call needs only a stream and scratch: a multi-GPU handle runs it on
 *     its own stream with the arrays on devices[0].
 * WQ_E_INVALID, with nothing launched and a wq_last_error text: a null handle, `in` or d_peer_offsets; a
 * null array with a non-zero size; n_peers == 2^32 - 1; the sum of the capacities differs from n_elems or
 * exceeds 2^32 - 1; a region with pad_ != 0 or src_sel > 1; a region that reaches outside d_offsets
 * (n_rows > 0), d_peers or its src array (n_rows > 0).
 * Not covered: `@global` broadcasts (WQ_CLS_BCAST). PeerMap::broadcast_all reaches peers that never
 * subscribed and hold no id: that is the transport's operation. Heartbeat echoes and record replies are
 * expressible as unit-row regions with a frame_base behind the received frames; building their frames
 * into one index space is the caller's. */
#define WQ_SEND_UNIT_ROWS 0xFFFFFFFFu /* wq_send_region.off_at */
#define WQ_SEND_NO_SRC    0xFFFFFFFFu /* wq_send_region.src_at */
typedef struct wq_send_region {   /* HOST array, 32 bytes each */
    uint32_t off_at;      /* first of n_rows + 1 entries in d_offsets, or WQ_SEND_UNIT_ROWS */
    uint32_t peers_at;    /* the region's first element in d_peers */
    uint32_t n_rows;
    uint32_t capacity;    /* the region's elements in d_peers: what the route call was given */
    uint32_t src_at;      /* first of n_rows entries in d_src[src_sel], or WQ_SEND_NO_SRC: row r is frame r */
    uint32_t frame_base;  /* added to the frame index (several frame arrays behind one another in one index space) */
    uint32_t src_sel;     /* 0 or 1 */
    uint32_t pad_;        /* 0 */
} wq_send_region;

typedef struct wq_tick_sends_in {
    const wq_send_region* regions;           /* HOST, [n_regions] */
    const uint32_t* d_offsets; size_t n_offsets;
    const uint32_t* d_peers;   size_t n_pairs;
    const uint32_t* d_src[2];  size_t n_src[2];   /* l_src and g_src of the dispatch, or NULL */
    const uint32_t* d_connected;             /* nullable, as wq_peer_major_device */
    uint32_t n_regions, n_peers, n_frames, pad_;  /* n_frames: size of the frame index space */
} wq_tick_sends_in;

typedef struct wq_tick_sends_counters {      /* 64 bytes */
    uint64_t n_regions, n_elems, n_covered, n_kept, n_drop_peer, n_drop_frame;
    uint32_t error, pad_; uint64_t reserved_;
} wq_tick_sends_counters;

int wq_tick_sends_device(wq_router* h, const wq_tick_sends_in* in,
                         uint32_t* d_peer_offsets /* [n_peers + 1] */,
                         uint32_t* d_frames_out   /* [n_elems] */, size_t n_elems /* sum of capacity */,
                         wq_tick_sends_counters* d_counters /* nullable */);

/* ---- interest changes: who entered and who left each row between two ticks ----
 * A server that replicates entities (row m of every tick = entity m) sends a spawn to the
 * observers that entered an entity's interest set since the last tick and a despawn to those that
 * left. An extension like follow and the radius filter: the reference stores neither positions nor
 * earlier results (local_message.rs:52-86 routes and forgets).
 *
 * Inputs
 *   - Both inputs are CSRs over the same n_rows rows: offsets[n_rows + 1] from 0, peers ascending
 *     and distinct within a row — what wq_route_tick* and wq_route_global* write.
 *   - Row identity across the two ticks is the caller's business: row m is the same entity in both.
 *   - old_capacity and new_capacity are the element counts of the two peers arrays, the `capacity`
 *     the ticks were given.
 *   - The kernels clamp every row bound to them: row m is the part of [offsets[m], offsets[m + 1])
 *     inside [0, capacity), empty when offsets[m + 1] < offsets[m].
 *   - A truncated tick (one whose own `overflow` was set) can never make the diff read outside an
 *     array. Its rows then compare only what was written, and `error` bit 0 is set.
 *   - No input is ever dereferenced outside [0, capacity) or [0, n_rows], whatever it holds.
 *   - Offsets that descend in several places can make the clamped rows overlap; a side's rows are
 *     walked up to 2 x capacity elements in total (one descending pair never reaches that), the
 *     rows past it are taken as empty.
 * Outputs
 *   - Row m of the entered CSR is new_m \ old_m, row m of the left CSR is old_m \ new_m, both
 *     ascending.
 *   - Both output offset arrays are always written in full, [n_rows + 1] from 0, even on overflow.
 *   - Pairs at index >= capacity are not written, as wq_route_tick_device does.
 *   - The left side is optional: with d_left_offsets == NULL, d_left_peers must also be NULL and
 *     left_capacity 0. The left set is then neither computed nor counted: n_left = 0 and overflow
 *     bit 1 is never set.
 *   - d_counters is nullable.
 *   - Output is deterministic, byte for byte: placement comes from prefix sums, never from atomic
 *     arrival order.
 * Execution
 *   - wq_csr_diff_device is asynchronous on the handle's stream and reads nothing back. The grids
 *     are sized from n_rows and the capacities; the pair totals are read on the device.
 *   - Scratch lives in the handle, grow-only: at most 16 (n_rows + 1) + 3 (new_capacity +
 *     old_capacity) / 4 bytes. A steady-state call does no hipMalloc, no memset and no memcpy launch.
 *   - wq_csr_diff uploads, runs and downloads. It returns WQ_E_CAPACITY with *n_entered and
 *     *n_left set when an output is too small; it then copies the offsets and no pairs. n_left may
 *     be NULL when the left side is off.
 * Limits and handle kinds
 *   - n_rows < 2^32 - 1024 and capacities <= 2^32 - 1 (larger ones count as that), the route's
 *     limits. n_rows == 0 is valid and writes the two offsets[0] = 0.
 *   - WQ_E_INVALID for a null handle, a null required array with a non-zero size, or a half-given
 *     left side; nothing is launched then.
 *   - As wq_peer_major_device the call needs only a stream and scratch: a multi-GPU handle runs it
 *     on the handle's own stream with the arrays on devices[0]. The sharded views have no form of
 *     their own. */
typedef struct wq_diff_counters {
    uint64_t n_entered;  /* sum over rows of |new \ old| */
    uint64_t n_left;     /* sum over rows of |old \ new| */
    uint32_t overflow;   /* bit 0: n_entered > ent_capacity, bit 1: n_left > left_capacity */
    uint32_t error;      /* bit 0: some row had offsets[m+1] < offsets[m] or reached past its
                            array's capacity; such a row is taken as the part inside bounds */
} wq_diff_counters;
int wq_csr_diff_device(wq_router* h, size_t n_rows,
                       const uint32_t* d_old_offsets, const uint32_t* d_old_peers, size_t old_capacity,
                       const uint32_t* d_new_offsets, const uint32_t* d_new_peers, size_t new_capacity,
                       uint32_t* d_ent_offsets, uint32_t* d_ent_peers, size_t ent_capacity,
                       uint32_t* d_left_offsets, uint32_t* d_left_peers, size_t left_capacity,
                       wq_diff_counters* d_counters);
int wq_csr_diff(wq_router* h, size_t n_rows,
                const uint32_t* old_offsets, const uint32_t* old_peers, size_t old_capacity,
                const uint32_t* new_offsets, const uint32_t* new_peers, size_t new_capacity,
                uint32_t* ent_offsets, uint32_t* ent_peers, size_t ent_capacity,
                uint32_t* left_offsets, uint32_t* left_peers, size_t left_capacity,
                size_t* n_entered, size_t* n_left);

/* ---- send budgets: of every peer's send list the B nearest messages ----
 * wq_peer_major_device gives every observer all it could be told this tick; a connection has a
 * budget. This call keeps, per peer, the min(B, len) messages nearest to the peer and leaves the
 * rest for a later tick. An extension like the radius filter, follow and the interest diff: the
 * reference routes and forgets (local_message.rs:52-86, peer_map.rs:151-163) and has no budget.
 *
 * Input rows
 *   - d_peer_offsets[n_peers + 1] and d_msgs[n_in] are a peer-major CSR, what wq_peer_major_device
 *     writes. n_in is the element count of d_msgs and of d_out_msgs.
 *   - Row p is the part of [d_peer_offsets[p], d_peer_offsets[p + 1]) inside [0, n_in), empty when
 *     the offsets descend.
 *   - d_msg_pos[3 n_msgs] are the tick's message positions. d_peer_pos[3 n_peer_pos] are the peers'
 *     positions; NULL (with n_peer_pos 0): the handle's wq_set_peer_positions[_device]. A non-NULL
 *     d_peer_pos with n_peer_pos 0 is an explicit "no peer has a position" and is not read.
 *   - No input is dereferenced outside [0, n_in), [0, n_peers], [0, 3 n_msgs), [0, 3 n_peer_pos) or
 *     d_budget[0 .. n_peers), whatever the arrays hold.
 *   - Offsets that descend can make the clamped rows overlap. The rows are walked up to n_in
 *     elements in total: the row that passes it is cut there and the rows behind it are empty.
 *     Ascending offsets never reach that. `error` bit 0 is set, and the result is the contract
 *     below applied to those rows.
 * Key of element j of row p, with message index m = d_msgs[j]
 *   - dx = mx - px; dy = my - py; dz = mz - pz; d2 = (dx*dx + dy*dy) + dz*dz, in f64, left to right,
 *     no FMA contraction: the radius filter's expression ("C5: exact radius filter" above).
 *   - d2 counts as +infinity when it is NaN, when m >= n_msgs (this also sets `error` bit 1) or when
 *     p >= n_peer_pos; such an element never reads a position it does not have.
 *   - Elements order by (d2, position in the input row): a total order. Co-located entities have
 *     equal d2, and a row may hold a message twice.
 * Output
 *   - Row p of the output holds the min(B_p, len_p) smallest elements of row p, B_p = d_budget[p],
 *     or k when d_budget is NULL, in input order (a stable compaction: ascending messages stay
 *     ascending). B_p == 0 empties the row; B_p >= len_p copies it.
 *   - d_out_offsets[0 .. n_peers] is always written in full, from 0, including n_in == 0 and
 *     n_peers == 0.
 *   - Nothing is written outside d_out_offsets[0 .. n_peers] and d_out_msgs[0 .. n_kept); n_kept <=
 *     n_in, so the output never overflows. The output must not alias the input.
 *   - d_counters is nullable.
 *   - Output is deterministic, byte for byte: placement comes from counts and prefix sums, never
 *     from atomic arrival order (the atomics are integer adds into histograms).
 * Execution
 *   - Asynchronous on the handle's stream; nothing is read back. The grids are sized from n_in and
 *     n_peers. No lane, wave or block walks a row: a row longer than 256 elements is selected by a
 *     radix select whose histograms all its elements build, a shorter one is ranked by counting.
 *   - Scratch lives in the handle, grow-only: at most 18 n_in + 12 (n_peers + 1) bytes plus the
 *     scans' (each buffer is allocated a quarter above its need). A steady-state call does no
 *     hipMalloc.
 * Limits and handle kinds
 *   - n_in <= 2^32 - 1 and n_peers < 2^32 - 1; n_msgs and n_peer_pos above 2^32 - 1 count as that.
 *   - WQ_E_INVALID for a null handle, a null required array with a non-zero size (d_out_offsets is
 *     always required), d_peer_pos == NULL when the handle has no positions, and d_peer_pos == NULL
 *     on a multi-GPU handle, whose positions live in its sub-handles. Nothing is launched then.
 *   - With explicit positions a multi-GPU handle runs the call on its own stream with the arrays on
 *     devices[0], as wq_peer_major_device does. */
typedef struct wq_budget_counters {
    uint64_t n_in;       /* elements inside the clamped input rows */
    uint64_t n_kept;     /* elements written = out_offsets[n_peers] */
    uint32_t rows_cut;   /* rows longer than their budget */
    uint32_t error;      /* bit 0: an input row had off[p+1] < off[p] or reached past n_in;
                            bit 1: some element's message index was >= n_msgs */
} wq_budget_counters;
int wq_peer_budget_device(wq_router* h,
        const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers, size_t n_in,
        const double* d_msg_pos, size_t n_msgs,
        const double* d_peer_pos, size_t n_peer_pos,
        uint32_t k, const uint32_t* d_budget,
        uint32_t* d_out_offsets, uint32_t* d_out_msgs,
        wq_budget_counters* d_counters);

/* ---- byte budgets: of every peer's send list the nearest messages that fit in W bytes ----
 * A connection's budget is bytes per tick, and frames differ in size by orders of magnitude
 * (wq_serialize_messages returns every frame's size as offsets[i + 1] - offsets[i]). This call keeps,
 * per peer, the longest prefix of its list in nearest-first order whose sizes sum to at most W_p.
 *
 * Inputs
 *   - Rows, their clamping, overlapping rows and `error` bit 0 are as in wq_peer_budget_device: row p
 *     is the part of [d_peer_offsets[p], d_peer_offsets[p + 1]) inside [0, n_in), and the rows are
 *     walked up to n_in elements in total.
 *   - Keys are as in wq_peer_budget_device: d2 = (dx*dx + dy*dy) + dz*dz in f64, no contraction;
 *     +infinity for NaN, for m >= n_msgs (`error` bit 1) and for a peer without a position. Elements
 *     order by (d2, position in the input row). Positions are resolved in the same way: the handle's
 *     when d_peer_pos is NULL.
 *   - The size of element j is d_msg_size[d_msgs[j]], a u32; it is 0, and nothing is read, when
 *     d_msgs[j] >= n_msgs. d_msg_size[n_msgs] is required when n_msgs > 0 and never read outside
 *     [0, n_msgs).
 *   - W_p = d_budget_bytes[p] (u64 per peer), or w when d_budget_bytes is NULL.
 * Output
 *   - An element of row p is kept iff the sum of the sizes of all elements of row p at or before it in
 *     the (d2, position) order, its own included, is <= W_p. The sum is taken in u64; a row has fewer
 *     than 2^32 elements of less than 2^32 bytes each, so neither a row's total nor the call's wraps.
 *   - So the kept set is a prefix of that order. W_p == 0 keeps exactly the leading zero-size
 *     elements. If the nearest message alone exceeds W_p nothing behind it is kept either (zero-size
 *     elements before it are): priority is strict, a far small message never overtakes a near large
 *     one. A caller who must always send the head sets W_p at least to its largest frame. A row whose
 *     total is <= W_p is copied.
 *   - The output keeps input order (a stable compaction) and is deterministic byte for byte; nothing
 *     is read back. d_out_offsets[0 .. n_peers] is always written in full, from 0.
 *   - d_out_bytes (nullable): entry p is the kept bytes of row p, what a transport sizes its send
 *     buffers from. d_counters is nullable.
 *   - Nothing is written outside d_out_offsets[0 .. n_peers], d_out_msgs[0 .. n_kept),
 *     d_out_bytes[0 .. n_peers) and the counters. Outputs must not alias inputs.
 * Composition
 *   - wq_peer_budget_device (count B) first and this call on its output keeps exactly the elements
 *     with both "rank < B" and "running bytes <= W": a stable compaction preserves the elements'
 *     relative positions, so the order of the survivors is the order they had, and the first cap keeps
 *     a prefix of it. That is how a caller gets both caps; there is no combined entry point.
 * Execution
 *   - Asynchronous on the handle's stream. As the count budget, with a weighted radix select for rows
 *     longer than 256 elements: its histograms sum sizes in u64 and each pass picks the bin in which
 *     the running byte total first exceeds what is left of W_p. No lane, wave or block walks a row;
 *     placement comes from counts and prefix sums, the atomics are integer adds.
 *   - Scratch lives in the handle, grow-only, released with it: the count budget's buffers, shared
 *     with it, plus at most 20.1 n_in + 2080 bytes of its own (size 4, one u64 scan 8, the select's u64
 *     histograms 8 per element); together at most 38.1 n_in + 12 (n_peers + 1) bytes plus the scans'
 *     (each buffer is allocated a quarter above its need). A steady-state call does no hipMalloc,
 *     and the two budget calls may alternate on one handle.
 * Limits and handle kinds
 *   - As wq_peer_budget_device: n_in <= 2^32 - 1, n_peers < 2^32 - 1; the same WQ_E_INVALID cases
 *     (d_msg_size NULL with n_msgs > 0 among the null arrays), nothing launched then; a multi-GPU
 *     handle needs explicit positions and takes the arrays on devices[0]. */
typedef struct wq_budget_bytes_counters {
    uint64_t n_in;        /* elements inside the clamped input rows */
    uint64_t n_kept;      /* elements written = out_offsets[n_peers] */
    uint64_t bytes_in;    /* sum of the sizes of those n_in elements */
    uint64_t bytes_kept;  /* sum of the sizes of the kept ones */
    uint32_t rows_cut;    /* rows that lost at least one element */
    uint32_t error;       /* bits 0 and 1 as in wq_budget_counters */
} wq_budget_bytes_counters;
int wq_peer_budget_bytes_device(wq_router* h,
        const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers, size_t n_in,
        const double* d_msg_pos, const uint32_t* d_msg_size, size_t n_msgs,
        const double* d_peer_pos, size_t n_peer_pos,
        uint64_t w, const uint64_t* d_budget_bytes,
        uint32_t* d_out_offsets, uint32_t* d_out_msgs, uint64_t* d_out_bytes,
        wq_budget_bytes_counters* d_counters);

/* ---- fair share: rotate what the budgets cut so every entity arrives ----
 * Both budgets keep the nearest messages of a peer's list, every tick the same ones while the crowd
 * stands still. This call gives a second, small share of the connection's budget to the elements the
 * budget cut, in turn: per peer one u32 cursor holds a message index, and the cut elements that
 * follow it in cyclic order of message index are added to the budget's output. The lists ascend by
 * message index and, for entity workloads, row m of every tick is entity m, so the cursor is an id
 * that survives lists that change under it. There is no per-pair state. An element that stays in a
 * peer's list and stays cut is sent at least once every ceil(T / R) ticks, T the row's cut elements
 * and R its share. The call takes a budget's output and not its rule, so it composes with either
 * budget or both. An extension like the budgets: the reference has neither.
 *
 * Input rows
 *   - d_peer_offsets[n_peers + 1] / d_msgs[n_in] is the full peer-major CSR, the budget's input.
 *     d_kept_offsets[n_peers + 1] / d_kept_msgs[n_kept_in] is the kept CSR over the same peers, either
 *     budget's output on it.
 *   - Rows, their clamping to their own array, the walk of at most n_in (n_kept_in) elements in total
 *     and `error` bit 0 are wq_peer_budget_device's, for either CSR.
 *   - R_p = d_extra[p] (u32 per peer), or r when d_extra is NULL: the count share.
 *   - d_msg_size[n_msgs] (nullable, then n_msgs is ignored and the share is by count only) gives the
 *     size of an element as in wq_peer_budget_bytes_device: d_msg_size[m], and 0 without a read when
 *     m >= n_msgs (`error` bit 1). V_p = d_extra_bytes[p] (u64 per peer), or v when it is NULL: the
 *     byte share. Without sizes v and d_extra_bytes are ignored.
 *   - d_cursor[n_peers] is read and written in place. 0xFFFFFFFF starts at the row's beginning, which
 *     is what a new peer's cursor holds.
 *   - Nothing is dereferenced outside [0, n_in), [0, n_kept_in), [0, n_peers] of the offsets,
 *     [0, n_peers) of the per-peer arrays and [0, n_msgs) of d_msg_size, whatever the arrays hold.
 * Rule, for rows that ascend
 *   - A value m occurs cf times in full row p and ck times in kept row p. The first min(cf, ck)
 *     occurrences in the full row are kept, the others are cut. A kept element with no partner
 *     (ck > cf, or a value the full row does not hold) is ignored and sets `error` bit 2.
 *   - pos_p is the first index of full row p whose message index is greater than d_cursor[p], the
 *     row's end when there is none. The cut elements are numbered q = 0, 1, ... from pos_p to the
 *     row's end, then from the row's start to pos_p.
 *   - The chosen elements are the longest prefix of that order with q < R_p and, with sizes, a running
 *     size sum (u64, own size included) <= V_p. When R_p >= 1 the element q = 0 is always chosen: one
 *     frame larger than V_p cannot block the rotation, and the overshoot is at most that frame.
 *     R_p == 0 chooses nothing.
 * Output
 *   - Row p of d_out_offsets / d_out_msgs holds the kept and the chosen elements of full row p in the
 *     full row's order (a stable compaction: ascending stays ascending), always a sub-multiset of the
 *     full row. d_out_offsets[0 .. n_peers] is always written in full, from 0.
 *   - d_cursor[p] becomes the message index of the chosen element with the largest q, and is left as
 *     it is when nothing was chosen.
 *   - d_out_bytes (nullable, needs sizes): entry p is the size sum of output row p, at most
 *     W_p + V_p + the largest frame after a byte budget W_p: what the pack's buffer is sized from.
 *   - d_counters is nullable.
 *   - Nothing is written outside d_out_offsets[0 .. n_peers], d_out_msgs[0 .. n_out), n_out <= n_in,
 *     d_out_bytes[0 .. n_peers), d_cursor[0 .. n_peers) and the counters. Outputs must not alias
 *     inputs.
 *   - Rows that do not ascend give an unspecified but well formed result: offsets ascend from 0,
 *     d_out_offsets[n_peers] <= n_in, every written index comes from the full row, nothing is touched
 *     out of bounds, and two calls on the same inputs give the same bytes.
 *   - The output is deterministic byte for byte: placement comes from prefix sums; the atomics are
 *     integer adds and ORs into the counters.
 * Execution
 *   - Asynchronous on the handle's stream; nothing is read back. The grids are sized from n_in and
 *     n_peers. No lane, wave or block walks a row: an element finds its row, its occurrence index and
 *     its value's bounds in the kept row by binary search, a peer finds pos_p by binary search, and
 *     ranks and running bytes are differences of two scans over all elements.
 *   - d_cursor[p] is read before it is written: read by the pass over the peers that precedes every
 *     pass over the elements, and written by the call's last kernel.
 *   - Scratch lives in the handle, grow-only, released with it: the budgets' buffers, shared with
 *     them, of which this call uses at most 16.5 n_in + 40 + 12 (n_peers + 1) bytes (per element the
 *     row 4, the size 4 and one u64 scan 8, the last two only with sizes; the flag words), plus
 *     44 (n_peers + 1) + 4096 bytes of its own (the kept CSR's rows 12, the row's folded scan terms 32,
     the slots over which the counters' adds are spread), plus
 *     the scans' (each buffer is allocated a quarter above its need). A steady-state call does no
 *     hipMalloc, and the call may alternate freely with both budget calls and the pack on one handle.
 * Limits and handle kinds
 *   - n_in <= 2^32 - 1, n_kept_in <= 2^32 - 1 and n_peers < 2^32 - 1; n_msgs above 2^32 - 1 counts
 *     as that.
 *   - WQ_E_INVALID, with nothing launched, for a null handle, a null required array with a non-zero
 *     size (d_out_offsets is always required, d_cursor when n_peers > 0), and d_out_bytes without
 *     d_msg_size.
 *   - Positions are not needed: a multi-GPU handle runs the call on its own stream with the arrays on
 *     devices[0], as wq_peer_major_device does. */
typedef struct wq_rotate_counters {
    uint64_t n_in;          /* elements inside the clamped full rows */
    uint64_t n_kept_in;     /* elements of them matched by a kept element */
    uint64_t n_chosen;      /* cut elements chosen */
    uint64_t n_out;         /* elements written = out_offsets[n_peers] = n_kept_in + n_chosen */
    uint64_t bytes_chosen;  /* sum of the sizes of the chosen elements (0 without sizes) */
    uint64_t bytes_out;     /* sum of the sizes of the written ones (0 without sizes) */
    uint32_t rows_rotated;  /* rows with at least one chosen element */
    uint32_t rows_behind;   /* rows that still have cut elements not chosen */
    uint32_t error;         /* bit 0: a row of either CSR descended or reached past its array;
                               bit 1: with sizes, a full element's message index was >= n_msgs;
                               bit 2: a kept element had no partner in its full row */
    uint32_t pad_;
} wq_rotate_counters;       /* 64 bytes */
int wq_peer_rotate_device(wq_router* h,
        const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers, size_t n_in,
        const uint32_t* d_kept_offsets, const uint32_t* d_kept_msgs, size_t n_kept_in,
        const uint32_t* d_msg_size, size_t n_msgs,          /* nullable pair: count share only */
        uint32_t r, const uint32_t* d_extra,
        uint64_t v, const uint64_t* d_extra_bytes,
        uint32_t* d_cursor,                                   /* [n_peers], in place, required */
        uint32_t* d_out_offsets, uint32_t* d_out_msgs, uint64_t* d_out_bytes,
        wq_rotate_counters* d_counters);

/* ---- send buffers: every peer's frames packed into one contiguous byte run ----
 * The budgets leave, per peer, a list of message indices, and wq_serialize_messages leaves the tick's
 * frames in one array (frame i is out[offsets[i] .. offsets[i + 1])). This call does the fan-out on
 * the device: for every peer the frames of its list, in list order, in one byte run that a transport
 * hands to a socket with one write. An extension like the budgets: the reference has no batching
 * transport, its broadcast_to! (transport/peer_map.rs:22-40) clones the bytes and calls send_raw
 * once per recipient.
 *
 * Rows
 *   - d_peer_offsets[n_peers + 1] / d_msgs[n_in] are any peer-major CSR: wq_peer_major_device's,
 *     either budget's, or the transposed output of wq_csr_diff.
 *   - Rows, their clamping to [0, n_in), the walk of at most n_in elements in total and `error` bit 0
 *     are exactly wq_peer_budget_device's.
 *   - Ordinal q is the q-th walked element. For offsets that ascend from 0 without gaps, which is
 *     every CSR this library writes, q equals the index into d_msgs.
 * Frames
 *   - The frame of the element with message m = d_msgs[j] is d_frames[fo[m] .. fo[m + 1]), with
 *     fo = d_frame_offsets[n_msgs + 1].
 *   - The frame is taken as empty (size 0, nothing read from d_frames) when m >= n_msgs (`error` bit 1,
 *     fo is not read), and when fo[m] > fo[m + 1], fo[m + 1] > n_frame_bytes or
 *     fo[m + 1] - fo[m] >= 2^32 (`error` bit 2). Only frames that an element references are looked at.
 *   - A frame is whole or empty, never truncated. d_frames may have any alignment.
 *   - Nothing is dereferenced outside [0, n_in), [0, n_peers], [0, n_msgs] of fo and
 *     [0, n_frame_bytes) of d_frames, whatever the arrays hold.
 * Records and output layout
 *   - The record of an element is the optional 4-byte prefix (flags & WQ_PACK_LEN_PREFIX: the frame's
 *     size as a u32, little endian) followed by the frame. With the prefix on, an empty frame is
 *     still a 4-byte record holding 0.
 *   - E[q] is the exclusive u64 prefix sum of the record sizes over the ordinals. Record q occupies
 *     d_out[E[q] .. E[q] + rec_q).
 *   - Peer p's run is d_out[PB[p] .. PB[p + 1]), PB[p] = E[first ordinal of row p] and
 *     PB[n_peers] = bytes_need. Without the prefix, after wq_peer_budget_bytes_device,
 *     PB[p + 1] - PB[p] is that call's d_out_bytes[p].
 *   - d_out_peer_bytes is PB, always written in full, from 0 and uncut, including n_in == 0 and
 *     n_peers == 0.
 *   - d_out_elem_bytes[q] = E[q] for every walked ordinal (nullable): the record boundaries, for a
 *     transport that sends frame by frame.
 * Capacity
 *   - Bytes at positions >= capacity_bytes are not written, as wq_csr_diff_device does with pairs;
 *     everything below is exact, so a peer with PB[p + 1] <= capacity_bytes has its whole run. A cut
 *     may fall inside a prefix or inside a frame. `overflow` and bytes_need tell the caller to grow.
 *   - d_out == NULL with capacity_bytes == 0 is the sizing call: offsets and counters only.
 * Output guarantees
 *   - Nothing is written outside d_out[0 .. bytes_written), d_out_peer_bytes[0 .. n_peers],
 *     d_out_elem_bytes[0 .. n_in walked) and the counters. Outputs must not alias inputs.
 *   - The output is deterministic byte for byte: placement comes from scans, and the only atomics are
 *     ORs into the error word.
 *   - d_out must be 16-byte aligned (every hipMalloc result is).
 * Execution
 *   - Asynchronous on the handle's stream; nothing is read back. The copy's grid is sized from
 *     capacity_bytes and walks the output bytes: a wave owns 1 KiB of output and a lane 16 bytes, so
 *     no lane, wave or block owns a row or a frame.
 *   - Scratch lives in the handle, grow-only: at most 20 n_in + 8 + 12 (n_peers + 1) bytes (per
 *     ordinal the frame's size 4, its start 8 and E 8; the rows' three words, shared with the
 *     budgets) plus the scans' (each buffer is allocated a quarter above its need). A steady-state
 *     call does no hipMalloc, and the call may alternate freely with both budget calls on one handle.
 * Limits and handle kinds
 *   - WQ_E_INVALID, with nothing launched, for a null handle, a null required array with a non-zero
 *     size (d_out_peer_bytes is always required), d_out == NULL with capacity_bytes > 0, a misaligned
 *     d_out, unknown flag bits, n_in > 2^32 - 1 and n_peers >= 2^32 - 1.
 *   - Like wq_peer_major_device the call needs only a stream and scratch: a multi-GPU handle runs it
 *     on its own stream with the arrays on devices[0].
 *   - Packing into mapped host memory is not covered here and has not been measured. */
#define WQ_PACK_LEN_PREFIX 1u   /* every frame is preceded by its size as a u32, little endian */

typedef struct wq_pack_counters {
    uint64_t n_in;          /* elements inside the clamped input rows (the ordinals walked) */
    uint64_t n_complete;    /* elements whose whole record lies below capacity_bytes */
    uint64_t bytes_need;    /* bytes of the whole result = d_out_peer_bytes[n_peers] */
    uint64_t bytes_written; /* min(bytes_need, capacity_bytes) */
    uint32_t overflow;      /* bit 0: bytes_need > capacity_bytes */
    uint32_t error;         /* bit 0: a row descended or reached past n_in;
                               bit 1: a message index was >= n_msgs;
                               bit 2: a referenced frame's offsets descend, reach past
                                      n_frame_bytes or span 2^32 bytes or more */
} wq_pack_counters;         /* 40 bytes */

int wq_peer_pack_device(wq_router* h,
        const uint32_t* d_peer_offsets, const uint32_t* d_msgs, uint32_t n_peers, size_t n_in,
        const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n_msgs, size_t n_frame_bytes,
        uint32_t flags,
        uint8_t* d_out, size_t capacity_bytes,
        uint64_t* d_out_peer_bytes,   /* [n_peers + 1], required */
        uint64_t* d_out_elem_bytes,   /* [n_in], nullable */
        wq_pack_counters* d_counters  /* nullable */);

/* ---- frame builder: a tick's flat messages serialized on the device ----
 * wq_serialize_messages (wq_codec.h) builds the frames on the host. For entity updates the device
 * already holds every value that goes into them, so this call writes the same bytes there: the three
 * arrays it leaves are the d_frames / d_frame_offsets / d_msg_size that wq_peer_pack_device and
 * wq_peer_budget_bytes_device take, with bytes_need as n_frame_bytes. An extension like the send
 * buffers: the reference serializes once per message on the host (structures/message.rs:120-134).
 *
 * Flat messages
 *   - A flat message has an instruction, a replication, a sender uuid and a world name, an optional
 *     position, an optional parameter and an optional flex, and no records and no entities (the two
 *     vectors are written, empty, as the host writes them). Messages with records or entities stay with
 *     wq_serialize_messages.
 * Worlds
 *   - wq_frames_set_worlds gives the handle the table world id -> name. names / name_offsets are HOST
 *     arrays: world w is names[name_offsets[w] .. name_offsets[w + 1]), name_offsets has n_worlds + 1
 *     ascending entries.
 *   - WQ_E_INVALID, with the old table kept, for offsets that descend (or a null name_offsets) and for
 *     a name that is not UTF-8 as wq_serialize_message checks it.
 *   - The table is copied: the caller's arrays are free on return. The call waits for the handle's
 *     stream, so it is ordered behind earlier builds and before later ones. n_worlds == 0 clears the
 *     table. It is not a per-tick call.
 * Source (wq_frames_src: device pointers, any alignment)
 *   - instruction / replication: u8 per message, or NULL for instruction_all / replication_all.
 *   - sender_uuid: 16 bytes per message; world: u32 ids into the table. Both required for n_msgs > 0.
 *   - pos: 3 f64 per message, or NULL: no message has a position.
 *   - param / param_offsets / n_param_bytes: message i's parameter is param[po[i] .. po[i + 1]), po =
 *     param_offsets[n_msgs + 1] (u64). NULL / NULL / 0: no message has a parameter. flex likewise.
 *   - msg_flags: u8 per message, bit 0 position, bit 1 parameter, bit 2 flex: the fields the message
 *     has. A bit whose array is NULL counts as clear. NULL: every message has every field whose array
 *     is given.
 * Byte identity
 *   - Frame i is byte for byte what wq_serialize_message writes for the message with those fields,
 *     d_frame_offsets[n_msgs + 1] is what wq_serialize_messages returns in `offsets`, and
 *     d_frame_size[i] (nullable) is frame i's size. Frame i is d_frames[fo[i] .. fo[i + 1]).
 *   - Instruction and replication are written as given: 0 is omitted as the default and any other
 *     value, 255 included, is written, as the host does. Positions are copied as bits, NaN included.
 *     The uuid's text is lower-case hyphenated.
 *   - Parameter bytes are NOT checked for UTF-8 on the device (the host serializer refuses such a
 *     message with WQ_SER_INVALID_UTF8). Byte identity is promised for input the host serializer
 *     accepts.
 * Malformed input (never a fault, never fatal; `error` bits)
 *   - bit 0: a world id >= n_worlds: the world name is empty. With no table set every id is.
 *   - bit 1: a parameter range that descends, reaches past n_param_bytes or spans 2^32 bytes or more:
 *     the parameter is present and empty. bit 2: the same for flex.
 *   - bit 3: a frame above the builder's 2^30 bytes, where the host returns WQ_SER_TOO_LARGE: the
 *     frame is empty, size 0.
 *   - Nothing is dereferenced outside the n_msgs-sized arrays, [0, n_msgs] of the offset arrays,
 *     [0, n_*_bytes) of the payloads and the handle's table, whatever the arrays hold.
 * Capacity
 *   - As wq_peer_pack_device: bytes at positions >= capacity_bytes are not written, everything below
 *     is exact; the offsets, the sizes and the counters are always complete. d_frames == NULL with
 *     capacity_bytes == 0 is the sizing call, which reads no payload byte. n_complete counts the
 *     frames that lie wholly below the capacity.
 * Output guarantees
 *   - Nothing is written outside d_frames[0 .. bytes_written), d_frame_offsets[0 .. n_msgs],
 *     d_frame_size[0 .. n_msgs) and the counters. d_frames must be 16-byte aligned (every hipMalloc
 *     result is), d_frame_offsets 8-byte and d_frame_size 4-byte. Outputs must not alias inputs.
 *   - Deterministic byte for byte: placement comes from a u64 scan, and the only atomics are ORs into
 *     the error word.
 * Execution
 *   - Asynchronous on the handle's stream; nothing is read back. The copy's grid is sized from
 *     capacity_bytes and walks the output bytes: a wave owns 1 KiB of output and a lane 16 bytes, so no
 *     lane, wave or block owns a frame or a payload; a tile that lies inside one payload is copied
 *     with 16-byte loads and stores.
 *   - Scratch lives in the handle, grow-only: 4 n_msgs + 64 bytes (the sizes and the error word) plus
 *     the scan's and the world table (each buffer is allocated a quarter above its need). A
 *     steady-state call does no hipMalloc, and the call may alternate freely with both budget calls
 *     and wq_peer_pack_device on one handle.
 * Limits and handle kinds
 *   - WQ_E_INVALID, with nothing launched, for a null handle, a null src, a null required array with
 *     n_msgs > 0 (d_frame_offsets is always required), param without param_offsets or the reverse
 *     (likewise flex), d_frames == NULL with capacity_bytes > 0, a misaligned d_frames and
 *     n_msgs >= 2^32 - 1.
 *   - Like wq_peer_pack_device the call needs only a stream, scratch and the table: a multi-GPU handle
 *     runs it on its own stream with the arrays on devices[0].
 *   - Building into mapped host memory is not covered here and has not been measured. */
int wq_frames_set_worlds(wq_router* h, const char* names, const uint32_t* name_offsets, uint32_t n_worlds);

typedef struct wq_frames_src {            /* all device pointers */
    const uint8_t*  instruction;  uint8_t instruction_all;   /* NULL: every message has instruction_all */
    const uint8_t*  replication;  uint8_t replication_all;   /* NULL: replication_all */
    const uint8_t*  sender_uuid;                             /* [16 n], required for n > 0 */
    const uint32_t* world;                                   /* [n] ids into the handle's table, required */
    const double*   pos;                                     /* [3 n], NULL: no message has a position */
    const uint8_t*  param; const uint64_t* param_offsets; uint64_t n_param_bytes;  /* NULL/NULL/0: none */
    const uint8_t*  flex;  const uint64_t* flex_offsets;  uint64_t n_flex_bytes;
    const uint8_t*  msg_flags;  /* [n], NULL: every message has every field whose array is given;
                                   bit 0 position, 1 parameter, 2 flex; a bit whose array is NULL counts as clear */
} wq_frames_src;            /* 112 bytes */

typedef struct wq_frames_counters {
    uint64_t n_frames;      /* n_msgs */
    uint64_t n_complete;    /* frames that lie wholly below capacity_bytes */
    uint64_t bytes_need;    /* bytes of all frames = d_frame_offsets[n_msgs] */
    uint64_t bytes_written; /* min(bytes_need, capacity_bytes) */
    uint32_t overflow;      /* bit 0: bytes_need > capacity_bytes */
    uint32_t error;         /* bits 0 - 3 above */
} wq_frames_counters;       /* 40 bytes */

int wq_frames_build_device(wq_router* h, const wq_frames_src* src, size_t n_msgs,
        uint8_t* d_frames, size_t capacity_bytes,
        uint64_t* d_frame_offsets /* [n_msgs + 1], required */,
        uint32_t* d_frame_size    /* [n_msgs], nullable */,
        wq_frames_counters* d_counters /* nullable */);

/* ---- ingest: a tick's received frames decoded on the device ----
 * wq_decode_messages (wq_codec.h) verifies and decodes a tick's frames on the host's cores; the host then
 * sanitizes and interns one world name and looks up one sender uuid per message and uploads four arrays
 * before wq_route_tick_device or wq_follow_peers_device can start. Here the raw frames are uploaded once
 * and verified, decoded and resolved where they land: pos / world / sender / repl are the arrays those
 * calls take. An extension like the frame builder: the reference decodes one message at a time on the
 * host (structures/message.rs:136-142). The contract is wq_decode_messages'.
 *
 * Decode
 *   - Frame i is d_frames[fo[i] .. fo[i + 1]), fo = d_frame_offsets[n_frames + 1], at any alignment.
 *   - Every check of wq_decode_messages, in its order: the FlatBuffers 2.0.0 verifier over Message,
 *     Record and Entity (aligned in-bounds offsets, even vtables, UTF-8 strings with a NUL behind them,
 *     the 2^31 apparent-size, 1,000,000-table and depth limits), then the decode rules (required fields,
 *     records before entities, the uuid's three text forms, instruction codes above 12 become 255,
 *     replication codes above 2 become 0). out->msg[i] is byte for byte what wq_decode_messages writes
 *     for that frame, failed frames included (the struct is zeroed first and has no padding).
 * SoA outputs (wq_ingest_out: device pointers, each nullable; msg and pos 8-byte aligned, the u32 arrays 4)
 *   - pos, repl, instruction, sender_uuid repeat the struct's fields; flex_range is the one it lacks: where
 *     Message.flex lies inside the frame and its length, 0, 0 when absent.
 *   - flags: bit 0 status OK, 1 position, 2 parameter, 3 flex, 4 the world is "@global", 5 the world was
 *     found in the table, 6 the sender was found in the table.
 *   - A frame that is not OK has zeros in all of them, flags 0, world WQ_WORLD_INVALID and sender
 *     0xFFFFFFFF, so it routes to nobody.
 * Worlds
 *   - A decoded world name of exactly "@global" gives WQ_WORLD_GLOBAL (flag bit 4, bit 5 clear).
 *   - Every other name goes through wq_sanitize_world_name's rules on the device, and the result is looked
 *     up among the names of wq_frames_set_worlds: the lowest id with that name wins. A sanitize error, a
 *     name the table does not hold and a handle without a table give WQ_WORLD_INVALID with bit 5 clear,
 *     and count in n_world_unresolved.
 * Senders
 *   - wq_ingest_set_peers copies a uuid -> id table (HOST arrays: 16 bytes per uuid; ids NULL: id = index)
 *     into the handle. Not a per-tick call: it sorts on the host and waits for the handle's stream.
 *     n == 0 clears the table. WQ_E_INVALID, with the old table kept, for a uuid that occurs twice or a
 *     null uuids with n > 0.
 *   - A sender the table lacks gives 0xFFFFFFFF (bit 6 clear, counted in n_sender_unknown); its uuid is in
 *     sender_uuid, so the host handles the tick's few joins and not every message.
 * Hostile input (never a fault, never fatal)
 *   - error bit 0: an offset is suspect when it lies past n_frame_bytes or stands in a descending pair
 *     (either side may be the wrong one). A frame with a suspect offset — its own pair descends or
 *     reaches past the end, or a neighbour's does at the offset they share — cannot be told from its
 *     neighbours and is WQ_DEC_INVALID_FLATBUFFER; every other frame is decoded as usual.
 *     (wq_decode_messages returns -1 for the whole call when offsets descend: the one difference.)
 *   - error bit 1: a frame of 2^32 bytes or more is WQ_DEC_INVALID_FLATBUFFER. Parity is promised below.
 *   - No byte is read outside d_frames[0 .. n_frame_bytes) and d_frame_offsets[0 .. n_frames], whatever
 *     the frames say; every loop over frame content is bounded by the frame's size or the verifier's
 *     limits; nothing spins.
 * Execution
 *   - Asynchronous on the handle's stream; nothing is read back. Three launches: the walk (one lane per
 *     frame; strings of up to 256 bytes are validated there), the long strings (longer strings go through
 *     a fixed-capacity work list and are validated 16 bytes per lane; a lane that finds the list full
 *     validates its string itself, with the same result), the finish (frames a long string overturned,
 *     and the counters: per-block sums added with integer atomics). Deterministic byte for byte.
 *   - Scratch lives in the handle, grow-only: 4 n_frames bytes, the work list (16 bytes an entry, 65,536
 *     entries) and 128 bytes. A steady-state call does no hipMalloc, and the call alternates freely with
 *     the route, budget, builder and pack calls on one handle.
 * Limits and handle kinds
 *   - WQ_E_INVALID, with nothing launched, for a null handle or out, a null d_frame_offsets with
 *     n_frames > 0, a null d_frames with n_frame_bytes > 0 and n_frames >= 2^32 - 1.
 *   - A multi-GPU handle runs the call on its own stream with the arrays on devices[0], as the builder.
 *   - Compacting parameter and flex payloads for wq_frames_build_device, and mapped host memory, are not
 *     covered here. */
int wq_ingest_set_peers(wq_router* h, const uint8_t* uuids /* host, [16 n] */,
                        const uint32_t* ids /* host, [n], NULL: id = index */, uint32_t n);

typedef struct wq_ingest_out {       /* device pointers, each nullable */
    struct wq_decoded_msg* msg;      /* [n]   byte for byte what wq_decode_messages writes (wq_codec.h) */
    double*   pos;                   /* [3 n] */
    uint32_t* world;                 /* [n]   world id, WQ_WORLD_GLOBAL, or WQ_WORLD_INVALID */
    uint32_t* sender;                /* [n]   peer id, or 0xFFFFFFFF */
    uint8_t*  repl;                  /* [n] */
    uint8_t*  instruction;           /* [n] */
    uint8_t*  sender_uuid;           /* [16 n] */
    uint32_t* flex_range;            /* [2 n] off, len inside the frame; 0, 0 when absent */
    uint8_t*  flags;                 /* [n] bits 0 - 6 above */
} wq_ingest_out;            /* 72 bytes */

typedef struct wq_ingest_counters {
    uint64_t n_frames, n_ok, n_invalid, n_missing, n_bad_uuid;  /* frames per status */
    uint64_t n_world_unresolved, n_sender_unknown;              /* among the OK frames */
    uint32_t error;         /* bits 0 and 1 above */
    uint32_t pad_;
} wq_ingest_counters;       /* 64 bytes */

int wq_frames_decode_device(wq_router* h, const uint8_t* d_frames, const uint64_t* d_frame_offsets,
                            size_t n_frames, size_t n_frame_bytes,
                            const wq_ingest_out* out, wq_ingest_counters* d_counters /* nullable */);

/* ---- ingest dispatch: a decoded tick split by instruction on the device ----
 * wq_frames_decode_device leaves pos / world / sender / repl / instruction / flags for every frame of a
 * tick, whatever its instruction. The reference dispatches one message at a time on the host
 * (processing/thread.rs:72-108: heartbeats at once, the subscription task in order, the database task in
 * order) and its handlers drop what they drop; processing.SubscriptionProcessor.process_tick restates
 * that as a Python loop. Here one call takes the decode's arrays and writes, in arrival order, the
 * compact inputs of wq_route_tick_device, wq_route_global_device and wq_apply_ops_device, the frame
 * indices the host must see, and the table of runs that says in which order to issue those calls.
 * Nothing is read back until the counters and the run table. An extension like the decoder.
 *
 * Classes (out->cls[i]; the first rule that matches decides)
 *   "@global" means flag bit 4. "World resolved" means flag bit 5 AND world < WQ_WORLD_GLOBAL. "Sender
 *   known" means flag bit 6 AND sender != 0xFFFFFFFF. "Position" means flag bit 1.
 *   - WQ_CLS_BAD        flag bit 0 clear: the frame did not decode. Nothing else of it is looked at.
 *   - WQ_CLS_HEARTBEAT  instruction 0 (thread.rs:76-81). Listed in side_src. With in->last_seen given and
 *                       a known sender < n_last_seen, last_seen[sender] = now: a plain store, every
 *                       writer writes the same value, so the result is deterministic.
 *   - WQ_CLS_LOCAL      instruction 7, not "@global", position, world resolved (local_message.rs:17-56
 *                       passed). One row in l_*: the frame index, the position copied as bits, world,
 *                       sender, repl.
 *   - WQ_CLS_GLOBAL     instruction 6, not "@global", world resolved (global_message.rs:37-54 passed).
 *                       One row in g_*.
 *   - WQ_CLS_BCAST      instruction 6 to "@global": the PeerMap broadcast of global_message.rs:18-35.
 *                       Listed in side_src, the host's to send.
 *   - WQ_CLS_OP         instruction 4 or 5, not "@global", position, world resolved, sender known
 *                       (area_subscribe.rs:17-46, area_unsubscribe.rs passed). One wq_op: world, peer =
 *                       sender, kind WQ_OP_SUBSCRIBE / WQ_OP_UNSUBSCRIBE, key_is_raw 0, pad_ zero, the
 *                       position as bits; op_src holds its frame index.
 *   - WQ_CLS_DEFERRED   instruction 4 with a position, not "@global", whose world or sender did not
 *                       resolve: a join. The host interns the world or assigns the id. Listed in side_src.
 *   - WQ_CLS_DB         instructions 8, 9, 11 (thread.rs:96-104). Listed in arrival order; the record path
 *                       is the caller's.
 *   - WQ_CLS_OTHER      instructions 1, 2, 3, 10, 12, 255 and any other byte. Listed; the reference
 *                       panics or warns (thread.rs:83-94, 136).
 *   - WQ_CLS_DROPPED    what the reference's handlers drop silently: Local / Subscribe / Unsubscribe to
 *                       "@global"; Local / Subscribe / Unsubscribe without a position; a Local or Global
 *                       whose world did not resolve (sanitize error or "no subscriptions in this world");
 *                       an Unsubscribe whose world or sender did not resolve (a peer without an id holds
 *                       nothing).
 *   - A decoded frame whose flag and value disagree (bit 5 against world < WQ_WORLD_GLOBAL, bit 4 against
 *     world == WQ_WORLD_GLOBAL, bit 6 against sender != 0xFFFFFFFF) sets error bit 0, and what disagrees
 *     counts as unresolved. The input arrays are the caller's and may hold anything: an emitted wq_op
 *     never carries a reserved world or the no-peer id (wq_apply_ops_device refuses a whole batch for one
 *     such op), and a LocalMessage or GlobalMessage row whose sender is not known carries 0xFFFFFFFF, as
 *     SubscriptionProcessor._sender_id passes it.
 *   - The class counts sum to n_frames.
 * Rows
 *   - l_*, g_*, ops / op_src hold their class's frames in ascending frame index; side_src holds five
 *     lists one behind the other — heartbeat | "@global" broadcast | database | other | deferred — each
 *     ascending, side_begin[k] .. side_begin[k + 1] of the counters. Every row array has room for
 *     n_frames rows; only [0, count) of each is written.
 * Runs
 *   - Only OP frames (table events) and LOCAL / GLOBAL frames (read events) are effective. A run is a
 *     maximal stretch of effective frames of one kind, every other class ignored: process_tick's batching
 *     with the events that have no effect left out, so there are never more runs than there. A dropped
 *     event neither reads nor changes the table, so leaving it out of the rule changes no outcome.
 *   - runs[r] = { kind (WQ_RUN_TABLE / WQ_RUN_READ), the run's first frame, where its rows begin in l_*,
 *     g_* and ops }. Run r's rows end where run r + 1's begin; runs[n_runs] closes the table with kind
 *     WQ_RUN_END, first_frame = n_frames and the three totals. Rows are stable, so a run's rows are
 *     contiguous. With n_runs + 1 > runs_capacity the first runs_capacity entries are written and overflow
 *     bit 0 is set.
 *   - The caller reads the counters and the run table once, then issues in run order
 *     wq_apply_ops_device(ops + op_begin, count) for a table run, and wq_route_tick_device /
 *     wq_route_global_device on slices of l_* / g_* for a read run. The route kernels read their inputs
 *     with scalar element loads at natural alignment, so a slice that begins at any row is a valid input
 *     (tests/test_gpu_ingest_dispatch.py pins it).
 *   - With n_deferred == 0 the outcome equals the reference's sequential loop. With deferred joins it is
 *     exact for every frame before first_deferred; the caller either accepts that the joiners' events take
 *     effect one tick later, or updates its tables and dispatches the suffix again. A deferred frame
 *     whose world name the host then finds refused by the sanitizer is dropped there, as
 *     area_subscribe.rs:23-33 drops it; it never had an effect, so it does not limit what is exact.
 *   - Disconnects arrive on another channel (remove_rx, thread.rs:124-125) and stay wq_remove_peers
 *     between ticks.
 * Execution
 *   - Asynchronous on the handle's stream; nothing is read back. Three launches, no lane waits for
 *     another: classify (one lane per frame; a summary per block of 1,024 frames), scan (one block over
 *     the block summaries; it writes the counters and the closing run), emit (every lane places its row at
 *     its block's base + the frames of its class below it). n_frames == 0 runs the scan alone and writes
 *     the counters and the closing run only. Deterministic byte for byte.
 *   - Nothing is written outside [0, count) of each array, [0, min(n_runs + 1, runs_capacity)) of runs and
 *     the counters; the inputs are never written, apart from last_seen. Arrays are at their element's
 *     natural alignment (pos, l_pos, ops 8 bytes; the u32 arrays and runs 4).
 *   - Scratch lives in the handle, grow-only: n_frames bytes and 60 bytes per 1,024 frames. A steady-state
 *     call does no hipMalloc, and the call alternates freely with decode, route, apply, budget, builder
 *     and pack on one handle.
 *   - WQ_E_INVALID, with nothing launched, for a null handle, in or out, a null required array with
 *     n_frames > 0, runs null with runs_capacity > 0 and n_frames >= 2^32 - 1.
 *   - A multi-GPU handle runs the call on its own stream with the arrays on devices[0]. */
#define WQ_CLS_BAD 0
#define WQ_CLS_HEARTBEAT 1
#define WQ_CLS_LOCAL 2
#define WQ_CLS_GLOBAL 3
#define WQ_CLS_BCAST 4
#define WQ_CLS_OP 5
#define WQ_CLS_DEFERRED 6
#define WQ_CLS_DB 7
#define WQ_CLS_OTHER 8
#define WQ_CLS_DROPPED 9
#define WQ_CLS_COUNT 10

#define WQ_RUN_END 0
#define WQ_RUN_TABLE 1
#define WQ_RUN_READ 2

typedef struct wq_dispatch_in {      /* device pointers: the arrays wq_frames_decode_device wrote */
    const uint8_t*  instruction;     /* [n] required */
    const uint8_t*  flags;           /* [n] required: bits 0 - 6 of wq_ingest_out.flags */
    const uint32_t* world;           /* [n] required */
    const uint32_t* sender;          /* [n] required */
    const uint8_t*  repl;            /* [n] required */
    const double*   pos;             /* [3 n] required */
    uint32_t*       last_seen;       /* [n_last_seen] nullable: heartbeat stamps, see above */
    uint32_t        n_last_seen, now;
} wq_dispatch_in;            /* 64 bytes */

typedef struct wq_dispatch_run { uint32_t kind, first_frame, l_begin, g_begin, op_begin; } wq_dispatch_run; /* 20 B */

typedef struct wq_dispatch_out {     /* device pointers, each nullable; every row array holds n_frames rows */
    uint8_t*  cls;                   /* [n] the class of every frame (WQ_CLS_*) */
    uint32_t* l_src; double* l_pos; uint32_t* l_world; uint32_t* l_sender; uint8_t* l_repl;  /* LocalMessage rows */
    uint32_t* g_src; uint32_t* g_world; uint32_t* g_sender; uint8_t* g_repl;                 /* GlobalMessage rows */
    wq_op*    ops;   uint32_t* op_src;                                                       /* table ops */
    uint32_t* side_src;              /* [n] heartbeat | @global broadcast | database | other | deferred, each ascending */
    wq_dispatch_run* runs; uint32_t runs_capacity;   /* runs[0 .. min(n_runs + 1, capacity)) incl. the closing entry */
    uint32_t pad_;
} wq_dispatch_out;           /* 120 bytes */

typedef struct wq_dispatch_counters {
    uint64_t n_frames;
    uint64_t n_bad, n_heartbeat, n_local, n_global, n_bcast, n_op, n_deferred, n_db, n_other, n_dropped; /* per WQ_CLS_* */
    uint64_t n_runs;
    uint64_t side_begin[6];  /* the starts of the five lists inside side_src, and the end */
    uint64_t first_deferred; /* the frame index of the first deferred event; n_frames when there is none */
    uint64_t overflow;       /* bit 0: n_runs + 1 > runs_capacity */
    uint64_t error;          /* bit 0: a flag and its value disagree */
} wq_dispatch_counters;      /* 168 bytes */

int wq_ingest_dispatch_device(wq_router* h, const wq_dispatch_in* in, size_t n_frames,
                              const wq_dispatch_out* out, wq_dispatch_counters* d_counters /* nullable */);

/* ---- ingest joins: new senders get their peer ids on the device ----
 * An AreaSubscribe from a uuid the sender table lacks is WQ_CLS_DEFERRED above: the host reads the uuids
 * back, assigns ids, rebuilds the whole table with wq_ingest_set_peers and dispatches the suffix again.
 * Here one call between the decode and the dispatch assigns the ids with the caller's allocator state
 * (the convention of wq_records_dispatch_device's handles), patches the decode's sender / flags in place
 * and merges the new uuids into the handle's table, so the dispatch that follows sees no deferred sender
 * and the next tick's decode resolves the joiners. World-name joins stay deferred and stay the host's.
 * An extension like the decoder; the host definitions are ingest.join_peers_np / ingest.drop_peers_np and
 * the arithmetic is csrc/join_ops.hpp.
 *
 * wq_ingest_peers_reserve (host call, not per tick; waits for the stream)
 *   - The sender table gets room for `capacity` entries (existing entries are kept; a capacity below the
 *     reserved one or below the live count keeps the larger room) and its live count becomes a device
 *     word the handle owns, which the decode reads. capacity >= 2^32 - 1 is WQ_E_INVALID.
 *   - wq_ingest_set_peers keeps working as before and keeps the reserved room (n > capacity grows it).
 *     Without a reserve the handle behaves exactly as before.
 * wq_ingest_join_device
 *   - Candidate: a frame with flag bit 0, instruction 4, flag bit 1 (position), not flag bit 4, world
 *     resolved (bit 5 and world < WQ_WORLD_GLOBAL) and sender not known (bit 6 clear or sender ==
 *     0xFFFFFFFF): exactly a frame the dispatch classes WQ_CLS_DEFERRED for its sender alone. A subscribe
 *     whose world did not resolve is no candidate: it stays deferred, and so does its sender. A candidate
 *     whose uuid the handle's table already holds (the arrays were not decoded against this table) is no
 *     candidate either and sets error bit 0: the table never holds a uuid twice.
 *   - Joins: the distinct uuids of the candidates, ordered by the frame index of their first candidate
 *     (first_frame). Join k gets free_ids[k] for k < n_free, else id_next + (k - n_free); the caller
 *     passes its free list in pop order. out->j_uuid[16 k], j_id[k], j_frame[k] = first_frame list them.
 *   - Patch: every frame i with flag bit 0 set and sender not known whose uuid joined gets sender[i] = id
 *     and flag bit 6, but only when i >= first_frame of that uuid: as in the reference's sequential loop,
 *     an unsubscribe or heartbeat that precedes a peer's first subscribe sees a peer without an id.
 *   - Table: the joins are merged into the handle's sender table, keys ascending as before, and the live
 *     count is updated on the device.
 *   - All or nothing: with an overflow bit set sender, flags, the table and j_* are untouched and the
 *     counters say what was needed (n_joined is what would have joined, n_patched 0, n_free_used 0,
 *     id_next and n_table unchanged). overflow bit 0: more joins than n_free + (id_limit - id_next);
 *     bit 1: live + joins above the reserved capacity; bit 2: more joins than joined_capacity (looked at
 *     only when one of j_uuid / j_id / j_frame is given). The frames then stay deferred and the host path
 *     above still works.
 *   - wq_join_counters: n_frames, n_candidates, n_joined, n_patched, n_free_used, id_next (after),
 *     n_table (after), first_join (the first join's frame index; n_frames when none or on overflow),
 *     overflow, error. error bit 0: a decoded frame's flag and value disagree, as in the dispatch (what
 *     disagrees counts as unresolved). error bit 1: the handle has no reserved table; the call is then a
 *     no-op: nothing is written but the counters, with n_frames, error bit 1, first_join = n_frames,
 *     id_next as given and everything else 0.
 *   - Asynchronous on the handle's stream, nothing read back, deterministic byte for byte (the only
 *     atomics are integer adds and ORs into the counters). Scratch lives in the handle, grow-only: 69
 *     bytes per frame and 12 per 64 frames, 20 bytes per reserved table entry (the table's second buffer
 *     during a merge) and the sort's temporary storage; a steady-state
 *     call does no hipMalloc. The passes over the frames have n_frames lanes; the table passes read the
 *     number of joins on the device and return at once when it is zero. No lane owns a uuid's frames.
 *   - WQ_E_INVALID, nothing launched: a null handle, in or out; a null instruction, flags, world,
 *     sender_uuid or sender with n_frames > 0; n_free > 0 without free_ids; n_frames >= 2^32 - 1;
 *     id_next > id_limit.
 *   - A multi-GPU handle runs the call on its own stream with the arrays on devices[0], as the decoder.
 * wq_ingest_drop_peers_device (the leave side)
 *   - Every table entry whose id is in d_ids[n] is removed by a stable compaction (keys stay ascending)
 *     and the live count is updated on the device. Ids the table lacks and duplicates are ignored.
 *     Asynchronous, nothing read back. A server calls it with the ids it gives to wq_remove_peers, before
 *     those ids go back on its free list: a reused id then never resolves from its old uuid.
 *   - Counters: n_frames = n, n_patched = the entries removed, n_table (after), first_join = n, error
 *     bit 1 and a no-op without a reserved table; every other field 0. Scratch: 4 n bytes, 20 bytes per
 *     reserved entry. WQ_E_INVALID for a null handle, a null d_ids with n > 0 and n >= 2^32 - 1.
 * wq_ingest_peers_read (host call; waits for the stream)
 *   - The live table, keys ascending: uuids[16 i], ids[i]. *n is the live count; with both arrays null it
 *     is only counted (the sizing convention of wq_records_drain_dead); else capacity < *n is WQ_E_INVALID
 *     with *n set. Works with and without a reserve. For snapshots and tests. */
typedef struct wq_join_in {          /* device pointers: the arrays wq_frames_decode_device wrote */
    const uint8_t*  instruction;     /* [n] required */
    const uint32_t* world;           /* [n] required */
    const uint8_t*  sender_uuid;     /* [16 n] required */
    uint8_t*        flags;           /* [n] required, patched in place */
    uint32_t*       sender;          /* [n] required, patched in place */
    const uint32_t* free_ids;        /* [n_free] nullable with n_free 0: the free list in pop order */
    uint32_t        n_free, id_next, id_limit, pad_;
} wq_join_in;                /* 64 bytes */

typedef struct wq_join_out {         /* device pointers, each nullable */
    uint8_t*  j_uuid;                /* [16 joined_capacity] */
    uint32_t* j_id;                  /* [joined_capacity] */
    uint32_t* j_frame;               /* [joined_capacity] */
    uint32_t  joined_capacity, pad_;
} wq_join_out;               /* 32 bytes */

typedef struct wq_join_counters {
    uint64_t n_frames, n_candidates, n_joined, n_patched, n_free_used;
    uint64_t id_next, n_table, first_join, overflow, error;
} wq_join_counters;          /* 80 bytes */

int wq_ingest_peers_reserve(wq_router* h, size_t capacity);
int wq_ingest_join_device(wq_router* h, const wq_join_in* in, size_t n_frames, const wq_join_out* out,
                          wq_join_counters* d_counters /* nullable */);
int wq_ingest_drop_peers_device(wq_router* h, const uint32_t* d_ids, size_t n,
                                wq_join_counters* d_counters /* nullable */);
int wq_ingest_peers_read(wq_router* h, uint8_t* uuids /* host, [16 capacity] */, uint32_t* ids /* host */,
                         size_t capacity, size_t* n);

/* ---- ingest leaves: stale and disconnected senders leave on the device ----
 * The dispatch stamps last_seen[sender] = now for every heartbeat, and the join brings new senders in
 * without a host leg; the way out was the host's: download the stamps, compare, wq_remove_peers (which
 * builds and uploads a bitmap and waits), wq_ingest_drop_peers_device, the free list, and the uuid text of
 * every PeerDisconnect made per peer. Here one call finds who leaves and writes everything that hangs on
 * it, and a second takes the first one's bitmap through WorldMap::remove_peer. Reference:
 * transport/peer.rs:50-69 (is_stale: now - last_heartbeat > max_duration, strict; WebSocket peers never),
 * transport/zeromq/outgoing.rs:132-150 (collect the stale set, then remove each),
 * transport/peer_map.rs:121-141 (remove broadcasts PeerDisconnect with parameter = uuid.to_string()),
 * processing/thread.rs:124-125 -> WorldMap::remove_peer. An extension like the join; the host definition is
 * ingest.leave_peers_np and the arithmetic is csrc/leave_ops.hpp.
 *
 * wq_ingest_leave_device
 *   - Walks the live entries of the handle's sender table (wq_ingest_peers_reserve; the live count is the
 *     device word). An entry with id < n_ids leaves when its id is in leave_ids[n_leave] (the disconnects
 *     the transport reported) or when it is stale: its bit in pinned_bits is clear (pinned ids are never
 *     stale: the WebSocket rule), stamp = last_seen[id] != WQ_SEEN_NEVER, now > stamp and
 *     now - stamp > max_age. A stamp in the future is not stale. Listed ids the table lacks, listed ids
 *     >= n_ids and duplicates are ignored. A live entry with id >= n_ids is never judged, never stamped
 *     and sets error bit 2. The table's ids are distinct.
 *   - WQ_SEEN_NEVER (0xFFFFFFFF) means "not seen yet": the caller initialises last_seen to all ones, and
 *     the join does not stamp a joiner. A live entry that does not leave and carries it gets
 *     last_seen[id] = now, so a joiner's clock starts at the first sweep after it joined: at most one sweep
 *     interval later than the reference's Peer::new_zmq, which starts it at creation. Every leaver's stamp
 *     is reset to WQ_SEEN_NEVER, so a recycled id starts fresh and never inherits its previous owner's
 *     stamp. now == WQ_SEEN_NEVER is WQ_E_INVALID.
 *   - Leavers are listed in table order (uuid ascending), leaver k of n_left in row k of the out arrays,
 *     each nullable, leave_capacity rows: l_uuid[16 k], l_id[k], l_reason[k] (bit 0 listed, bit 1 stale),
 *     l_param[36 k ..) = the uuid as lower-case hyphenated text with l_param_offsets[k] = 36 k and the
 *     entry l_param_offsets[n_left] behind them (leave_capacity + 1 entries): exactly the param /
 *     param_offsets pair of wq_frames_src, so the PeerDisconnect frames come from wq_frames_build_device
 *     with no text made on the host.
 *   - gone_bits[ceil(n_ids / 32)]: one bit per leaver's id, every other bit zero; always written whole
 *     (also without a reserved table), all zeros on overflow. What wq_remove_peers_device takes.
 *   - free_out[free_capacity]: the caller's new free list in pop order: the leavers' ids in reverse leave
 *     order, then free_ids[0 .. n_free) (its free list in pop order, as the join takes it). That is what
 *     releasing the leavers in leave order leaves. free_out must not overlap free_ids.
 *   - The sender table loses the leavers by a stable compaction (keys stay ascending) and the live count is
 *     updated on the device: the next decode no longer resolves them.
 *   - wq_leave_counters: n_table_before, n_listed (= n_leave), n_listed_found (live entries whose id is
 *     listed), n_stale (live entries that are stale, listed or not), n_left, n_stamped (clocks started),
 *     n_table (after), n_free (the free list's length after), overflow, error. n_left is the device word
 *     wq_remove_peers_device reads as d_count.
 *   - All or nothing: overflow bit 0: n_left > leave_capacity (looked at only when an l_* array is
 *     given); bit 1: n_free + n_left > free_capacity (only when free_out is given). With either set no
 *     stamp, no table entry, no l_* row and no free_out entry is written, gone_bits is zero and the
 *     counters say what was needed: n_left is what would have left, n_stamped 0, n_table and n_free as
 *     before the call.
 *   - error bit 1: the handle has no reserved table; the call is then a no-op: gone_bits is zeroed and the
 *     counters hold n_listed, n_free as given and error bit 1, everything else 0. error bit 2 above.
 *   - Asynchronous on the handle's stream, nothing read back, deterministic byte for byte: no lane owns a
 *     peer, every placement comes from one scan, and the only atomics are integer ORs into the bitmaps and
 *     integer adds / ORs into the counters. Scratch lives in the handle, grow-only: 21 bytes per reserved
 *     table entry (20 of them the table's second buffer, shared with the join), 12 per 64 entries and 4
 *     per 32 ids; a steady-state call does no hipMalloc. Every table pass has one lane per reserved entry
 *     and reads the live count on the device.
 *   - WQ_E_INVALID, nothing launched: a null handle, in or out; a null last_seen with n_ids > 0; n_leave > 0
 *     without leave_ids; n_free > 0 without free_ids; n_ids, n_leave or n_free >= 2^32 - 1; now ==
 *     WQ_SEEN_NEVER.
 *   - A multi-GPU handle runs the call on its own stream with the arrays on devices[0], as the join.
 * wq_remove_peers_device
 *   - wq_remove_peers for the ids < n_ids whose bit is set in d_bits[ceil(n_ids / 32)]: every world, in
 *     place, the same kernel on the same pass, with the same results. Follow state, peer positions and
 *     last_seen are left alone, as wq_remove_peers leaves them.
 *   - No bitmap is built on the host, nothing is uploaded and the call does not wait for the stream;
 *     d_bits (and *d_count) must stay unchanged until the stream has passed the call. A batch still in
 *     flight is folded in first, as in wq_remove_peers; an empty table launches nothing.
 *   - d_count (nullable): a device u64, the number of set bits or any value that is 0 only when no bit
 *     is set (wq_leave_counters.n_left). With *d_count == 0 every block returns before it touches the
 *     table.
 *   - The host cannot know whether a bit is set, so the call invalidates what wq_remove_peers
 *     invalidates (the table generation, the compact headers, the sorted state) whether or not anybody is
 *     removed. It belongs at the sweep interval, not in every tick; the reference sweeps on a timer too.
 *   - WQ_E_INVALID: a null handle; a null d_bits with n_ids > 0; a multi-GPU handle (its shards take the
 *     ids on the host: wq_remove_peers). */
#define WQ_SEEN_NEVER 0xFFFFFFFFu    /* last_seen: not seen yet */

typedef struct wq_leave_in {         /* device pointers unless noted */
    uint32_t*       last_seen;       /* [n_ids] required with n_ids > 0; written */
    const uint32_t* pinned_bits;     /* [ceil(n_ids / 32)] nullable: ids that are never stale */
    const uint32_t* leave_ids;       /* [n_leave] nullable with n_leave 0 */
    const uint32_t* free_ids;        /* [n_free] nullable with n_free 0: the free list in pop order */
    uint32_t        n_ids, now, max_age, n_leave, n_free, pad_;   /* host values */
} wq_leave_in;               /* 56 bytes */

typedef struct wq_leave_out {        /* device pointers, each nullable */
    uint8_t*  l_uuid;                /* [16 leave_capacity] */
    uint32_t* l_id;                  /* [leave_capacity] */
    uint8_t*  l_reason;              /* [leave_capacity] */
    uint8_t*  l_param;               /* [36 leave_capacity] */
    uint64_t* l_param_offsets;       /* [leave_capacity + 1] */
    uint32_t* gone_bits;             /* [ceil(n_ids / 32)] */
    uint32_t* free_out;              /* [free_capacity] */
    uint32_t  leave_capacity, free_capacity;
} wq_leave_out;              /* 64 bytes */

typedef struct wq_leave_counters {
    uint64_t n_table_before, n_listed, n_listed_found, n_stale;
    uint64_t n_left, n_stamped, n_table, n_free, overflow, error;
} wq_leave_counters;         /* 80 bytes */

int wq_ingest_leave_device(wq_router* h, const wq_leave_in* in, const wq_leave_out* out,
                           wq_leave_counters* d_counters /* nullable */);
int wq_remove_peers_device(wq_router* h, const uint32_t* d_bits, uint32_t n_ids, const uint64_t* d_count /* nullable */);

/* ---- record store: RecordCreate / RecordRead / RecordDelete ----
 * The reference sends these three instructions to DatabaseClient (database/client.rs) and PostgreSQL.
 * Here the spatial index of the records lives in the handle: one row per stored record holding its
 * region, table, uuid, time and the caller's `handle`. The record's text and bytes (data, flex, the
 * exact x, y, z) stay with the caller under that handle; the GPU never sees them.
 *
 * A store is configured like DatabaseClient (args.rs:194-224): region sizes >= 1 and a table size
 * that each of them divides, else WQ_E_INVALID. The region of a position is clamp_region_coord per
 * axis (world_region.rs:18-35, 93-110) and the table of a region clamp_table_size of its minimum
 * corner (world_region.rs:112-129).
 *
 *   - Times are microseconds given by the caller per op; "no after" is INT64_MIN.
 *   - The store numbers every op it ever received. Among rows of one uuid with equal times the one
 *     with the higher number is "met later" (record_read.rs:61-81) and is the one a read returns.
 *     PostgreSQL leaves that order open; this is parity with the restatement in records.py.
 *   - Ops of one batch act in op order: a delete removes the matching rows with a lower number,
 *     creates earlier in the same batch included, later ones not.
 *   - Every query of one read call is answered from the store as it was when the call began, and all
 *     of the call's dedupe deletions apply afterwards (the reference dedupes "in background"). This
 *     differs from the reference's one-query-at-a-time loop in one case: two queries of one call read
 *     different regions of one table that hold the same uuid with different times; the stale copy is
 *     still returned once. Single-query calls reproduce the sequential reference exactly.
 *   - A reply row lists its records by ascending (uuid_hi, uuid_lo) (the reference's HashMap order
 *     is random).
 *   - Limits: a position is packable when every axis's region index (region minimum / region size)
 *     lies in [-2^23, 2^23) and the world id is < 2^24 - 1. Ops and queries that are not packable or
 *     hold a NaN coordinate are rejected and counted, never stored or answered; a rejected query
 *     gets an empty row. Rows are appended and never moved until wq_records_vacuum: a dead row's
 *     slot is not reused, and rows_stored counts the dead until a vacuum drops them. The
 *     regions of one read call together hold fewer than 2^32 - 64 rows, a region counted once per
 *     query that asks it (the offsets are u32); a call past that returns WQ_E_CAPACITY, answers
 *     nothing and kills nothing: split it. A multi-GPU handle has no record store (WQ_E_INVALID). */
#define WQ_RECORD_CREATE 0u /* DatabaseClient::insert_records, database/client.rs + query_constants.rs */
#define WQ_RECORD_DELETE 1u /* DatabaseClient::delete_records, query_delete_record */
#define WQ_RECORD_READ_DEDUPE 1u /* flags bit 0: DatabaseClient::dedupe_records, query_delete_duplictes */
typedef struct wq_rec_op {
    uint32_t kind; /* WQ_RECORD_CREATE | WQ_RECORD_DELETE */
    uint32_t world;
    double pos[3];
    uint64_t uuid_hi, uuid_lo;
    int64_t ts_us;   /* create: the row's last_modified; delete: unused */
    uint32_t handle; /* create: the caller's payload slot; delete: unused */
    uint32_t reserved;
} wq_rec_op; /* 64 bytes */
typedef struct wq_rec_apply_result {
    uint64_t created, deleted_rows, rejected, rows_live;
} wq_rec_apply_result;
typedef struct wq_rec_read_result {
    uint64_t returned, deduped_rows, rejected;
    uint64_t scanned;  /* rows of the queried regions the call walked (a region asked twice counts twice) */
    uint32_t overflow; /* 1: `returned` exceeds the capacity; the pairs past it were not written */
    uint32_t error;    /* reserved: 0 */
} wq_rec_read_result;

/* DatabaseClient::new (database/client.rs): opens the handle's (empty) store. */
int wq_records_open(wq_router* h, uint16_t region_x_size, uint16_t region_y_size, uint16_t region_z_size,
                    uint32_t table_size);
int wq_records_close(wq_router* h);
/* insert_records / delete_records for a batch of ops in op order. wq_records_apply uploads the ops
 * and waits for the result; wq_records_apply_device reads them from device memory, is asynchronous
 * on the handle's stream and reads nothing back (d_ops stays valid until the stream has passed the
 * call; what it created, deleted and rejected is counted in wq_records_totals). */
int wq_records_apply(wq_router* h, const wq_rec_op* ops, size_t n, wq_rec_apply_result* out);
int wq_records_apply_device(wq_router* h, const wq_rec_op* d_ops, size_t n);
/* get_records_in_region + handle_record_read (record_read.rs:43-96) for n queries, and with
 * WQ_RECORD_READ_DEDUPE dedupe_records for every returned row. after_us may be null (no `after`).
 * Output: a CSR, offsets[n + 1] and per returned row handles[] and ts_us[]; pairs at index >=
 * capacity are not written, the offsets are always complete. Both forms wait for the call's totals
 * (one read at the end); the _device form takes device arrays, `out` is host memory in both. */
int wq_records_read(wq_router* h, size_t n, const uint32_t* world, const double* pos, const int64_t* after_us,
                    uint32_t flags, uint32_t* offsets, uint32_t* handles, int64_t* ts_us, size_t capacity,
                    wq_rec_read_result* out);
int wq_records_read_device(wq_router* h, size_t n, const uint32_t* d_world, const double* d_pos,
                           const int64_t* d_after_us, uint32_t flags, uint32_t* d_offsets, uint32_t* d_handles,
                           int64_t* d_ts_us, size_t capacity, wq_rec_read_result* out);
/* Handles of the rows killed by deletes and dedupes since the last drain, ascending, so the caller
 * frees their payload slots. *n is the count; with *n > capacity nothing is drained (WQ_E_CAPACITY). */
int wq_records_drain_dead(wq_router* h, uint32_t* out, size_t capacity, size_t* n);
int wq_records_stats(wq_router* h, uint64_t* rows_live, uint64_t* rows_stored, uint64_t* ops_seen);
/* Counts since wq_records_open, the asynchronous applies included (waits for the stream): nothing an
 * apply or a read rejected goes uncounted. */
typedef struct wq_rec_totals {
    uint64_t created, deleted_rows, deduped_rows, rejected_ops, rejected_queries;
} wq_rec_totals;
int wq_records_totals(wq_router* h, wq_rec_totals* out);

/* ---- record store: vacuum and snapshots ----
 * One stored row as a snapshot carries it. `region` is the region's minimum corner per axis, as
 * wq_region_quantize returns it; `seq` the number of the op that created the row. */
typedef struct wq_rec_row {
    uint32_t world, handle;
    int64_t region[3];
    uint64_t uuid_hi, uuid_lo;
    int64_t ts_us;
    uint64_t seq;
} wq_rec_row; /* 64 bytes */
typedef struct wq_rec_vacuum_result {
    uint64_t rows_before, rows_after; /* rows stored */
    uint64_t bytes_before, bytes_after; /* the row arrays, the dead list and the views */
} wq_rec_vacuum_result;
typedef struct wq_rec_import_result {
    uint64_t imported, rejected;
} wq_rec_import_result;
/* Drops the dead rows: the live ones move together in their order (they keep seq, ts_us and handle),
 * both views are renumbered and every array is reallocated to fit. Nothing a later apply, read,
 * drain or total returns changes; wq_records_stats then reports rows_stored == rows_live, and the
 * store's limit of 2^32 - 1 rows counts live rows again. Handles not yet drained stay in the dead
 * list. Synchronous. A store with nothing dead is left as it is. `out` may be null. */
int wq_records_vacuum(wq_router* h, wq_rec_vacuum_result* out);
/* The live rows in row order as wq_rec_row. *n is the live count and *ops_seen the store's op
 * counter; with *n > capacity nothing is written (WQ_E_CAPACITY), and `out` may be null with
 * capacity 0 to ask for the count. The store is not changed: no vacuum, and handles not yet drained
 * are not part of a snapshot. Two exports of one store give the same bytes. The _device form writes
 * to device memory (16-byte aligned). Both forms wait for the count. */
int wq_records_export(wq_router* h, wq_rec_row* out, size_t capacity, size_t* n, uint64_t* ops_seen);
int wq_records_export_device(wq_router* h, wq_rec_row* d_out, size_t capacity, size_t* n, uint64_t* ops_seen);
/* Builds a store from a snapshot. The store must have received no op and hold no row (else
 * WQ_E_INVALID); its region and table sizes may differ from the snapshot's source. A row is rejected
 * and counted when a region[d] is no multiple of that axis's region size, its index is outside
 * [-2^23, 2^23), the world is not packable or seq >= ops_seen. Accepted rows are stored in the given
 * order under their own seq; the table is recomputed from the region. Two accepted rows with the same
 * (world, region, uuid, ts_us, seq) refuse the whole import (WQ_E_INVALID, the store stays empty).
 * Afterwards the op counter is `ops_seen`, wq_records_totals is all zeros and rows_live == imported.
 * Synchronous. */
int wq_records_import(wq_router* h, const wq_rec_row* rows, size_t n, uint64_t ops_seen, wq_rec_import_result* out);
int wq_records_import_device(wq_router* h, const wq_rec_row* d_rows, size_t n, uint64_t ops_seen,
                             wq_rec_import_result* out);
/* clamp_region_coord (world_region.rs:93-110) on the host; WQ_E_INVALID for size 0 or a NaN. */
int wq_region_quantize(const double* coords, size_t n, uint16_t size, int64_t* out);
/* clamp_table_size (world_region.rs:112-129) on the host. */
int wq_table_quantize(const int64_t* region, size_t n, uint32_t table_size, int64_t* out);

/* ---- record dispatch: a tick's record frames to store ops and queries on the device ----
 * wq_ingest_dispatch_device lists the RecordCreate / RecordRead / RecordDelete frames of a tick
 * (WQ_CLS_DB, the database segment of side_src) and leaves the record path to the caller. The reference
 * handles them one message at a time (processing/record_create.rs:15-18, record_read.rs:18-41,
 * record_delete.rs:15-18: "@global" is ignored; database/client.rs:86-111 and :365-379: a record without
 * a position or with a world name the sanitizer refuses is dropped; utils/time.rs:6-16: the `after` of a
 * read) and records.RecordProcessor.process restates that as a Python loop over every record. Here one
 * call walks the listed frames' records where the frames lie and writes the arrays wq_records_apply_device
 * and wq_records_read_device take, with the table of runs that says in which order to issue them. Nothing
 * is read back until the counters and the run table. The host definition is ingest.records_dispatch_np.
 *
 * Input (wq_recdisp_in; device pointers unless stated)
 *   - frames / frame_offsets[n_frames + 1] / n_frame_bytes: the tick's raw frames as the decoder took them;
 *     msg / world / flags: the decoder's outputs, [n_frames] each.
 *   - db_src[n_db]: ascending frame indices; NULL means frames 0 .. n_db - 1.
 *   - now_us: the ts_us of every op. free_handles[n_free] (nullable with n_free 0) / handle_next: the k-th
 *     accepted create of the call gets free_handles[k] for k < n_free, else handle_next + (k - n_free); the
 *     caller updates its allocator from n_creates.
 *   - max_records: the caller's bound on the records the listed frames hold, < 2^32 - 64. Scratch is sized
 *     from it, never from a value read back. Every record owns a 4-byte slot of its frame's records vector,
 *     so n_frame_bytes / 4 always suffices. Records past the bound are not examined: overflow bit 3.
 * Frame classes (out->cls[j] for listed entry j, frame f = db_src[j])
 *   - WQ_RCLS_SKIP           flag bit 0 clear, flag bit 4 set (the message's world is "@global"), or an
 *                            instruction other than 8, 9, 11. Also a listed index >= n_frames.
 *   - WQ_RCLS_APPLY          instruction 8 (create) or 11 (delete). The message's own world plays no further
 *                            part; each record carries its own.
 *   - WQ_RCLS_READ           instruction 9 with a position (flag bit 1), a parameter that is absent (flag bit
 *                            2 clear) or parses, a world name the sanitizer accepts and a resolved world (flag
 *                            bit 5 and world < WQ_WORLD_GLOBAL). One query row.
 *   - WQ_RCLS_READ_DROPPED   instruction 9 without a position, or with a parameter that does not parse, or
 *                            with a world name the sanitizer refuses (dec_sanitize over msg.world_off / len
 *                            inside the frame tells "refused" from "unknown"). Checked in that order.
 *   - WQ_RCLS_READ_DEFERRED  instruction 9 that passes those checks but whose world did not resolve: the
 *                            host interns the name. Listed in defer with record WQ_RDEFER_READ.
 *   - Parameter: u64::from_str — an optional single '+', then one or more ASCII digits and nothing else,
 *     leading zeros allowed, the value below 2^64 — then chrono's range, ms / 1000 <= 8,210,298,412,799.
 *     q_after = ms * 1000; "no after" is INT64_MIN. The lane stops at the first byte that is no digit and
 *     once the significant digits exceed 20; a run of leading zeros is the only long walk, bounded by the
 *     frame. (records.parse_epoch_millis goes through Python's int(), which refuses very long digit
 *     strings; this definition parses digit by digit and follows time.rs.)
 * Records of an APPLY frame, in (frame, record index) order; the count is the vector's in the frame, never
 * msg.n_records
 *   - dropped and counted by reason: no position; a world name the sanitizer refuses ("@global" is refused
 *     with IsGlobalWorld); rec_pack_position fails under the open store's configuration (a NaN, a region
 *     index outside [-2^23, 2^23)).
 *   - deferred: the sanitized name is not in the handle's world table (wq_frames_set_worlds). Listed in
 *     defer as (frame, record index); the host interns the name and applies the record after the tick.
 *   - accepted: one wq_rec_op { kind, world, the position's bits as they lie, uuid_hi / uuid_lo (the
 *     big-endian halves of the uuid re-parsed from its text), ts_us = now_us, handle (create: from the
 *     allocator; delete: 0), reserved 0 }: byte for byte the rows RecordProcessor.process assembles.
 *     op_ref beside it holds the frame and record index, where the record's data and flex lie inside the
 *     frame and whether they are present (bits 0 and 1), so the caller copies the payload into its slab
 *     under the op's handle before the frame buffer is reused.
 * Runs: RecordProcessor.process's non-empty apply and read calls, in its order, each with the same rows
 *   - process keeps one batch of ops and one of reads. A barrier is a listed frame of class APPLY (kind
 *     apply) or READ / READ_DROPPED / READ_DEFERRED (kind read): it flushes the other kind's batch, whether or
 *     not it yields a row itself. An effective frame has at least one accepted op or is a READ: it joins its
 *     kind's batch, and starts a run when that batch is empty — no effective frame of its kind has come since
 *     the last barrier of the other kind.
 *   - Two consecutive runs may have the same kind (reads, a create frame without an accepted record, reads),
 *     and a barrier that yields nothing still ends the other kind's run (creates, a dropped read, a read: an
 *     apply run and a read run). The split of a read batch is observable, see "two queries of one read
 *     call" under the record store above.
 *   - runs[r] = { kind (WQ_RRUN_APPLY / WQ_RRUN_READ), the run's first frame, where its rows begin in ops
 *     and in q_* }; runs[n_runs] closes the table with WQ_RRUN_END, first_frame = n_frames and the totals.
 *     Rows are stable, so a run's rows are contiguous.
 *   - With no deferred entry the outcome equals RecordProcessor.process's. With deferred entries it is
 *     exact for every frame before first_deferred.
 * Output (wq_recdisp_out: device pointers, each nullable, at natural alignment)
 *   - cls[n_db]; q_src / q_world / q_pos (3 f64) / q_after (i64), [n_db] each: q_world, q_pos, q_after are
 *     the arrays wq_records_read_device takes; ops / op_ref[ops_capacity]; defer[defer_capacity]: (frame,
 *     record) ascending; runs[runs_capacity].
 *   - Rows below a capacity are exact; the counters and the closing run (when it fits) are always complete:
 *     overflow bit 0 ops, 1 defer, 2 runs, 3 max_records. A NULL array with capacity 0 makes a sizing call.
 *     Nothing is written outside [0, count) of each array; the inputs are never written.
 * Hostile input (never a fault): the arrays are the caller's and may disagree with the frames.
 *   - No byte is read outside frames[0 .. n_frame_bytes), frame_offsets[0 .. n_frames], db_src[0 .. n_db)
 *     and the n_frames-sized arrays; every access to a frame goes through the decoder's bounded reader.
 *   - error bit 0: a walk failed — frame offsets the decoder would refuse, a records vector, record table,
 *     uuid, parameter or world range that does not lie in the frame. Such a frame or record yields nothing
 *     (an APPLY frame keeps its class with no records, a read is READ_DROPPED) and a record counts in
 *     n_drop_walk. error bit 1: a db_src entry >= n_frames (SKIP) or not above its predecessor (processed
 *     in list order all the same).
 *   - Every loop is bounded by the frame's size or by max_records; nothing spins or waits on another lane.
 * Execution
 *   - Asynchronous on the handle's stream; nothing is read back. A frame pass (one lane per listed frame:
 *     class, parameter, the records vector), a scan of the record counts, a record pass (element-parallel
 *     over granules of 64 records on a grid-stride loop: every lane finds its frame by search and
 *     evaluates one record; wave ballots give the granule's flag words), scans of the granules' counts, the
 *     scan over the listed frames that carries rows and runs (a frame's own sum is computed from the granules'
 *     prefixes as the scan reads it), and a stable emit that walks the accepted records once more. No lane, wave or block owns a frame's records.
 *     Deterministic byte for byte: the only atomics are integer adds and ORs into the counters.
 *   - Scratch lives in the handle, grow-only: 57 bytes per listed frame and 40 bytes per 64 records of
 *     max_records. A steady-state call does no hipMalloc, and the call alternates freely with decode,
 *     dispatch, route, records apply / read, builder and pack on one handle.
 *   - WQ_E_INVALID, with nothing launched, for a null handle, in or out; a null required array with a
 *     non-zero size (frames, frame_offsets, msg, world, flags); no open record store (a multi-GPU handle has none);
 *     n_db >= 2^32 - 1 or n_frames >= 2^32 - 1; max_records >= 2^32 - 64; n_free > 0 without free_handles;
 *     an array given with capacity 0, or a capacity without its array (ops and op_ref share ops_capacity). */
#define WQ_RCLS_SKIP 0
#define WQ_RCLS_APPLY 1
#define WQ_RCLS_READ 2
#define WQ_RCLS_READ_DROPPED 3
#define WQ_RCLS_READ_DEFERRED 4
#define WQ_RCLS_COUNT 5

#define WQ_RRUN_END 0
#define WQ_RRUN_APPLY 1
#define WQ_RRUN_READ 2

#define WQ_RDEFER_READ 0xFFFFFFFFu   /* wq_recdisp_defer.record of a deferred read */

struct wq_decoded_msg;
typedef struct wq_recdisp_in {
    const uint8_t*  frames;          /* [n_frame_bytes] */
    const uint64_t* frame_offsets;   /* [n_frames + 1] */
    uint64_t        n_frames, n_frame_bytes;
    const struct wq_decoded_msg* msg; /* [n_frames] */
    const uint32_t* world;           /* [n_frames] */
    const uint8_t*  flags;           /* [n_frames] */
    const uint32_t* db_src;          /* [n_db] nullable: frames 0 .. n_db - 1 */
    uint64_t        n_db;
    int64_t         now_us;
    const uint32_t* free_handles;    /* [n_free] nullable with n_free 0 */
    uint32_t        n_free, handle_next;
    uint64_t        max_records;
} wq_recdisp_in;             /* 104 bytes */

typedef struct wq_rec_op_ref {
    uint32_t frame, record;          /* the frame index and the record's index in its vector */
    uint32_t data_off, data_len, flex_off, flex_len;  /* inside the frame; 0, 0 when absent */
    uint32_t bits;                   /* bit 0: data present, bit 1: flex present */
    uint32_t pad_;
} wq_rec_op_ref;             /* 32 bytes */

typedef struct wq_recdisp_defer { uint32_t frame, record; } wq_recdisp_defer;                      /* 8 bytes */
typedef struct wq_recdisp_run { uint32_t kind, first_frame, op_begin, q_begin; } wq_recdisp_run;   /* 16 bytes */

typedef struct wq_recdisp_out {      /* device pointers, each nullable */
    uint8_t*  cls;                   /* [n_db] WQ_RCLS_* */
    wq_rec_op* ops; wq_rec_op_ref* op_ref;                               /* [ops_capacity] */
    uint32_t* q_src; uint32_t* q_world; double* q_pos; int64_t* q_after; /* [n_db] query rows */
    wq_recdisp_defer* defer;         /* [defer_capacity] */
    wq_recdisp_run* runs;            /* [runs_capacity] runs[0 .. min(n_runs + 1, capacity)) */
    uint32_t ops_capacity, defer_capacity, runs_capacity, pad_;
} wq_recdisp_out;            /* 88 bytes */

typedef struct wq_recdisp_counters {
    uint64_t n_db;
    uint64_t n_skip, n_apply, n_read, n_read_dropped, n_read_deferred;   /* listed frames per WQ_RCLS_* */
    uint64_t n_records_total;        /* records the APPLY frames hold */
    uint64_t n_records;              /* of them examined: min(n_records_total, max_records) */
    uint64_t n_creates, n_deletes;   /* accepted */
    uint64_t n_drop_walk, n_drop_no_position, n_drop_world, n_drop_unpackable;  /* dropped, by reason */
    uint64_t n_deferred_records;     /* deferred reads: n_read_deferred */
    uint64_t n_runs;
    uint64_t first_deferred;         /* the frame index of the first deferred entry; n_frames when there is none */
    uint64_t overflow;               /* bits 0 - 3 above */
    uint64_t error;                  /* bits 0 and 1 above */
} wq_recdisp_counters;       /* 152 bytes */

int wq_records_dispatch_device(wq_router* h, const wq_recdisp_in* in, const wq_recdisp_out* out,
                               wq_recdisp_counters* d_counters /* nullable */);

/* ---- record payload slab: the created records' payloads kept in device memory ----
 * wq_records_dispatch_device leaves, per accepted create, an op with the caller's payload slot (`handle`) and
 * an op_ref that says where the record's data and flex lie inside its frame. records.DeviceRecordProcessor
 * reads both back and slices the frames on the host, one Python dict per record. Here one call copies the
 * payloads from the frames where they lie into an arena in device memory and writes one 64-byte entry per
 * handle. The memory is the caller's (it grows it); the view describes it. Nothing is read back. The host
 * definition is records.slab_store_np.
 *
 *   - Every op of kind WQ_RECORD_CREATE writes entries[op.handle]: uuid = the big-endian bytes of uuid_hi
 *     then uuid_lo (the uuid's 16 bytes as the decoder parsed them from the text), pos and world as the op
 *     holds them, bits 0 and 1 from op_ref.bits, bit 2 (position) and bit 31 (live) set, and data_len /
 *     flex_len. Its data lies at payload[off .. off + data_len) and its flex directly behind it. Ops of any
 *     other kind are skipped. A payload whose bit is clear has length 0 whatever op_ref's length says.
 *   - Placement: the u64 exclusive scan of data_len + flex_len over the ops in op order, starting at
 *     *d_cursor, a device word the call advances by the total. No padding between payloads.
 *   - All or nothing. With *d_cursor + total > n_payload_bytes (overflow bit 0) or a create whose handle is
 *     >= n_entries (overflow bit 1) no entry and no payload byte is written and the cursor stays; bytes_need
 *     is the arena size and entries_need the entry count that suffice. The caller grows and calls again.
 *   - Hostile references (never a fault). frame_offsets[n_frames] is taken as the size of d_frames. error
 *     bit 0: op_ref.frame >= n_frames, or that frame's offsets descend or pass frame_offsets[n_frames]: both
 *     payloads present as op_ref.bits says, and empty. Bit 1: the data range leaves its frame (off + len in
 *     u64): data empty. Bit 2: the same for flex. The handles of one call's creates are distinct, as the
 *     dispatch's allocator gives them; of two creates with one handle the entry is either's.
 *   - The copy runs over the arena's bytes [cursor, cursor + total) like wq_peer_pack_device's: a wave owns
 *     a 1 KiB-aligned tile of the arena and a lane one 16-byte store, so a 1 MiB flex spreads over the
 *     grid and empty payloads cost nothing. Only the first and last chunk of the range use narrower stores;
 *     no byte outside the range is written.
 *   - Asynchronous on the handle's stream. Scratch lives in the handle, grow-only (40 bytes per op): a
 *     steady-state call does no hipMalloc. entries and payload are 16-byte aligned.
 *   - WQ_E_INVALID, with nothing launched: a null handle, view, d_cursor; a multi-GPU handle; a null array
 *     with a non-zero size (d_ops, d_op_ref with n_ops; d_frame_offsets with n_frames; entries with n_entries;
 *     payload with n_payload_bytes); misaligned entries or payload; n_ops >= 2^31 or n_frames >= 2^32 - 1.
 * Freeing a dead handle is clearing bit 31 of its entry; wq_slab_compact_device (below) gets its bytes back. */
typedef struct wq_slab_entry {      /* 64 bytes, indexed by the store's `handle` */
    uint8_t  uuid[16];
    double   pos[3];
    uint32_t world;                 /* id into the table of wq_frames_set_worlds */
    uint32_t bits;                  /* bit 0 data present, 1 flex present, 2 position present, 31 live */
    uint64_t off;                   /* data at payload[off .. off+data_len), flex directly behind it */
    uint32_t data_len, flex_len;
} wq_slab_entry;
typedef struct wq_slab_view { wq_slab_entry* entries; uint64_t n_entries; uint8_t* payload; uint64_t n_payload_bytes; } wq_slab_view;
#define WQ_SLAB_DATA 1u
#define WQ_SLAB_FLEX 2u
#define WQ_SLAB_POSITION 4u
#define WQ_SLAB_LIVE 0x80000000u
typedef struct wq_slab_counters {
    uint64_t n_ops, n_creates;
    uint64_t bytes_stored;          /* the creates' payload bytes: what the cursor advances by */
    uint64_t bytes_need;            /* cursor + bytes_stored before the call (saturating): the arena size that suffices */
    uint64_t entries_need;          /* the largest create handle + 1; 0 without a create */
    uint64_t cursor;                /* *d_cursor after the call */
    uint32_t overflow;              /* bit 0: the arena, bit 1: the entries; nothing was written */
    uint32_t error;                 /* bits 0 - 2 above */
} wq_slab_counters;                 /* 56 bytes */
int wq_slab_store_device(wq_router* h, const wq_rec_op* d_ops, const wq_rec_op_ref* d_op_ref, size_t n_ops,
                         const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n_frames,
                         const wq_slab_view* view, uint64_t* d_cursor, wq_slab_counters* d_counters /* nullable */);

/* ---- slab compaction: a slab rewritten in its canonical form ----
 * The store appends and a free only clears a live bit, so an arena fills with bytes nothing refers to. This
 * call writes the slab `src` into the slab `dst` in one canonical form: the live payloads back to back in
 * handle order, every other entry zero. Into a second arena that is compaction (the caller swaps), into a
 * buffer the host reads back it is an export, from an uploaded file into a fresh slab it is a validated
 * import. Handles keep their numbers: the record store's rows hold them. The host definition is
 * records.slab_compact_np.
 *
 *   - Handle i < src->n_entries is kept when bit 31 (live) of its entry is set. A kept entry goes to
 *     dst->entries[i] with every field as it was except `off`; its data_len + flex_len bytes go to
 *     dst->payload[off' ..), data first and flex directly behind it.
 *   - Every other entry of dst is 64 zero bytes: dead handles, and handles at or above src->n_entries when
 *     dst is longer. All dst->n_entries entries are written, so two slabs that hold the same live records
 *     compact to the same bytes whatever their histories.
 *   - Placement: off' is the u64 exclusive scan of the kept entries' data_len + flex_len in ascending handle
 *     order, from 0, without padding. *d_dst_cursor becomes the total.
 *   - All or nothing. Overflow bit 0: the total exceeds dst->n_payload_bytes. Bit 1: the highest live handle
 *     + 1 exceeds dst->n_entries. After either no byte of dst is written and *d_dst_cursor stays; the
 *     counters' bytes_live and entries_need are the sizes that suffice. dst may have fewer entries than src
 *     (trailing dead handles are trimmed). A dst with n_payload_bytes == 0 and a null payload is the sizing
 *     call.
 *   - Hostile entries (never a fault). A live entry whose range [off, off + data_len + flex_len) leaves
 *     src->n_payload_bytes (checked in u64: an `off` near 2^64 does not wrap) stays live and keeps its
 *     presence bits, both lengths become 0 and error bit 0 is set: the reply builder's bit-5 rule. Two live
 *     entries that share or overlap a source range are each copied; that is no error. world and pos are
 *     carried as they are. A total past 2^64 - 1 saturates, which is an arena overflow.
 *   - No byte of dst->payload at or beyond the total is written, and no input is written.
 *   - The passes: flags and sizes over the entries as 16-byte chunks, four lanes per entry; one scan of
 *     (live, size); a one-lane decision; the entries, again four lanes each; the copy over the destination's
 *     bytes like wq_slab_store_device's, whose elements are the live entries alone, so a run of dead handles
 *     costs the copy nothing. Placement comes from the scan: the result is the same bytes every time.
 *   - Asynchronous on the handle's stream. Scratch lives in the handle, grow-only (40 bytes per source
 *     entry); nothing is read back.
 *   - WQ_E_INVALID, with nothing launched: a null handle, src, dst or d_dst_cursor; a multi-GPU handle; a null
 *     array with a non-zero size; entries, or dst's payload, that are not 16-byte aligned (src's arena is only
 *     read, at any alignment, as the reply builder reads it); n_entries >= 2^32 - 1 on either side; src and dst entry arrays that overlap, or payload arenas that overlap (the call is out of
 *     place). */
typedef struct wq_slab_compact_counters {
    uint64_t n_entries;             /* src->n_entries */
    uint64_t n_live;                /* kept entries */
    uint64_t bytes_live;            /* their payload bytes: the total, and the arena size that suffices */
    uint64_t entries_need;          /* the highest live handle + 1; 0 without a live entry */
    uint32_t overflow;              /* bit 0: the arena, bit 1: the entries; nothing was written */
    uint32_t error;                 /* bit 0 above */
} wq_slab_compact_counters;         /* 40 bytes */
int wq_slab_compact_device(wq_router* h, const wq_slab_view* src, const wq_slab_view* dst, uint64_t* d_dst_cursor,
                           wq_slab_compact_counters* d_counters /* nullable */);

/* ---- record replies: frames of messages that carry records, built on the device from the slab ----
 * wq_frames_build_device serializes flat messages. This call serializes messages whose `records` vector is a
 * row of a CSR of slab handles (what wq_records_read_device returns), with `entities` empty: the RecordReply
 * of record_read.rs:43-96. The message part is wq_frames_src under every rule it has there; the bytes are
 * wq_serialize_message's for a message whose records are the row's entries in row order. The host definition
 * is frames.build_record_frames_np.
 *   - rec->row_offsets[n_msgs + 1] / handles[n_handles]: the rows, read as the send side reads a CSR: row i is
 *     the part of [off[i], off[i + 1]) inside [0, n_handles), empty when it descends, and the rows together
 *     are walked for at most n_handles elements (error bit 6 for any of these).
 *   - rec->slab: read only. A handle >= n_entries or an entry whose live bit is clear is left out of the
 *     frame (bit 4). Data at payload[off, off + data_len) or flex at [off + data_len, off + data_len +
 *     flex_len) that leaves the arena is present and empty (bit 5). An entry's world id outside the table of
 *     wq_frames_set_worlds gives an empty name (bit 0). The same handle twice gives the record twice. `data`
 *     is not checked for UTF-8: it came through the decoder.
 *   - rec->world_bytes / world_off (u64[n_msgs]) / world_len (u32[n_msgs]) / n_world_bytes: optional; when
 *     given, message i's world name is world_bytes[world_off[i] .. + world_len[i]) and src->world is not
 *     read. A range that leaves world_bytes is an empty name (bit 0).
 *   - rec->flags bit 0, WQ_FRAMES_SKIP_EMPTY: a message left without a record is an empty frame of size 0
 *     (the reference returns before sending, record_read.rs:56-58). Frame i stays message i's.
 *   - src->sender_uuid NULL is the nil uuid. A frame above 2^30 bytes is empty (bit 3).
 *   - Capacity, sizing call (d_frames NULL with capacity 0: the arena is then not read), determinism,
 *     alignment and scratch are wq_frames_build_device's: asynchronous, nothing read back, byte-identical
 *     every time, a steady-state call does no hipMalloc (scratch: 28 bytes per handle, 36 per message).
 *     With every row empty and the flag clear the output is wq_frames_build_device's.
 *   - No lane owns a row or a payload: an element pass over the handles, a segmented scan (the shapes a row
 *     has seen and the residue its last record left), a place pass, prefix sums of sizes and kept counts, a
 *     row pass, the scan of the frame sizes and the 1 KiB-tile copy whose composer replays only the records
 *     that touch its 16-byte chunk.
 *   - WQ_E_INVALID: what wq_frames_build_device refuses (sender_uuid may be NULL; world may be NULL with
 *     world_bytes), a null rec, row_offsets NULL with n_msgs, handles NULL with n_handles, n_handles >=
 *     2^32 - 1, slab entries that are not 16-byte aligned (the arena is read at any alignment), world_off / world_len missing beside world_bytes, unknown flag bits. */
#define WQ_FRAMES_SKIP_EMPTY 1u
typedef struct wq_frames_rec_src {
    const uint32_t* row_offsets;     /* [n_msgs + 1] */
    const uint32_t* handles;         /* [n_handles] */
    uint64_t        n_handles;
    wq_slab_view    slab;            /* read only */
    const uint8_t*  world_bytes;     /* nullable */
    const uint64_t* world_off;       /* [n_msgs] */
    const uint32_t* world_len;       /* [n_msgs] */
    uint64_t        n_world_bytes;
    uint32_t        flags, pad_;
} wq_frames_rec_src;                 /* 96 bytes */
int wq_frames_build_records_device(wq_router* h, const wq_frames_src* src, const wq_frames_rec_src* rec, size_t n_msgs,
                                   uint8_t* d_frames, size_t capacity_bytes, uint64_t* d_frame_offsets,
                                   uint32_t* d_frame_size, wq_frames_counters* d_counters);

/* ---- health of asynchronous ticks ----
 * OR of wq_route_counters.error (error_bits) and of .overflow over every route / global call since
 * the previous wq_route_health on this handle; reading clears them (synchronises the stream). A
 * normal tick never writes them, so a caller that runs many _device ticks without reading their
 * counters checks the whole run here: error bit 4 = a bounded spin gave up (WQ_E_TIMEOUT), 2 =
 * more than 2^32-1 pairs in one tick, 8 = a tick ran on a table still missing an incremental
 * batch (wq_apply_ops_device), 16 = a device op batch held an invalid op and was not applied;
 * overflow = some tick's pairs exceeded its capacity. */
int wq_route_health(wq_router* h, uint32_t* error_bits, uint32_t* overflow);

/* ---- instrumentation ----
 * When enabled, every route launch is bracketed by HIP events on the launch stream;
 * wq_profile_read returns the summed kernel-only milliseconds and launch count (and resets). */
int wq_profile_enable(wq_router* h, int enable);
int wq_profile_read(wq_router* h, double* kernel_ms, uint64_t* launches);
/* The same, plus per-kernel time of the launches that ran the three-launch shape (count / tile scan /
 * emit: events between the kernels): phase_ms[0..2] summed over those `phased` launches. */
int wq_profile_read_phases(wq_router* h, double* kernel_ms, uint64_t* launches, double* phase_ms,
                           uint64_t* phased);
/* The shader clock in MHz right now (a short all-CU spin: s_memtime cycles over s_memrealtime wall
 * time), so a bench line can say what clock its timed region ran at. Synchronises the stream. */
int wq_probe_sclk(wq_router* h, double* mhz);

/* ---- test hook: keep only the low `bits` bits of the 64-bit cube hash (64 = normal).
 * Forces bucket collisions so the exact-compare fallback paths are exercised. */
int wq_debug_set_hash_bits(wq_router* h, int bits);
/* ---- tuning hook: record slots per cube at the next full build (default 8: load <= 1/8). More
 * slots = fewer displaced keys (fewer second probe rounds) for more HBM. */
int wq_debug_set_record_slack(wq_router* h, uint32_t slots_per_cube);
/* ---- test hook: how many op batches took the incremental update (wq_delta.hip), how many
 * tried it but fell back to the full rebuild (irregular keys, list space, record load), and how
 * many incremental batches had a cube go through the wave path (a list longer than 48 peers;
 * shorter lists are merged one lane per cube). */
int wq_debug_update_counts(wq_router* h, uint64_t* incremental, uint64_t* rebuild_fallbacks,
                           uint64_t* wave_batches);
/* ---- tuning hook: select a compiled route-kernel shape (messages per thread, expansion chunk);
 * 0 is the default. Results are identical for every shape. */
int wq_debug_set_route_config(wq_router* h, int cfg);
/* ---- test hook: the capacity of wq_frames_decode_device's long-string work list in entries (0: every
 * lane validates its long strings itself; negative: the default). Results are identical for every value. */
int wq_debug_set_ingest_list(wq_router* h, int64_t entries);
/* ---- tuning hook: the heavy-fan-out tick (count / scan / emit) in `chunks` pipelined chunks — the
 * chunks' counts on a side stream, each chunk's scan and emit on the launch stream as soon as its
 * count is done (0 = the default; 1 = one chunk). Applies to ticks of >= 2 chunks of at most 8,192
 * count tiles each. Results are identical for every value. */
int wq_debug_set_route_chunks(wq_router* h, int chunks);
/* ---- test hook: the handle's route-call counter (single-GPU handles). The single-launch tick tags
 * its look-back granules with this counter modulo 2^22 - 1, plus one, and zeroes them each time the
 * tags wrap; moving the counter lets a test place two long ticks one tag period apart without
 * running the four million ticks between them. Results are identical for every value. */
int wq_debug_set_route_calls(wq_router* h, uint64_t calls);
int wq_debug_route_calls(wq_router* h, uint64_t* calls);
/* The tick shape the next default-config tick takes (heavy_fanout = count / scan / emit) and
 * whether it is still chosen automatically (no hint set, or reset by a negative hint). */
int wq_debug_route_shape(wq_router* h, int* heavy_fanout, int* fanout_auto);
/* Number of route kernel configurations (valid cfg values are 0 .. n-1). */
int wq_debug_route_config_count(void);
/* Diagnostics: when d_stamps is non-null, the single-launch tick writes four s_memrealtime stamps
 * (100 MHz) per block — start, counted, prefix known, done — to d_stamps[4*block ..]. */
int wq_debug_set_timeline(wq_router* h, uint64_t* d_stamps);

#ifdef __cplusplus
}
#endif

#endif /* WQ_ROUTER_H */
