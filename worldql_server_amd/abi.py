"""Host-side constants and record layouts of the C ABI (include/wq_router.h).

Pure data: importing this module loads no native code.
"""
from __future__ import annotations

import ctypes

import numpy as np

WQ_OK = 0
WQ_E_INVALID = -1
WQ_E_OOM = -2
WQ_E_HIP = -3
WQ_E_RCCL = -4
WQ_E_CAPACITY = -5
WQ_E_NODEV = -6
WQ_E_TIMEOUT = -7

OP_SUBSCRIBE = 0    # AreaMap::add_subscription (area_map.rs:72-85)
OP_UNSUBSCRIBE = 1  # AreaMap::remove_subscription (area_map.rs:88-119)
OP_REMOVE_PEER = 2  # WorldMap::remove_peer (world_map.rs:41-61)

REPL_EXCEPT_SELF = 0     # Replication wire codes, WorldQLFB_generated.rs:176-188
REPL_INCLUDING_SELF = 1
REPL_ONLY_SELF = 2

WORLD_INVALID = 0xFFFFFFFF
WORLD_GLOBAL = 0xFFFFFFFE          # WQ_WORLD_GLOBAL: "@global" as wq_frames_decode_device reports it

MAX_PAIRS = 0xFFFFFFFF             # pairs per tick: the CSR offsets are u32 (error bit 2, WQ_E_CAPACITY beyond)
ROUTE_ERROR_PAIR_LIMIT = 2         # wq_route_counters.error bit 2
TICK_TAG_PERIOD = (1 << 22) - 1    # route calls after which the single-launch tick's granule tags repeat

# struct wq_op: 40 bytes; `key` aliases `pos` (union).
OP_DTYPE = np.dtype({
    "names": ["world", "peer", "kind", "key_is_raw", "pos", "key"],
    "formats": [np.uint32, np.uint32, np.uint8, np.uint8, (np.float64, 3), (np.int64, 3)],
    "offsets": [0, 4, 8, 9, 16, 16],
    "itemsize": 40,
})

# struct wq_route_counters: 24 bytes
COUNTERS_DTYPE = np.dtype([("n_pairs", np.uint64), ("n_candidates", np.uint64),
                           ("overflow", np.uint32), ("error", np.uint32)])

# struct wq_diff_counters: 24 bytes (wq_csr_diff_device)
DIFF_COUNTERS_DTYPE = np.dtype([("n_entered", np.uint64), ("n_left", np.uint64),
                                ("overflow", np.uint32), ("error", np.uint32)])
DIFF_OVERFLOW_ENTERED = 1  # wq_diff_counters.overflow bits
DIFF_OVERFLOW_LEFT = 2
DIFF_ERROR_ROWS = 1        # wq_diff_counters.error bit 0: a row was cut to the part inside bounds

# struct wq_budget_counters: 24 bytes (wq_peer_budget_device)
BUDGET_COUNTERS_DTYPE = np.dtype([("n_in", np.uint64), ("n_kept", np.uint64),
                                  ("rows_cut", np.uint32), ("error", np.uint32)])
BUDGET_ERROR_ROWS = 1      # wq_budget_counters.error bit 0: a row descended or reached past n_in
BUDGET_ERROR_MSG = 2       # bit 1: a message index was >= n_msgs

# struct wq_budget_bytes_counters: 40 bytes (wq_peer_budget_bytes_device); the error bits are the same
BUDGET_BYTES_COUNTERS_DTYPE = np.dtype([("n_in", np.uint64), ("n_kept", np.uint64), ("bytes_in", np.uint64),
                                        ("bytes_kept", np.uint64), ("rows_cut", np.uint32), ("error", np.uint32)])

# struct wq_rotate_counters: 64 bytes (wq_peer_rotate_device)
ROTATE_COUNTERS_DTYPE = np.dtype([("n_in", np.uint64), ("n_kept_in", np.uint64), ("n_chosen", np.uint64),
                                  ("n_out", np.uint64), ("bytes_chosen", np.uint64), ("bytes_out", np.uint64),
                                  ("rows_rotated", np.uint32), ("rows_behind", np.uint32), ("error", np.uint32),
                                  ("pad_", np.uint32)])
ROTATE_ERROR_ROWS = 1      # wq_rotate_counters.error bit 0: a row of either CSR descended or reached past its array
ROTATE_ERROR_MSG = 2       # bit 1: with sizes, a message index was >= n_msgs
ROTATE_ERROR_KEPT = 4      # bit 2: a kept element had no partner in its full row
ROTATE_CURSOR_START = 0xFFFFFFFF   # a new peer's cursor: the rotation starts at the row's beginning

# struct wq_pack_counters: 40 bytes (wq_peer_pack_device)
PACK_COUNTERS_DTYPE = np.dtype([("n_in", np.uint64), ("n_complete", np.uint64), ("bytes_need", np.uint64),
                                ("bytes_written", np.uint64), ("overflow", np.uint32), ("error", np.uint32)])
PACK_LEN_PREFIX = 1        # WQ_PACK_LEN_PREFIX: every frame is preceded by its size as a u32, little endian
PACK_ERROR_ROWS = 1        # wq_pack_counters.error bit 0: a row descended or reached past n_in
PACK_ERROR_MSG = 2         # bit 1: a message index was >= n_msgs
PACK_ERROR_FRAME = 4       # bit 2: a referenced frame's offsets descend, reach past n_frame_bytes or span >= 2^32


# struct wq_frames_counters: 40 bytes (wq_frames_build_device)
FRAMES_COUNTERS_DTYPE = np.dtype([("n_frames", np.uint64), ("n_complete", np.uint64), ("bytes_need", np.uint64),
                                  ("bytes_written", np.uint64), ("overflow", np.uint32), ("error", np.uint32)])
FRAME_MAX = 1 << 30          # the builder's limit: the host returns WQ_SER_TOO_LARGE above it
FRAMES_ERROR_WORLD = 1       # wq_frames_counters.error bit 0: a world id >= n_worlds
FRAMES_ERROR_PARAM = 2       # bit 1: a parameter range descends, reaches past n_param_bytes or spans >= 2^32
FRAMES_ERROR_FLEX = 4        # bit 2: the same for flex
FRAMES_ERROR_TOO_LARGE = 8   # bit 3: a frame above FRAME_MAX, left empty
FRAMES_HAS_POSITION, FRAMES_HAS_PARAMETER, FRAMES_HAS_FLEX = 1, 2, 4   # wq_frames_src.msg_flags bits


class FramesSrc(ctypes.Structure):  # struct wq_frames_src: device pointers
    _fields_ = [("instruction", ctypes.c_void_p), ("instruction_all", ctypes.c_uint8),
                ("replication", ctypes.c_void_p), ("replication_all", ctypes.c_uint8),
                ("sender_uuid", ctypes.c_void_p), ("world", ctypes.c_void_p), ("pos", ctypes.c_void_p),
                ("param", ctypes.c_void_p), ("param_offsets", ctypes.c_void_p), ("n_param_bytes", ctypes.c_uint64),
                ("flex", ctypes.c_void_p), ("flex_offsets", ctypes.c_void_p), ("n_flex_bytes", ctypes.c_uint64),
                ("msg_flags", ctypes.c_void_p)]


assert ctypes.sizeof(FramesSrc) == 112 and FRAMES_COUNTERS_DTYPE.itemsize == 40


# struct wq_ingest_counters: 64 bytes (wq_frames_decode_device)
INGEST_COUNTERS_DTYPE = np.dtype([("n_frames", np.uint64), ("n_ok", np.uint64), ("n_invalid", np.uint64),
                                  ("n_missing", np.uint64), ("n_bad_uuid", np.uint64),
                                  ("n_world_unresolved", np.uint64), ("n_sender_unknown", np.uint64),
                                  ("error", np.uint32), ("pad_", np.uint32)])
INGEST_ERROR_OFFSETS = 1     # wq_ingest_counters.error bit 0: a frame's offsets descend or reach past n_frame_bytes
INGEST_ERROR_HUGE = 2        # bit 1: a frame of 2^32 bytes or more
INGEST_NO_PEER = 0xFFFFFFFF  # wq_ingest_out.sender of a uuid the table lacks (processing.NO_PEER)
# wq_ingest_out.flags bits
INGEST_OK, INGEST_HAS_POSITION, INGEST_HAS_PARAMETER, INGEST_HAS_FLEX = 1, 2, 4, 8
INGEST_WORLD_GLOBAL, INGEST_WORLD_KNOWN, INGEST_SENDER_KNOWN = 16, 32, 64
INGEST_LANE_STRING = 256     # strings up to this many bytes are validated by the walking lane
INGEST_CHUNK = 16            # bytes one lane validates of a longer string


class IngestOut(ctypes.Structure):  # struct wq_ingest_out: device pointers, each nullable
    _fields_ = [(k, ctypes.c_void_p) for k in ("msg", "pos", "world", "sender", "repl", "instruction", "sender_uuid",
                                               "flex_range", "flags")]


assert ctypes.sizeof(IngestOut) == 72 and INGEST_COUNTERS_DTYPE.itemsize == 64

# ---- ingest dispatch (wq_ingest_dispatch_device) ----
# WQ_CLS_*: the class of a frame, in the order of wq_dispatch_counters' per-class counts
(CLS_BAD, CLS_HEARTBEAT, CLS_LOCAL, CLS_GLOBAL, CLS_BCAST, CLS_OP, CLS_DEFERRED, CLS_DB, CLS_OTHER,
 CLS_DROPPED) = range(10)
CLS_NAMES = ("bad", "heartbeat", "local", "global", "bcast", "op", "deferred", "db", "other", "dropped")
RUN_END, RUN_TABLE, RUN_READ = 0, 1, 2          # WQ_RUN_*: wq_dispatch_run.kind
DISPATCH_SIDE_LISTS = (CLS_HEARTBEAT, CLS_BCAST, CLS_DB, CLS_OTHER, CLS_DEFERRED)  # side_src's lists in order
DISPATCH_ERROR_DISAGREE = 1                     # wq_dispatch_counters.error bit 0: a flag and its value disagree
DISPATCH_OVERFLOW_RUNS = 1                      # wq_dispatch_counters.overflow bit 0: n_runs + 1 > runs_capacity
# struct wq_dispatch_run: 20 bytes
DISPATCH_RUN_DTYPE = np.dtype([("kind", np.uint32), ("first_frame", np.uint32), ("l_begin", np.uint32),
                               ("g_begin", np.uint32), ("op_begin", np.uint32)])
# struct wq_dispatch_counters: 168 bytes
DISPATCH_COUNTERS_DTYPE = np.dtype([("n_frames", np.uint64)] + [("n_" + k, np.uint64) for k in CLS_NAMES] +
                                   [("n_runs", np.uint64), ("side_begin", np.uint64, (6,)), ("first_deferred", np.uint64),
                                    ("overflow", np.uint64), ("error", np.uint64)])


class DispatchIn(ctypes.Structure):  # struct wq_dispatch_in: device pointers
    _fields_ = [(k, ctypes.c_void_p) for k in ("instruction", "flags", "world", "sender", "repl", "pos", "last_seen")] + \
               [("n_last_seen", ctypes.c_uint32), ("now", ctypes.c_uint32)]


DISPATCH_OUT_ARRAYS = ("cls", "l_src", "l_pos", "l_world", "l_sender", "l_repl", "g_src", "g_world", "g_sender", "g_repl",
                       "ops", "op_src", "side_src", "runs")


class DispatchOut(ctypes.Structure):  # struct wq_dispatch_out: device pointers, each nullable
    _fields_ = [(k, ctypes.c_void_p) for k in DISPATCH_OUT_ARRAYS] + [("runs_capacity", ctypes.c_uint32),
                                                                      ("pad_", ctypes.c_uint32)]


assert ctypes.sizeof(DispatchIn) == 64 and ctypes.sizeof(DispatchOut) == 120
assert DISPATCH_RUN_DTYPE.itemsize == 20 and DISPATCH_COUNTERS_DTYPE.itemsize == 168

# ---- ingest joins (wq_ingest_join_device, wq_ingest_drop_peers_device) ----
JOIN_ERROR_DISAGREE, JOIN_ERROR_NO_TABLE = 1, 2                 # wq_join_counters.error bits 0 and 1
JOIN_OVERFLOW_IDS, JOIN_OVERFLOW_TABLE, JOIN_OVERFLOW_OUT = 1, 2, 4   # wq_join_counters.overflow bits 0 - 2
# struct wq_join_counters: 80 bytes
JOIN_COUNTERS_DTYPE = np.dtype([(k, np.uint64) for k in ("n_frames", "n_candidates", "n_joined", "n_patched", "n_free_used",
                                                         "id_next", "n_table", "first_join", "overflow", "error")])


class JoinIn(ctypes.Structure):  # struct wq_join_in: device pointers; flags and sender are patched in place
    _fields_ = [(k, ctypes.c_void_p) for k in ("instruction", "world", "sender_uuid", "flags", "sender", "free_ids")] + \
               [(k, ctypes.c_uint32) for k in ("n_free", "id_next", "id_limit", "pad_")]


class JoinOut(ctypes.Structure):  # struct wq_join_out: device pointers, each nullable
    _fields_ = [(k, ctypes.c_void_p) for k in ("j_uuid", "j_id", "j_frame")] + \
               [("joined_capacity", ctypes.c_uint32), ("pad_", ctypes.c_uint32)]


assert ctypes.sizeof(JoinIn) == 64 and ctypes.sizeof(JoinOut) == 32 and JOIN_COUNTERS_DTYPE.itemsize == 80


# ---- ingest leaves (wq_ingest_leave_device, wq_remove_peers_device) ----
SEEN_NEVER = 0xFFFFFFFF                                         # WQ_SEEN_NEVER: last_seen of an id not seen yet
LEAVE_LISTED, LEAVE_STALE = 1, 2                                # wq_leave_out.l_reason bits 0 and 1
LEAVE_ERROR_NO_TABLE, LEAVE_ERROR_ID_RANGE = 2, 4               # wq_leave_counters.error bits 1 and 2
LEAVE_OVERFLOW_OUT, LEAVE_OVERFLOW_FREE = 1, 2                  # wq_leave_counters.overflow bits 0 and 1
LEAVE_TEXT = 36                                                 # bytes of a uuid's text in l_param
# struct wq_leave_counters: 80 bytes
LEAVE_COUNTERS_DTYPE = np.dtype([(k, np.uint64) for k in ("n_table_before", "n_listed", "n_listed_found", "n_stale", "n_left",
                                                          "n_stamped", "n_table", "n_free", "overflow", "error")])


class LeaveIn(ctypes.Structure):  # struct wq_leave_in: device pointers and host values; last_seen is written
    _fields_ = [(k, ctypes.c_void_p) for k in ("last_seen", "pinned_bits", "leave_ids", "free_ids")] + \
               [(k, ctypes.c_uint32) for k in ("n_ids", "now", "max_age", "n_leave", "n_free", "pad_")]


class LeaveOut(ctypes.Structure):  # struct wq_leave_out: device pointers, each nullable
    _fields_ = [(k, ctypes.c_void_p) for k in ("l_uuid", "l_id", "l_reason", "l_param", "l_param_offsets", "gone_bits",
                                               "free_out")] + \
               [("leave_capacity", ctypes.c_uint32), ("free_capacity", ctypes.c_uint32)]


assert ctypes.sizeof(LeaveIn) == 56 and ctypes.sizeof(LeaveOut) == 64 and LEAVE_COUNTERS_DTYPE.itemsize == 80


# ---- record dispatch (wq_records_dispatch_device) ----
# WQ_RCLS_*: the class of a listed frame, in the order of wq_recdisp_counters' per-class counts
RCLS_SKIP, RCLS_APPLY, RCLS_READ, RCLS_READ_DROPPED, RCLS_READ_DEFERRED = range(5)
RCLS_NAMES = ("skip", "apply", "read", "read_dropped", "read_deferred")
RRUN_END, RRUN_APPLY, RRUN_READ = 0, 1, 2      # WQ_RRUN_*: wq_recdisp_run.kind
RDEFER_READ = 0xFFFFFFFF                       # WQ_RDEFER_READ: wq_recdisp_defer.record of a deferred read
RECDISP_ERROR_WALK, RECDISP_ERROR_LIST = 1, 2  # wq_recdisp_counters.error bits 0 and 1
RECDISP_OVERFLOW_OPS, RECDISP_OVERFLOW_DEFER, RECDISP_OVERFLOW_RUNS, RECDISP_OVERFLOW_RECORDS = 1, 2, 4, 8
RECDISP_MAX_RECORDS = 0xFFFFFFC0               # max_records stays below
# struct wq_rec_op_ref: 32 bytes; wq_recdisp_defer: 8; wq_recdisp_run: 16
REC_OP_REF_DTYPE = np.dtype([(k, np.uint32) for k in ("frame", "record", "data_off", "data_len", "flex_off", "flex_len",
                                                      "bits", "pad_")])
RECDISP_DEFER_DTYPE = np.dtype([("frame", np.uint32), ("record", np.uint32)])
RECDISP_RUN_DTYPE = np.dtype([(k, np.uint32) for k in ("kind", "first_frame", "op_begin", "q_begin")])
# struct wq_recdisp_counters: 152 bytes
RECDISP_COUNTERS_DTYPE = np.dtype([(k, np.uint64) for k in
                                   ("n_db",) + tuple("n_" + c for c in RCLS_NAMES) +
                                   ("n_records_total", "n_records", "n_creates", "n_deletes", "n_drop_walk",
                                    "n_drop_no_position", "n_drop_world", "n_drop_unpackable", "n_deferred_records",
                                    "n_runs", "first_deferred", "overflow", "error")])


class RecDispatchIn(ctypes.Structure):  # struct wq_recdisp_in: device pointers
    _fields_ = [("frames", ctypes.c_void_p), ("frame_offsets", ctypes.c_void_p), ("n_frames", ctypes.c_uint64),
                ("n_frame_bytes", ctypes.c_uint64), ("msg", ctypes.c_void_p), ("world", ctypes.c_void_p),
                ("flags", ctypes.c_void_p), ("db_src", ctypes.c_void_p), ("n_db", ctypes.c_uint64),
                ("now_us", ctypes.c_int64), ("free_handles", ctypes.c_void_p), ("n_free", ctypes.c_uint32),
                ("handle_next", ctypes.c_uint32), ("max_records", ctypes.c_uint64)]


RECDISP_OUT_ARRAYS = ("cls", "ops", "op_ref", "q_src", "q_world", "q_pos", "q_after", "defer", "runs")


class RecDispatchOut(ctypes.Structure):  # struct wq_recdisp_out: device pointers, each nullable
    _fields_ = [(k, ctypes.c_void_p) for k in RECDISP_OUT_ARRAYS] + \
               [(k, ctypes.c_uint32) for k in ("ops_capacity", "defer_capacity", "runs_capacity", "pad_")]


assert ctypes.sizeof(RecDispatchIn) == 104 and ctypes.sizeof(RecDispatchOut) == 88
assert REC_OP_REF_DTYPE.itemsize == 32 and RECDISP_DEFER_DTYPE.itemsize == 8 and RECDISP_RUN_DTYPE.itemsize == 16
assert RECDISP_COUNTERS_DTYPE.itemsize == 152


# ---- record payload slab (wq_slab_store_device) ----
# struct wq_slab_entry: 64 bytes, indexed by the store's handle
SLAB_ENTRY_DTYPE = np.dtype([("uuid", np.uint8, (16,)), ("pos", np.float64, (3,)), ("world", np.uint32), ("bits", np.uint32),
                             ("off", np.uint64), ("data_len", np.uint32), ("flex_len", np.uint32)])
SLAB_DATA, SLAB_FLEX, SLAB_POSITION, SLAB_LIVE = 1, 2, 4, 0x80000000   # wq_slab_entry.bits
SLAB_OVERFLOW_ARENA, SLAB_OVERFLOW_ENTRIES = 1, 2                      # wq_slab_counters.overflow
SLAB_ERROR_FRAME, SLAB_ERROR_DATA, SLAB_ERROR_FLEX = 1, 2, 4           # wq_slab_counters.error
SLAB_MAX_OPS = 1 << 31
# struct wq_slab_counters: 56 bytes
SLAB_COUNTERS_DTYPE = np.dtype([(k, np.uint64) for k in ("n_ops", "n_creates", "bytes_stored", "bytes_need", "entries_need",
                                                         "cursor")] + [("overflow", np.uint32), ("error", np.uint32)])


class SlabView(ctypes.Structure):  # struct wq_slab_view: the caller's device memory
    _fields_ = [("entries", ctypes.c_void_p), ("n_entries", ctypes.c_uint64), ("payload", ctypes.c_void_p),
                ("n_payload_bytes", ctypes.c_uint64)]


assert SLAB_ENTRY_DTYPE.itemsize == 64 and SLAB_COUNTERS_DTYPE.itemsize == 56 and ctypes.sizeof(SlabView) == 32

# ---- slab compaction (wq_slab_compact_device) ----
# struct wq_slab_compact_counters: 40 bytes; overflow takes SLAB_OVERFLOW_ARENA / SLAB_OVERFLOW_ENTRIES
SLAB_COMPACT_COUNTERS_DTYPE = np.dtype([(k, np.uint64) for k in ("n_entries", "n_live", "bytes_live", "entries_need")] +
                                       [("overflow", np.uint32), ("error", np.uint32)])
SLAB_COMPACT_ERROR_RANGE = 1          # wq_slab_compact_counters.error: a live entry whose range leaves the source arena
SLAB_COMPACT_MAX_ENTRIES = 0xFFFFFFFF
assert SLAB_COMPACT_COUNTERS_DTYPE.itemsize == 40


FRAMES_ERROR_HANDLE, FRAMES_ERROR_ARENA, FRAMES_ERROR_ROWS = 16, 32, 64   # wq_frames_build_records_device: bits 4 - 6
FRAMES_SKIP_EMPTY = 1                                                   # WQ_FRAMES_SKIP_EMPTY


class FramesRecSrc(ctypes.Structure):  # struct wq_frames_rec_src: device pointers
    _fields_ = [("row_offsets", ctypes.c_void_p), ("handles", ctypes.c_void_p), ("n_handles", ctypes.c_uint64),
                ("slab", SlabView), ("world_bytes", ctypes.c_void_p), ("world_off", ctypes.c_void_p),
                ("world_len", ctypes.c_void_p), ("n_world_bytes", ctypes.c_uint64), ("flags", ctypes.c_uint32),
                ("pad_", ctypes.c_uint32)]


assert ctypes.sizeof(FramesRecSrc) == 96


# ---- tick sends (wq_tick_sends_device) ----
SEND_UNIT_ROWS = 0xFFFFFFFF        # WQ_SEND_UNIT_ROWS: wq_send_region.off_at of a region whose row r is element r
SEND_NO_SRC = 0xFFFFFFFF           # WQ_SEND_NO_SRC: wq_send_region.src_at of a region whose row r is frame r
SENDS_ERROR_ROWS, SENDS_ERROR_FRAME = 1, 2   # wq_tick_sends_counters.error bits 0 and 1
# struct wq_send_region: 32 bytes, a HOST array
SEND_REGION_DTYPE = np.dtype([(k, np.uint32) for k in ("off_at", "peers_at", "n_rows", "capacity", "src_at", "frame_base",
                                                       "src_sel", "pad_")])
# struct wq_tick_sends_counters: 64 bytes
TICK_SENDS_COUNTERS_DTYPE = np.dtype([(k, np.uint64) for k in ("n_regions", "n_elems", "n_covered", "n_kept", "n_drop_peer",
                                                               "n_drop_frame")] +
                                     [("error", np.uint32), ("pad_", np.uint32), ("reserved_", np.uint64)])


class TickSendsIn(ctypes.Structure):  # struct wq_tick_sends_in: `regions` is a HOST array, the others device pointers
    _fields_ = [("regions", ctypes.c_void_p), ("d_offsets", ctypes.c_void_p), ("n_offsets", ctypes.c_size_t),
                ("d_peers", ctypes.c_void_p), ("n_pairs", ctypes.c_size_t), ("d_src", ctypes.c_void_p * 2),
                ("n_src", ctypes.c_size_t * 2), ("d_connected", ctypes.c_void_p), ("n_regions", ctypes.c_uint32),
                ("n_peers", ctypes.c_uint32), ("n_frames", ctypes.c_uint32), ("pad_", ctypes.c_uint32)]


assert SEND_REGION_DTYPE.itemsize == 32 and TICK_SENDS_COUNTERS_DTYPE.itemsize == 64 and ctypes.sizeof(TickSendsIn) == 96


def send_region(off_at=SEND_UNIT_ROWS, peers_at=0, n_rows=0, capacity=0, src_at=SEND_NO_SRC, frame_base=0, src_sel=0, pad_=0):
    """One wq_send_region as a tuple in SEND_REGION_DTYPE's field order."""
    return (off_at, peers_at, n_rows, capacity, src_at, frame_base, src_sel, pad_)


class ExportFilter(ctypes.Structure):  # struct wq_export_filter; `peers` is a HOST array
    _fields_ = [("world", ctypes.c_uint32), ("n_peers", ctypes.c_uint32), ("peers", ctypes.c_void_p)]


def make_op(world: int, peer: int, kind: int, pos=None, key=None) -> np.void:
    """One wq_op record; give `pos` (Vector3, quantised) or `key` (raw CubeArea)."""
    o = np.zeros((), dtype=OP_DTYPE)
    o["world"] = world
    o["peer"] = peer
    o["kind"] = kind
    if key is not None:
        o["key_is_raw"] = 1
        o["key"] = np.asarray(key, dtype=np.int64)
    else:
        o["key_is_raw"] = 0
        o["pos"] = np.asarray(pos if pos is not None else (0.0, 0.0, 0.0), dtype=np.float64)
    return o[()]


def ops_array(world, peer, kind, pos=None, key=None) -> np.ndarray:
    """Vectorised op construction (all arguments broadcast over n ops)."""
    world = np.asarray(world, dtype=np.uint32)
    n = world.shape[0]
    ops = np.zeros(n, dtype=OP_DTYPE)
    ops["world"] = world
    ops["peer"] = np.asarray(peer, dtype=np.uint32)
    ops["kind"] = np.asarray(kind, dtype=np.uint8)
    if key is not None:
        ops["key_is_raw"] = 1
        ops["key"] = np.asarray(key, dtype=np.int64).reshape(n, 3)
    else:
        ops["pos"] = np.asarray(pos, dtype=np.float64).reshape(n, 3)
    return ops


def concat_ops(parts) -> np.ndarray:
    """np.concatenate drops the union layout of OP_DTYPE; join the raw 40-byte records instead."""
    return np.concatenate([np.ascontiguousarray(p, dtype=OP_DTYPE).view(np.uint8) for p in parts]).view(OP_DTYPE)


# ---- multi-GPU (include/wq_router.h, "cube-hash ownership") ----
MAX_SHARDS = 64
RCCL_ID_BYTES = 128  # WQ_RCCL_ID_BYTES
SHARD_ALL = 0xFFFFFFFF  # owner of a REMOVE_PEER op

# struct wq_owner_view (wq_sharded_route_owner_device): device pointers + counts + source segments
class OwnerView(ctypes.Structure):
    _fields_ = [("recs", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("peers", ctypes.c_void_p),
                ("n_recs", ctypes.c_uint64), ("n_pairs", ctypes.c_uint64), ("seg", ctypes.c_uint32 * (MAX_SHARDS + 1))]


SLOT_WORDS = 5  # WQ_SLOT_WORDS


class OwnerSlotView(ctypes.Structure):  # struct wq_owner_slot_view
    _fields_ = [("slots", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("peers", ctypes.c_void_p),
                ("send_perm", ctypes.c_void_p), ("n_slots", ctypes.c_uint64),
                ("n_pairs", ctypes.c_uint64), ("seg", ctypes.c_uint32 * (MAX_SHARDS + 1)),
                ("send_seg", ctypes.c_uint32 * (MAX_SHARDS + 1))]


# wq_router_create_multi_mode layouts
MULTI_CUBE_HASH = 0
MULTI_REPLICATE = 1


class MsgSlice(ctypes.Structure):  # struct wq_msg_slice: one device's ingested messages
    _fields_ = [("d_pos", ctypes.c_void_p), ("d_keys", ctypes.c_void_p), ("d_world", ctypes.c_void_p),
                ("d_sender", ctypes.c_void_p), ("d_repl", ctypes.c_void_p), ("n_msgs", ctypes.c_uint64)]


class SliceView(ctypes.Structure):  # struct wq_slice_view: one device's CSR, left on that device
    _fields_ = [("device", ctypes.c_int32), ("pad_", ctypes.c_uint32), ("n_msgs", ctypes.c_uint64),
                ("n_pairs", ctypes.c_uint64), ("offsets", ctypes.c_void_p), ("peers", ctypes.c_void_p),
                ("msgs", ctypes.c_void_p)]


# struct wq_msg_rec: 40 bytes on the wire between GPUs
REC_POS = 1  # wq_msg_rec.flags: key holds the f64 position bits (radius filter on)
MSG_REC_DTYPE = np.dtype({
    "names": ["key", "world", "sender", "msg", "repl", "flags"],
    "formats": [(np.int64, 3), np.uint32, np.uint32, np.uint32, np.uint8, np.uint8],
    "offsets": [0, 24, 28, 32, 36, 37],
    "itemsize": 40,
})
