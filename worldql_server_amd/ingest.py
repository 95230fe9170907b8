"""Ingest, the host side (include/wq_router.h, "ingest"; kernels: csrc/wq_decode.hip).

`decode_frames_np` is the definition of what wq_frames_decode_device writes: the host decoder
(codec.decode_packed, the restatement of Message::deserialize) under the call's rules for frame
offsets, then per message what processing.py does one event at a time — "@global", the world-name
sanitizer (world_names.py), the world table, the sender table — plus the flags, the counters and
`flex_range`, which comes from a small walk of its own over a frame the decoder has already accepted.
`Router.set_ingest_peers` / `Router.decode_frames_device` (router.py) are the device call's bindings,
`abi.IngestOut` and `abi.INGEST_COUNTERS_DTYPE` its structs. `IngestTick` keeps the device arrays of a
tick and hands them to `Router.route_device` with nothing read back in between.

`dispatch_np` is the definition of what wq_ingest_dispatch_device writes (csrc/wq_dispatch.hip): the
classes of the header's table, the compact rows, the side lists and the run table, in plain Python over
the dict `decode_frames_np` returns. `IngestTick.dispatch` enqueues the device call on the decode's
arrays and `IngestTick.process` reads the counters and the run table, the tick's one read-back, and
issues the runs in order.

`join_peers_np` and `drop_peers_np` are the definitions of wq_ingest_join_device and
wq_ingest_drop_peers_device (csrc/wq_join.hip): between decode and dispatch the subscribes of senders the
table lacks get their peer ids by the caller's allocator state, sender and flags are patched in place and
the handle's sender table takes the joins; the drop is the leave side. `IngestTick.join` enqueues the call
on the decode's arrays with its counters beside the dispatch's, so `process` still has one read-back.

`records_dispatch_np` is the definition of what wq_records_dispatch_device writes (csrc/wq_recdispatch.hip):
the record frames of the dispatch's database list walked record by record into the ops and query rows of
the record store, the deferred list and the run table that reproduces records.RecordProcessor.process's
calls. `IngestTick.records_dispatch` enqueues the device call on the arrays decode() and dispatch() left;
records.DeviceRecordProcessor issues its runs on a GpuRecordStore.
"""
from __future__ import annotations

import struct
import uuid as _uuid

import numpy as np

from . import abi, codec, records as rec
from .abi import (INGEST_COUNTERS_DTYPE, INGEST_ERROR_HUGE as ERROR_HUGE, INGEST_ERROR_OFFSETS as ERROR_OFFSETS,  # noqa: F401
                  INGEST_HAS_FLEX as HAS_FLEX, INGEST_HAS_PARAMETER as HAS_PARAMETER,
                  INGEST_HAS_POSITION as HAS_POSITION, INGEST_NO_PEER as NO_PEER, INGEST_OK as OK,
                  INGEST_SENDER_KNOWN as SENDER_KNOWN, INGEST_WORLD_GLOBAL as WORLD_IS_GLOBAL,
                  INGEST_WORLD_KNOWN as WORLD_KNOWN, IngestOut)
from .world_names import GLOBAL_WORLD, SanitizeError, sanitize_world_name

OUT_FIELDS = ("msg", "pos", "world", "sender", "repl", "instruction", "sender_uuid", "flex_range", "flags")
VT_FLEX = 20  # Message.flex's vtable slot (WorldQLFB_generated.rs:947)


def uuid_rows(uuids) -> np.ndarray:
    """u8[n, 16] of a list of uuid.UUID / 16-byte strings, or of an array of 16 n bytes."""
    if isinstance(uuids, np.ndarray):
        return np.ascontiguousarray(uuids, dtype=np.uint8).reshape(-1, 16)
    rows = [u.bytes if isinstance(u, _uuid.UUID) else bytes(u) for u in uuids]
    if any(len(r) != 16 for r in rows):
        raise ValueError("uuids: 16 bytes each")
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 16).copy()


def flex_range_of(frame) -> tuple:
    """(offset, length, present) of Message.flex inside a frame the decoder accepted, (0, 0, False) when
    the field is absent: root table -> vtable -> slot 20 -> the vector's length word."""
    b = bytes(frame)
    root = struct.unpack_from("<I", b, 0)[0]
    vt = root - struct.unpack_from("<i", b, root)[0]
    if struct.unpack_from("<H", b, vt)[0] <= VT_FLEX:
        return 0, 0, False
    slot = struct.unpack_from("<H", b, vt + VT_FLEX)[0]
    if slot == 0:
        return 0, 0, False
    at = root + slot
    vec = at + struct.unpack_from("<I", b, at)[0]
    return vec + 4, struct.unpack_from("<I", b, vec)[0], True


def world_ids(world_names) -> dict:
    """Table name (bytes) -> the lowest id that holds it."""
    ids: dict = {}
    for w, name in enumerate(world_names or []):
        ids.setdefault(name if isinstance(name, (bytes, bytearray)) else name.encode("utf-8"), w)
    return ids


def resolve_world(name: bytes, ids: dict):
    """(world id, flag bits) of a decoded world name."""
    text = name.decode("utf-8")  # the verifier has accepted it
    if text == GLOBAL_WORLD:
        return abi.WORLD_GLOBAL, WORLD_IS_GLOBAL
    try:
        w = ids.get(sanitize_world_name(text).encode("utf-8"))
    except SanitizeError:
        w = None
    return (abi.WORLD_INVALID, 0) if w is None else (w, WORLD_KNOWN)


def decode_frames_np(data, offsets, world_names, peer_uuids, peer_ids=None, n_frame_bytes=None, n_threads=0):
    """The definition of wq_frames_decode_device: a dict of msg (codec.DECODED_DTYPE[n]), pos f64[n, 3],
    world u32[n], sender u32[n], repl, instruction, flags u8[n], sender_uuid u8[n, 16], flex_range
    u32[n, 2] and counters (a dict of abi.INGEST_COUNTERS_DTYPE's fields).

    Frame i is data[offsets[i] .. offsets[i + 1]). An offset is suspect when it lies past n_frame_bytes
    (default len(data)) or stands in a descending pair; a frame with a suspect offset (its own pair
    descends or reaches past the end, or a neighbour's does at the offset they share) is InvalidFlatbuffer
    with error bit 0, a frame of 2^32 bytes or more with bit 1; every other frame is what
    codec.decode_packed makes of it. world_names is the table of
    Router.set_worlds, peer_uuids / peer_ids that of Router.set_ingest_peers."""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    n = max(len(offsets) - 1, 0)
    nb = len(data) if n_frame_bytes is None else int(n_frame_bytes)
    error = 0
    good = np.ones(n, bool)
    off = [int(v) for v in offsets]
    # an offset is suspect when it lies past the buffer or stands in a descending pair (either side may be
    # the wrong one); a frame with a suspect offset cannot be told from its neighbours
    suspect = [off[j] > nb or (j > 0 and off[j - 1] > off[j]) or (j < n and off[j] > off[j + 1]) for j in range(n + 1)] \
        if n else []
    for i in range(n):
        if suspect[i] or suspect[i + 1]:
            error |= ERROR_OFFSETS
            good[i] = False
        elif off[i + 1] - off[i] >= 1 << 32:
            error |= ERROR_HUGE
            good[i] = False
    msg = np.zeros(n, dtype=codec.DECODED_DTYPE)
    if good.all():
        if n:
            msg[:] = codec.decode_packed(data, offsets, n_threads)
    else:
        msg["status"] = codec.DEC_INVALID_FLATBUFFER
        keep = np.flatnonzero(good)
        d, o = codec.pack_frames([data[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in keep])
        if len(keep):
            msg[keep] = codec.decode_packed(d, o, n_threads)

    ids = world_ids(world_names)
    peers = {}
    rows = uuid_rows(peer_uuids if peer_uuids is not None else [])
    pid = np.arange(len(rows), dtype=np.uint32) if peer_ids is None else np.asarray(peer_ids, dtype=np.uint32)
    for k, r in enumerate(rows):
        key = r.tobytes()
        if key in peers:
            raise ValueError("peer_uuids: a uuid occurs twice")
        peers[key] = int(pid[k])

    out = dict(msg=msg, pos=np.zeros((n, 3), np.float64), world=np.full(n, abi.WORLD_INVALID, np.uint32),
               sender=np.full(n, NO_PEER, np.uint32), repl=np.zeros(n, np.uint8), instruction=np.zeros(n, np.uint8),
               sender_uuid=np.zeros((n, 16), np.uint8), flex_range=np.zeros((n, 2), np.uint32), flags=np.zeros(n, np.uint8))
    cnt = {k: 0 for k in INGEST_COUNTERS_DTYPE.names if k != "pad_"}
    cnt["n_frames"], cnt["error"] = n, error
    by_status = ("n_ok", "n_invalid", "n_missing", "n_bad_uuid")
    for i in range(n):
        m = msg[i]
        cnt[by_status[int(m["status"])]] += 1
        if m["status"] != codec.DEC_OK:
            continue
        a = int(offsets[i])
        frame = data[a:int(offsets[i + 1])]
        flags = OK | (HAS_POSITION if m["has_position"] else 0) | (HAS_PARAMETER if m["has_parameter"] else 0)
        f_off, f_len, has_flex = flex_range_of(frame)
        flags |= HAS_FLEX if has_flex else 0
        w0 = int(m["world_off"])
        world, bits = resolve_world(frame[w0:w0 + int(m["world_len"])].tobytes(), ids)
        flags |= bits
        cnt["n_world_unresolved"] += bits == 0
        sender = peers.get(m["sender_uuid"].tobytes())
        flags |= SENDER_KNOWN if sender is not None else 0
        cnt["n_sender_unknown"] += sender is None
        out["pos"][i] = m["position"]   # the bits as they lie: numpy copies f64 without touching NaNs
        out["world"][i], out["sender"][i] = world, NO_PEER if sender is None else sender
        out["repl"][i], out["instruction"][i] = m["replication"], m["instruction"]
        out["sender_uuid"][i] = m["sender_uuid"]
        out["flex_range"][i] = (f_off, f_len)
        out["flags"][i] = flags
    out["counters"] = cnt
    return out


DISPATCH_ROWS = ("cls", "l_src", "l_pos", "l_world", "l_sender", "l_repl", "g_src", "g_world", "g_sender", "g_repl",
                 "ops", "op_src", "side_src")
_INS_HEARTBEAT, _INS_SUBSCRIBE, _INS_UNSUBSCRIBE, _INS_GLOBAL, _INS_LOCAL = 0, 4, 5, 6, 7
_INS_DB = (8, 9, 11)   # RecordCreate, RecordRead, RecordDelete


def classify_frame(ins: int, flags: int, world: int, sender: int):
    """(class, error bits) of one decoded frame: the table of include/wq_router.h, "ingest dispatch"."""
    if not flags & OK:
        return abi.CLS_BAD, 0
    at_global = bool(flags & WORLD_IS_GLOBAL)
    err = 0
    if bool(flags & WORLD_KNOWN) != (world < abi.WORLD_GLOBAL) or at_global != (world == abi.WORLD_GLOBAL) or \
            bool(flags & SENDER_KNOWN) != (sender != NO_PEER):
        err = abi.DISPATCH_ERROR_DISAGREE
    has_pos = bool(flags & HAS_POSITION)
    world_ok = bool(flags & WORLD_KNOWN) and world < abi.WORLD_GLOBAL
    sender_ok = bool(flags & SENDER_KNOWN) and sender != NO_PEER
    if ins == _INS_HEARTBEAT:
        cls = abi.CLS_HEARTBEAT
    elif ins == _INS_LOCAL:        # local_message.rs:17-56
        cls = abi.CLS_LOCAL if not at_global and has_pos and world_ok else abi.CLS_DROPPED
    elif ins == _INS_GLOBAL:       # global_message.rs:18-54
        cls = abi.CLS_BCAST if at_global else abi.CLS_GLOBAL if world_ok else abi.CLS_DROPPED
    elif ins == _INS_SUBSCRIBE:    # area_subscribe.rs:17-46; an unresolved world or sender is a join
        cls = abi.CLS_DROPPED if at_global or not has_pos else abi.CLS_OP if world_ok and sender_ok else abi.CLS_DEFERRED
    elif ins == _INS_UNSUBSCRIBE:  # area_unsubscribe.rs; a peer without an id holds nothing
        cls = abi.CLS_OP if not at_global and has_pos and world_ok and sender_ok else abi.CLS_DROPPED
    elif ins in _INS_DB:
        cls = abi.CLS_DB
    else:
        cls = abi.CLS_OTHER
    return cls, err


def dispatch_np(decoded, runs_capacity=None, last_seen=None, now=0):
    """The definition of wq_ingest_dispatch_device over the dict decode_frames_np returns (instruction,
    flags, world, sender, repl, pos): a dict of cls u8[n], the LocalMessage rows l_src / l_pos (f64[k, 3],
    the bits copied) / l_world / l_sender / l_repl, the GlobalMessage rows g_*, ops (abi.OP_DTYPE) /
    op_src, side_src (heartbeat | "@global" broadcast | database | other | deferred), runs
    (abi.DISPATCH_RUN_DTYPE: the first min(n_runs + 1, runs_capacity) entries, the closing one included;
    runs_capacity None: n_runs + 1), counters (a dict of abi.DISPATCH_COUNTERS_DTYPE's fields) and
    last_seen (a stamped copy of the argument, or None)."""
    ins_a, flags_a = np.asarray(decoded["instruction"], np.uint8), np.asarray(decoded["flags"], np.uint8)
    world_a, sender_a = np.asarray(decoded["world"], np.uint32), np.asarray(decoded["sender"], np.uint32)
    repl_a = np.asarray(decoded["repl"], np.uint8)
    pos_a = np.ascontiguousarray(decoded["pos"], np.float64).reshape(-1, 3).view(np.uint64)   # bits, not values
    n = len(ins_a)
    seen = None if last_seen is None else np.array(last_seen, dtype=np.uint32, copy=True)
    cls = np.zeros(n, np.uint8)
    rows = {c: [] for c in range(len(abi.CLS_NAMES))}
    runs, error, prev = [], 0, abi.RUN_END
    for i in range(n):
        c, e = classify_frame(int(ins_a[i]), int(flags_a[i]), int(world_a[i]), int(sender_a[i]))
        cls[i] = c
        error |= e
        kind = abi.RUN_TABLE if c == abi.CLS_OP else abi.RUN_READ if c in (abi.CLS_LOCAL, abi.CLS_GLOBAL) else abi.RUN_END
        if kind != abi.RUN_END and kind != prev:   # a run: a maximal stretch of effective frames of one kind
            runs.append((kind, i, len(rows[abi.CLS_LOCAL]), len(rows[abi.CLS_GLOBAL]), len(rows[abi.CLS_OP])))
            prev = kind
        rows[c].append(i)
    runs.append((abi.RUN_END, n, len(rows[abi.CLS_LOCAL]), len(rows[abi.CLS_GLOBAL]), len(rows[abi.CLS_OP])))
    n_runs = len(runs) - 1

    def row_sender(idx):
        known = (flags_a[idx] & SENDER_KNOWN).astype(bool) & (sender_a[idx] != NO_PEER)
        return np.where(known, sender_a[idx], np.uint32(NO_PEER)).astype(np.uint32)

    ix = {c: np.array(v, dtype=np.int64) for c, v in rows.items()}
    li, gi, oi = ix[abi.CLS_LOCAL], ix[abi.CLS_GLOBAL], ix[abi.CLS_OP]
    ops = np.zeros(len(oi), dtype=abi.OP_DTYPE)
    ops["world"], ops["peer"] = world_a[oi], sender_a[oi]
    ops["kind"] = np.where(ins_a[oi] == _INS_SUBSCRIBE, abi.OP_SUBSCRIBE, abi.OP_UNSUBSCRIBE)
    ops["key"] = pos_a[oi].view(np.int64)
    hb = ix[abi.CLS_HEARTBEAT]
    if seen is not None and len(hb):
        s = row_sender(hb)
        seen[s[s < len(seen)]] = now
    side = [ix[c] for c in abi.DISPATCH_SIDE_LISTS]
    cap = n_runs + 1 if runs_capacity is None else int(runs_capacity)
    cnt = {"n_frames": n, "n_runs": n_runs}
    cnt.update({"n_" + k: len(ix[c]) for c, k in enumerate(abi.CLS_NAMES)})
    cnt["side_begin"] = [int(v) for v in np.concatenate([[0], np.cumsum([len(v) for v in side])])]
    cnt["first_deferred"] = int(ix[abi.CLS_DEFERRED][0]) if len(ix[abi.CLS_DEFERRED]) else n
    cnt["overflow"] = abi.DISPATCH_OVERFLOW_RUNS if n_runs + 1 > cap else 0
    cnt["error"] = error
    u32 = lambda a: np.asarray(a, dtype=np.uint32)  # noqa: E731
    return dict(cls=cls, l_src=u32(li), l_pos=pos_a[li].view(np.float64), l_world=world_a[li], l_sender=row_sender(li),
                l_repl=repl_a[li], g_src=u32(gi), g_world=world_a[gi], g_sender=row_sender(gi), g_repl=repl_a[gi],
                ops=ops, op_src=u32(oi), side_src=u32(np.concatenate(side)) if n else u32([]),
                runs=np.array(runs[:min(n_runs + 1, cap)], dtype=abi.DISPATCH_RUN_DTYPE).reshape(-1),
                counters=cnt, last_seen=seen)


def dispatch_counters(raw) -> dict:
    """abi.DISPATCH_COUNTERS_DTYPE bytes as dispatch_np's counters dict."""
    c = np.asarray(raw).view(np.uint8)[:abi.DISPATCH_COUNTERS_DTYPE.itemsize].view(abi.DISPATCH_COUNTERS_DTYPE)[0]
    return {k: [int(v) for v in c[k]] if k == "side_begin" else int(c[k]) for k in abi.DISPATCH_COUNTERS_DTYPE.names}


# ---- ingest joins: new senders get their ids between decode and dispatch (wq_ingest_join_device) ----
def _table_dict(table_uuids, table_ids):
    rows = uuid_rows(table_uuids if table_uuids is not None else [])
    ids = np.arange(len(rows), dtype=np.uint32) if table_ids is None else np.asarray(table_ids, dtype=np.uint32)
    return {r.tobytes(): int(i) for r, i in zip(rows, ids)}


def _table_arrays(table: dict):
    keys = sorted(table)   # bytes compare as the big-endian 128-bit keys do
    u = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(-1, 16).copy() if keys else np.zeros((0, 16), np.uint8)
    return u, np.array([table[k] for k in keys], dtype=np.uint32)


def join_peers_np(decoded, table_uuids, table_ids, free_ids, id_next, id_limit, capacity, joined_capacity=None):
    """The definition of wq_ingest_join_device: a plain loop over the frames of the dict decode_frames_np
    returns (instruction, flags, world, sender, sender_uuid). A frame classify_frame calls CLS_DEFERRED
    whose world resolved is a candidate; the first candidate of a uuid is its join and takes the next id
    (free_ids in order, then id_next upwards; a "candidate" whose uuid the table already holds is none and
    sets error bit 0); from that frame on, every decoded frame of the uuid whose
    sender is not known gets the id and the SENDER_KNOWN bit. table_uuids / table_ids: the sender table
    (ids None: the index); capacity: its reserved room (None: no reserved table, the call is a no-op with
    error bit 1); joined_capacity None: the j_* arrays are not given. Returns a dict of sender, flags
    (patched copies), j_uuid u8[k, 16], j_id, j_frame u32[k], table (uuids ascending, ids) and counters (a
    dict of abi.JOIN_COUNTERS_DTYPE's fields). With an overflow bit set nothing changes and j_* are empty."""
    ins_a, flags_a = np.asarray(decoded["instruction"], np.uint8), np.array(decoded["flags"], np.uint8, copy=True)
    world_a, sender_a = np.asarray(decoded["world"], np.uint32), np.array(decoded["sender"], np.uint32, copy=True)
    uuid_a = np.ascontiguousarray(decoded["sender_uuid"], np.uint8).reshape(-1, 16)
    n = len(ins_a)
    free = [int(v) for v in (free_ids if free_ids is not None else [])]
    table = _table_dict(table_uuids, table_ids)
    empty = dict(j_uuid=np.zeros((0, 16), np.uint8), j_id=np.zeros(0, np.uint32), j_frame=np.zeros(0, np.uint32))
    cnt = {k: 0 for k in abi.JOIN_COUNTERS_DTYPE.names}
    cnt.update(n_frames=n, id_next=int(id_next), first_join=n)
    if capacity is None:
        cnt["error"] = abi.JOIN_ERROR_NO_TABLE
        return dict(sender=sender_a, flags=flags_a, table=_table_arrays(table), counters=cnt, **empty)
    joined: dict = {}            # uuid bytes -> id, in join order
    j_frame, patched, error, n_cand = [], [], 0, 0
    for i in range(n):
        f, w, s = int(flags_a[i]), int(world_a[i]), int(sender_a[i])
        cls, e = classify_frame(int(ins_a[i]), f, w, s)
        error |= e
        if cls == abi.CLS_BAD or (f & SENDER_KNOWN and s != NO_PEER):
            continue
        u = uuid_a[i].tobytes()
        if cls == abi.CLS_DEFERRED and f & WORLD_KNOWN and w < abi.WORLD_GLOBAL:
            if u in table:          # the flags and the table disagree: no candidate, the frame is the host's
                error |= abi.JOIN_ERROR_DISAGREE
                continue
            n_cand += 1
            if u not in joined:
                k = len(joined)
                joined[u] = free[k] if k < len(free) else int(id_next) + (k - len(free))
                j_frame.append(i)
        if u in joined:
            patched.append(i)
    k = len(joined)
    overflow = (abi.JOIN_OVERFLOW_IDS if k > len(free) + (int(id_limit) - int(id_next)) else 0) | \
               (abi.JOIN_OVERFLOW_TABLE if len(table) + k > int(capacity) else 0) | \
               (abi.JOIN_OVERFLOW_OUT if joined_capacity is not None and k > int(joined_capacity) else 0)
    cnt.update(n_candidates=n_cand, n_joined=k, overflow=overflow, error=error, n_table=len(table))
    if overflow:
        return dict(sender=sender_a, flags=flags_a, table=_table_arrays(table), counters=cnt, **empty)
    for i in patched:
        sender_a[i] = joined[uuid_a[i].tobytes()]
        flags_a[i] |= SENDER_KNOWN
    table.update(joined)
    used = min(k, len(free))
    cnt.update(n_patched=len(patched), n_free_used=used, id_next=int(id_next) + k - used, n_table=len(table),
               first_join=j_frame[0] if k else n)
    return dict(sender=sender_a, flags=flags_a, table=_table_arrays(table), counters=cnt,
                j_uuid=np.frombuffer(b"".join(joined), dtype=np.uint8).reshape(-1, 16).copy() if k else empty["j_uuid"],
                j_id=np.array(list(joined.values()), dtype=np.uint32), j_frame=np.array(j_frame, dtype=np.uint32))


def drop_peers_np(table_uuids, table_ids, ids, reserved=True):
    """The definition of wq_ingest_drop_peers_device: the table without the entries whose id is listed, and
    the counters (n_frames: the ids given, n_patched: the entries removed, n_table: what is left)."""
    table = _table_dict(table_uuids, table_ids)
    ids = [int(v) for v in ids]
    cnt = {k: 0 for k in abi.JOIN_COUNTERS_DTYPE.names}
    cnt.update(n_frames=len(ids), first_join=len(ids))
    if not reserved:
        cnt["error"] = abi.JOIN_ERROR_NO_TABLE
        return dict(table=_table_arrays(table), counters=cnt)
    gone = set(ids)
    kept = {u: i for u, i in table.items() if i not in gone}
    cnt.update(n_patched=len(table) - len(kept), n_table=len(kept))
    return dict(table=_table_arrays(kept), counters=cnt)


def join_counters(raw) -> dict:
    """abi.JOIN_COUNTERS_DTYPE bytes as join_peers_np's counters dict."""
    c = np.asarray(raw).view(np.uint8)[:abi.JOIN_COUNTERS_DTYPE.itemsize].view(abi.JOIN_COUNTERS_DTYPE)[0]
    return {k: int(c[k]) for k in abi.JOIN_COUNTERS_DTYPE.names}


# ---- ingest leaves: stale and disconnected senders leave (wq_ingest_leave_device) ----
def id_bits(ids, n_ids: int) -> np.ndarray:
    """The u32 bitmap of ceil(n_ids / 32) words with the bits of `ids` set: pinned_bits, gone_bits."""
    bits = np.zeros((int(n_ids) + 31) // 32, np.uint32)
    for i in ids:
        bits[int(i) >> 5] |= np.uint32(1 << (int(i) & 31))
    return bits


def leave_peers_np(table_uuids, table_ids, last_seen, now, max_age, pinned, leave_ids, free, leave_capacity, free_capacity,
                   reserved=True):
    """The definition of wq_ingest_leave_device: a plain loop over the sender table (uuids ascending, ids),
    one entry at a time. last_seen: the u32 stamps, one per id (n_ids of them); pinned: a u32 bitmap as
    id_bits makes it, or None; leave_ids: the listed disconnects; free: the free list in pop order;
    leave_capacity / free_capacity None: the l_* arrays / free_out are not given. An entry with id < n_ids
    leaves when its id is listed (reason bit 0) or its stamp is stale (bit 1): not pinned, not SEEN_NEVER,
    now > stamp and now - stamp > max_age. An entry that stays and carries SEEN_NEVER is stamped `now`; a
    leaver's stamp goes back to SEEN_NEVER. Returns a dict of l_uuid u8[k, 16], l_id u32[k], l_reason u8[k],
    l_param u8[36 k], l_param_offsets u64[k + 1], gone_bits, free_out (the leavers' ids in reverse leave
    order, then free), last_seen (a copy), table (uuids, ids) and counters (abi.LEAVE_COUNTERS_DTYPE's
    fields). With an overflow bit set or without a reserved table nothing changes, the rows and free_out are
    empty and gone_bits is zero."""
    rows = uuid_rows(table_uuids if table_uuids is not None else [])
    ids = np.arange(len(rows), dtype=np.uint32) if table_ids is None else np.asarray(table_ids, dtype=np.uint32)
    seen = np.array(last_seen, np.uint32, copy=True).reshape(-1)
    n_ids, now, max_age = len(seen), int(now), int(max_age)
    if not 0 <= now < abi.SEEN_NEVER:
        raise ValueError("now must be below SEEN_NEVER")
    listed = {int(v) for v in (leave_ids if leave_ids is not None else [])}
    n_listed = len(leave_ids) if leave_ids is not None else 0
    free = [int(v) for v in (free if free is not None else [])]
    pin = None if pinned is None else np.asarray(pinned, np.uint32)
    cnt = {k: 0 for k in abi.LEAVE_COUNTERS_DTYPE.names}
    cnt.update(n_listed=n_listed, n_free=len(free))
    empty = dict(l_uuid=np.zeros((0, 16), np.uint8), l_id=np.zeros(0, np.uint32), l_reason=np.zeros(0, np.uint8),
                 l_param=np.zeros(0, np.uint8), l_param_offsets=np.zeros(0, np.uint64), gone_bits=id_bits([], n_ids),
                 free_out=np.zeros(0, np.uint32))
    table = (rows.copy(), ids.copy())
    if not reserved:
        cnt["error"] = abi.LEAVE_ERROR_NO_TABLE
        return dict(last_seen=seen, table=table, counters=cnt, **empty)
    leavers, reasons, stamp_now, error, n_found, n_stale = [], [], [], 0, 0, 0
    for e in range(len(rows)):
        i = int(ids[e])
        if i >= n_ids:
            error |= abi.LEAVE_ERROR_ID_RANGE
            continue
        stamp = int(seen[i])
        is_pinned = pin is not None and (int(pin[i >> 5]) >> (i & 31)) & 1
        reason = abi.LEAVE_LISTED if i in listed else 0
        if not is_pinned and stamp != abi.SEEN_NEVER and now > stamp and now - stamp > max_age:
            reason |= abi.LEAVE_STALE
        n_found += bool(reason & abi.LEAVE_LISTED)
        n_stale += bool(reason & abi.LEAVE_STALE)
        if reason:
            leavers.append(e)
            reasons.append(reason)
        elif stamp == abi.SEEN_NEVER:
            stamp_now.append(i)
    k = len(leavers)
    overflow = (abi.LEAVE_OVERFLOW_OUT if leave_capacity is not None and k > int(leave_capacity) else 0) | \
               (abi.LEAVE_OVERFLOW_FREE if free_capacity is not None and len(free) + k > int(free_capacity) else 0)
    cnt.update(n_table_before=len(rows), n_listed_found=n_found, n_stale=n_stale, n_left=k, n_table=len(rows), overflow=overflow,
               error=error)
    if overflow:
        return dict(last_seen=seen, table=table, counters=cnt, **empty)
    l_id = ids[leavers].astype(np.uint32)
    for i in stamp_now:
        seen[i] = now
    for i in l_id:
        seen[int(i)] = abi.SEEN_NEVER
    keep = np.ones(len(rows), bool)
    keep[leavers] = False
    text = "".join(str(_uuid.UUID(bytes=rows[e].tobytes())) for e in leavers).encode()
    cnt.update(n_stamped=len(stamp_now), n_table=len(rows) - k, n_free=len(free) + k)
    return dict(l_uuid=rows[leavers].reshape(-1, 16).copy(), l_id=l_id, l_reason=np.array(reasons, np.uint8),
                l_param=np.frombuffer(text, np.uint8).copy(),
                l_param_offsets=np.arange(k + 1, dtype=np.uint64) * np.uint64(abi.LEAVE_TEXT),
                gone_bits=id_bits(l_id, n_ids), free_out=np.array([int(i) for i in l_id[::-1]] + free, np.uint32),
                last_seen=seen, table=(rows[keep].copy(), ids[keep].copy()), counters=cnt)


def leave_counters(raw) -> dict:
    """abi.LEAVE_COUNTERS_DTYPE bytes as leave_peers_np's counters dict."""
    c = np.asarray(raw).view(np.uint8)[:abi.LEAVE_COUNTERS_DTYPE.itemsize].view(abi.LEAVE_COUNTERS_DTYPE)[0]
    return {k: int(c[k]) for k in abi.LEAVE_COUNTERS_DTYPE.names}


# ---- the record dispatch: the record frames of a tick to store ops and queries (wq_records_dispatch_device) ----
_VT_RECORDS = 14                                              # Message.records' vtable slot
_VT_REC_UUID, _VT_REC_POS, _VT_REC_WORLD, _VT_REC_DATA, _VT_REC_FLEX = 4, 6, 8, 10, 12   # Record's slots
_INS_CREATE, _INS_READ, _INS_DELETE = 8, 9, 11
NO_AFTER = -(1 << 63)
_MAX_SECONDS = 8_210_298_412_799                              # chrono's last second


class _WalkError(Exception):
    """The bounded reader refused an access (decode_ops.hpp DecV::fail)."""


class _Reader:
    """decode_ops.hpp's DecV over one frame: every access aligned and inside b[0 .. n), or _WalkError."""

    def __init__(self, b: bytes):
        self.b, self.n, self.apparent, self.tables, self.depth = b, len(b), 0, 0, 0

    def aligned(self, pos, a):
        if pos % a:
            raise _WalkError

    def range(self, pos, size):
        self.apparent += size
        if pos + size > self.n or self.apparent > 1 << 31:
            raise _WalkError

    def u32_at(self, pos):
        self.aligned(pos, 4)
        self.range(pos, 4)
        return struct.unpack_from("<I", self.b, pos)[0]

    def u16_at(self, pos):
        self.aligned(pos, 2)
        self.range(pos, 2)
        return struct.unpack_from("<H", self.b, pos)[0]

    def follow(self, pos):
        return pos + self.u32_at(pos)

    def vec_range(self, pos, elem):
        n = self.u32_at(pos)
        self.aligned(pos + 4, elem)
        self.range(pos + 4, n * elem)
        return pos + 4, n

    def visit_table(self, pos):
        self.tables += 1
        so = self.u32_at(pos)
        so -= (so >> 31) << 32          # as i32
        if so > pos:
            raise _WalkError
        vt = pos - so
        if vt >= self.n:
            raise _WalkError
        vl = self.u16_at(vt)
        self.aligned(vt + vl, 2)
        self.range(vt, vl)
        self.depth += 1
        return pos, vt, vl

    def field(self, t, voff):
        pos, vt, vl = t
        fo = self.u16_at(vt + voff) if voff < vl else 0
        return pos + fo if fo else 0

    def field_bytes(self, t, voff):
        """(offset, length) of a byte vector or a string, None when absent."""
        fp = self.field(t, voff)
        if not fp:
            return None
        vp = self.follow(fp)
        self.aligned(vp, 4)
        return self.vec_range(vp, 1)

    def field_vec3(self, t, voff):
        fp = self.field(t, voff)
        if fp:
            self.range(fp, 24)
        return fp or None


def parse_after(s: bytes):
    """utils/time.rs:6-16 digit by digit: u64::from_str (an optional '+', digits only, below 2^64), then
    chrono's range. Microseconds, or None when it does not parse."""
    i = 1 if s[:1] == b"+" else 0
    if i == len(s):
        return None
    v = 0
    for c in s[i:]:
        if not 0x30 <= c <= 0x39:
            return None
        v = v * 10 + (c - 0x30)
        if v >= 1 << 64:
            return None
    return None if v // 1000 > _MAX_SECONDS else v * 1000


def parse_uuid_text(s: bytes):
    """uuid 0.8.2 Uuid::parse_str as the decoder restates it: 32 hex digits, the hyphenated form, or that
    behind "urn:uuid:". The value, or None."""
    if len(s) == 45 and s[:9] == b"urn:uuid:":
        s = s[9:]
    elif len(s) not in (32, 36):
        return None
    if len(s) == 36:
        if any(s[k] != 0x2D for k in (8, 13, 18, 23)):
            return None
        s = s[:8] + s[9:13] + s[14:18] + s[19:23] + s[24:]
    if len(s) != 32 or any(c not in b"0123456789abcdefABCDEF" for c in s):
        return None
    return int(s, 16)


def _sanitized(name: bytes):
    """The sanitized name as bytes, None when the sanitizer refuses it (bytes that are no UTF-8 hold a
    character outside its set)."""
    try:
        return sanitize_world_name(name.decode("utf-8")).encode("utf-8")
    except (SanitizeError, UnicodeDecodeError):
        return None


def _frame_bytes(data, off, f, n, nb):
    """Frame f's bytes under decode_frames_np's rules for offsets, None when they are refused."""
    a, b = off[f], off[f + 1]
    if a > b or b > nb or (f > 0 and off[f - 1] > a) or (f + 1 < n and b > off[f + 2]) or b - a >= 1 << 32:
        return None
    return data[a:b].tobytes()


def _record(rd: _Reader, vec, r, ids, sizes):
    """(status, fields) of record r of the vector at vec: "walk", "no_position", "world", "unpackable",
    "defer" or "accept" (csrc/recdispatch_ops.hpp rd_record)."""
    try:
        t = rd.visit_table(rd.follow(vec + 4 * r))
        uuid = rd.field_bytes(t, _VT_REC_UUID)
        at = rd.field_vec3(t, _VT_REC_POS)
        world = rd.field_bytes(t, _VT_REC_WORLD)
        data = rd.field_bytes(t, _VT_REC_DATA)
        flex = rd.field_bytes(t, _VT_REC_FLEX)
        if uuid is None or world is None:
            raise _WalkError
        u = parse_uuid_text(rd.b[uuid[0]:uuid[0] + uuid[1]])
        if u is None:
            raise _WalkError
    except _WalkError:
        return "walk", None
    if at is None:
        return "no_position", None
    name = _sanitized(rd.b[world[0]:world[0] + world[1]])
    if name is None:
        return "world", None
    w = ids.get(name)
    if w is None:
        return "defer", None
    bits = struct.unpack_from("<3Q", rd.b, at)
    if not rec.position_packable(sizes, w, struct.unpack_from("<3d", rd.b, at)):
        return "unpackable", None
    ref = (data or (0, 0)) + (flex or (0, 0)) + ((1 if data else 0) | (2 if flex else 0),)
    return "accept", (w, bits, u >> 64, u & ((1 << 64) - 1), ref)


def records_dispatch_np(frames, offsets, decoded, db_src, store_sizes, world_names, now_us, free_handles=None,
                        handle_next=0, ops_capacity=None, defer_capacity=None, runs_capacity=None, max_records=None,
                        n_frame_bytes=None):
    """The definition of wq_records_dispatch_device: the header's frame rules, record rules and runs in plain
    Python over the raw frames, the dict decode_frames_np returns (msg, world, flags) and the dispatch's
    database list (db_src None: every frame). The host decoder reports only a frame's record count, so the
    records are walked here with a bounded reader that restates the device's. store_sizes: the open
    store's three region sizes; world_names: the table of Router.set_worlds.

    Returns a dict of cls u8[n_db], ops (records.REC_OP_DTYPE) / op_ref (abi.REC_OP_REF_DTYPE), cut at
    ops_capacity, the query rows q_src / q_world / q_pos (f64[k, 3], the bits copied) / q_after, defer
    (abi.RECDISP_DEFER_DTYPE, cut at defer_capacity), runs (abi.RECDISP_RUN_DTYPE: the first min(n_runs + 1,
    runs_capacity) entries, the closing one included) and counters (abi.RECDISP_COUNTERS_DTYPE's fields).
    A capacity of None holds everything; max_records None examines every record."""
    data = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    off = [int(v) for v in np.asarray(offsets, dtype=np.uint64).reshape(-1)]
    n = max(len(off) - 1, 0)
    nb = len(data) if n_frame_bytes is None else int(n_frame_bytes)
    msg, world_a, flags_a = decoded["msg"], np.asarray(decoded["world"], np.uint32), np.asarray(decoded["flags"], np.uint8)
    src = list(range(n)) if db_src is None else [int(v) for v in db_src]
    ids = world_ids(world_names)
    sizes = tuple(int(s) for s in store_sizes)
    free = [] if free_handles is None else [int(v) for v in free_handles]
    limit = None if max_records is None else int(max_records)
    cnt = {k: 0 for k in abi.RECDISP_COUNTERS_DTYPE.names}
    cls = np.zeros(len(src), np.uint8)
    ops, refs, q, defer, runs = [], [], [], [], []
    error, open_run, examined, creates, first_def = 0, abi.RRUN_END, 0, 0, None
    for j, f in enumerate(src):
        if j and src[j - 1] >= f:
            error |= abi.RECDISP_ERROR_LIST
        if f >= n:
            error |= abi.RECDISP_ERROR_LIST
            continue
        b = _frame_bytes(data, off, f, n, nb)
        if b is None:
            error |= abi.RECDISP_ERROR_WALK
            continue
        flags, m = int(flags_a[f]), msg[f]
        ins = int(m["instruction"])
        if not flags & OK or flags & WORLD_IS_GLOBAL or ins not in _INS_DB:
            continue
        rd = _Reader(b)
        n_ops, n_q = len(ops), len(q)
        if ins != _INS_READ:   # record_create.rs / record_delete.rs: every record carries its own world
            c, kind = abi.RCLS_APPLY, abi.RRUN_APPLY
            try:
                fp = rd.field(rd.visit_table(rd.follow(0)), _VT_RECORDS)
                vec, count = (0, 0)
                if fp:
                    vp = rd.follow(fp)
                    rd.aligned(vp, 4)
                    vec, count = rd.vec_range(vp, 4)
            except _WalkError:
                error |= abi.RECDISP_ERROR_WALK
                vec, count = 0, 0
            cnt["n_records_total"] += count
            for r in range(count):
                if limit is not None and examined >= limit:
                    break
                examined += 1
                status, got = _record(_Reader(b), vec, r, ids, sizes)
                if status == "accept":
                    w, bits, hi, lo, ref = got
                    handle = 0
                    if ins == _INS_CREATE:
                        handle = free[creates] if creates < len(free) else (handle_next + creates - len(free)) & 0xFFFFFFFF
                        creates += 1
                    ops.append((rec.CREATE if ins == _INS_CREATE else rec.DELETE, w, bits, hi, lo, now_us, handle))
                    refs.append((f, r) + ref + (0,))
                    cnt["n_creates" if ins == _INS_CREATE else "n_deletes"] += 1
                elif status == "defer":
                    defer.append((f, r))
                    cnt["n_deferred_records"] += 1
                    first_def = f if first_def is None else min(first_def, f)
                else:
                    cnt[{"walk": "n_drop_walk", "no_position": "n_drop_no_position", "world": "n_drop_world",
                         "unpackable": "n_drop_unpackable"}[status]] += 1
                    error |= abi.RECDISP_ERROR_WALK if status == "walk" else 0
        else:                   # record_read.rs:18-41
            c, kind, after = abi.RCLS_READ_DROPPED, abi.RRUN_READ, NO_AFTER
            ok = bool(flags & HAS_POSITION)
            if ok and flags & HAS_PARAMETER:
                p0, pl = int(m["param_off"]), int(m["param_len"])
                if p0 + pl > len(b):
                    error |= abi.RECDISP_ERROR_WALK
                    ok = False
                else:
                    after = parse_after(b[p0:p0 + pl])
                    ok = after is not None
            if ok:
                w0, wl = int(m["world_off"]), int(m["world_len"])
                if w0 + wl > len(b):
                    error |= abi.RECDISP_ERROR_WALK
                    ok = False
                else:
                    ok = _sanitized(b[w0:w0 + wl]) is not None
            if ok and flags & WORLD_KNOWN and int(world_a[f]) < abi.WORLD_GLOBAL:
                c = abi.RCLS_READ
                q.append((f, int(world_a[f]), np.array(m["position"], np.float64).view(np.uint64).tolist(), after))
            elif ok:
                c = abi.RCLS_READ_DEFERRED
                defer.append((f, abi.RDEFER_READ))
                first_def = f if first_def is None else min(first_def, f)
        cls[j] = c
        if open_run != kind:                         # a barrier: process flushes the other kind's batch
            open_run = abi.RRUN_END
        if len(ops) > n_ops or len(q) > n_q:         # effective: it joins its kind's open batch or starts one
            if open_run != kind:
                runs.append((kind, f, n_ops, n_q))
            open_run = kind
    n_runs = len(runs)
    runs.append((abi.RRUN_END, n, len(ops), len(q)))
    caps = [len(ops) if ops_capacity is None else int(ops_capacity), len(defer) if defer_capacity is None else int(defer_capacity),
            n_runs + 1 if runs_capacity is None else int(runs_capacity)]
    cnt.update(n_db=len(src), n_records=examined, n_runs=n_runs, first_deferred=n if first_def is None else first_def, error=error)
    for k, name in enumerate(abi.RCLS_NAMES):
        cnt["n_" + name] = int((cls == k).sum())
    cnt["overflow"] = (abi.RECDISP_OVERFLOW_OPS if len(ops) > caps[0] else 0) | \
        (abi.RECDISP_OVERFLOW_DEFER if len(defer) > caps[1] else 0) | (abi.RECDISP_OVERFLOW_RUNS if n_runs + 1 > caps[2] else 0) | \
        (abi.RECDISP_OVERFLOW_RECORDS if limit is not None and cnt["n_records_total"] > limit else 0)
    op_a = np.zeros(min(len(ops), caps[0]), dtype=rec.REC_OP_DTYPE)
    for i, (k, w, bits, hi, lo, t, hd) in enumerate(ops[:caps[0]]):
        op_a[i] = (k, w, np.array(bits, np.uint64).view(np.float64), hi, lo, t, hd, 0)
    q_pos = np.array([r[2] for r in q], dtype=np.uint64).reshape(-1, 3).view(np.float64)
    return dict(cls=cls, ops=op_a, op_ref=np.array(refs[:caps[0]], dtype=abi.REC_OP_REF_DTYPE).reshape(-1),
                q_src=np.array([r[0] for r in q], np.uint32), q_world=np.array([r[1] for r in q], np.uint32), q_pos=q_pos,
                q_after=np.array([r[3] for r in q], np.int64), defer=np.array(defer[:caps[1]], dtype=abi.RECDISP_DEFER_DTYPE).reshape(-1),
                runs=np.array(runs[:min(n_runs + 1, caps[2])], dtype=abi.RECDISP_RUN_DTYPE).reshape(-1), counters=cnt)


def records_dispatch_counters(raw) -> dict:
    """abi.RECDISP_COUNTERS_DTYPE bytes as records_dispatch_np's counters dict."""
    c = np.asarray(raw).view(np.uint8)[:abi.RECDISP_COUNTERS_DTYPE.itemsize].view(abi.RECDISP_COUNTERS_DTYPE)[0]
    return {k: int(c[k]) for k in abi.RECDISP_COUNTERS_DTYPE.names}


class IngestTick:
    """The device arrays of one tick's decode, grow-only, and the step from received frames to
    Router.route_device: decode(frames, offsets) enqueues wq_frames_decode_device, route(...) the tick on
    the arrays it left, and nothing is read back or waited for between the two. read() is for tests and
    for the host's share of the tick (the counters, the unknown senders' uuids). A tick that is more than
    entity updates goes decode(...), dispatch(...), process(...): route() treats every frame as a
    LocalMessage, the dispatch splits them by instruction and process() issues the runs in order."""

    _SPEC = dict(msg=(72, np.uint8), pos=(24, np.uint8), world=(4, np.uint8), sender=(4, np.uint8), repl=(1, np.uint8),
                 instruction=(1, np.uint8), sender_uuid=(16, np.uint8), flex_range=(8, np.uint8), flags=(1, np.uint8))

    def __init__(self, router, capacity: int = 1024, device: str = "cuda:0"):
        import torch
        self.router, self.device, self.cap, self.n = router, device, 0, 0
        self.buf: dict = {}
        self.counters = torch.zeros(INGEST_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=device)
        # the control buffer's room in run entries and join rows; the frames of the tick's join(), None without one
        self.runs_cap, self.join_cap, self._join_n, self.join_counters = -1, 0, None, None
        self._grow(capacity)

    def _grow(self, n: int) -> None:
        import torch
        if n <= self.cap:
            return
        self.cap = max(n, 2 * self.cap)
        self.buf = {k: torch.zeros(max(self.cap * w, 8), dtype=torch.uint8, device=self.device)
                    for k, (w, _) in self._SPEC.items()}
        self.out = IngestOut(**{k: t.data_ptr() for k, t in self.buf.items()})

    def decode(self, frames, offsets, n_frames: int | None = None, n_frame_bytes: int | None = None) -> "IngestTick":
        """frames: a u8 device tensor; offsets: a device tensor of n + 1 u64 (torch int64 or uint64)."""
        n = offsets.numel() - 1 if n_frames is None else n_frames
        self._grow(n)
        self.n = n
        self._join_n = None   # a new tick: the control buffer holds no join of it yet
        self.router.decode_frames_device(frames.data_ptr() if frames.numel() else None, offsets.data_ptr(), n,
                                         frames.numel() if n_frame_bytes is None else n_frame_bytes, self.out,
                                         self.counters.data_ptr())
        return self

    def route(self, offsets_ptr: int, peers_ptr: int, msgs_ptr: int | None, capacity: int,
              counters_ptr: int | None = None) -> None:
        """Router.route_device on the decode's pos / world / sender / repl. Frames that did not decode,
        unresolved worlds and "@global" carry world ids no table holds, so they reach nobody."""
        o = self.out
        self.router.route_device(o.pos, o.world, o.sender, o.repl, self.n, offsets_ptr, peers_ptr, msgs_ptr, capacity,
                                 counters_ptr)

    def read(self) -> dict:
        """Every output and the counters as numpy arrays shaped like decode_frames_np's (synchronizes)."""
        import torch
        torch.cuda.synchronize()
        n = self.n
        raw = {k: self.buf[k][:n * w].cpu().numpy() for k, (w, _) in self._SPEC.items()}
        c = self.counters.cpu().numpy().view(INGEST_COUNTERS_DTYPE)[0]
        return dict(msg=raw["msg"].view(codec.DECODED_DTYPE), pos=raw["pos"].view(np.float64).reshape(n, 3),
                    world=raw["world"].view(np.uint32), sender=raw["sender"].view(np.uint32), repl=raw["repl"],
                    instruction=raw["instruction"], sender_uuid=raw["sender_uuid"].reshape(n, 16),
                    flex_range=raw["flex_range"].view(np.uint32).reshape(n, 2), flags=raw["flags"],
                    counters={k: int(c[k]) for k in INGEST_COUNTERS_DTYPE.names if k != "pad_"})

    # ---- the dispatch: the decoded tick split by instruction (wq_ingest_dispatch_device) ----
    _DSPEC = dict(cls=1, l_src=4, l_pos=24, l_world=4, l_sender=4, l_repl=1, g_src=4, g_world=4, g_sender=4, g_repl=1,
                  ops=40, op_src=4, side_src=4)
    _DTYPES = dict(cls=np.uint8, l_src=np.uint32, l_pos=np.float64, l_world=np.uint32, l_sender=np.uint32, l_repl=np.uint8,
                   g_src=np.uint32, g_world=np.uint32, g_sender=np.uint32, g_repl=np.uint8, ops=abi.OP_DTYPE,
                   op_src=np.uint32, side_src=np.uint32)
    _DCOUNT = dict(cls="n_frames", l_src="n_local", l_pos="n_local", l_world="n_local", l_sender="n_local", l_repl="n_local",
                   g_src="n_global", g_world="n_global", g_sender="n_global", g_repl="n_global", ops="n_op", op_src="n_op")
    RUNS_FIRST_READ = 4096   # run entries process() reads back with the counters; a longer table takes a second read

    def _grow_dispatch(self, n: int, runs_capacity: int) -> None:
        import torch
        if n > getattr(self, "dcap", 0) or not hasattr(self, "dbuf"):
            self.dcap = max(n, 2 * getattr(self, "dcap", 0), 1)
            # empty, not zeros: a fill would run on torch's stream, beside the call on the handle's
            self.dbuf = {k: torch.empty(max(self.dcap * w, 8), dtype=torch.uint8, device=self.device)
                         for k, w in self._DSPEC.items()}
        self._grow_ctrl(runs_capacity, 0)

    _CHEAD = abi.DISPATCH_COUNTERS_DTYPE.itemsize + abi.JOIN_COUNTERS_DTYPE.itemsize   # both counters, then the runs

    def _grow_ctrl(self, runs_capacity: int, joined_capacity: int) -> None:
        """The control buffer: the dispatch's counters, the join's counters, the run table, then j_id / j_frame /
        j_uuid. process() reads both counters and the run table with one copy."""
        import torch
        if runs_capacity <= self.runs_cap and joined_capacity <= self.join_cap:
            return
        if self._join_n is not None:
            raise ValueError("the control buffer would grow over a pending join: pass runs_capacity to join()")
        if runs_capacity > self.runs_cap:
            self.runs_cap = max(runs_capacity, 2 * self.runs_cap)
        if joined_capacity > self.join_cap:
            self.join_cap = max(joined_capacity, 2 * self.join_cap)
        self._j_at = (self._CHEAD + 20 * max(self.runs_cap, 1) + 7) // 8 * 8
        self.dctrl = torch.empty(self._j_at + 24 * self.join_cap + 8, dtype=torch.uint8, device=self.device)

    def dispatch(self, runs_capacity: int | None = None, last_seen=None, now: int = 0) -> "IngestTick":
        """Enqueues wq_ingest_dispatch_device on the arrays decode() left; nothing is read back. The rows, the
        side lists, the run table (runs_capacity entries, default n + 1: every table fits) and the counters
        stay on the device, grow-only beside the decode's. last_seen: a uint32 device tensor the heartbeats
        stamp with `now`."""
        n = self.n
        self._grow_dispatch(n, n + 1 if runs_capacity is None else runs_capacity)
        self.d_runs_capacity = n + 1 if runs_capacity is None else runs_capacity
        o = self.out
        self.d_in = abi.DispatchIn(instruction=o.instruction, flags=o.flags, world=o.world, sender=o.sender, repl=o.repl,
                                   pos=o.pos, last_seen=None if last_seen is None else last_seen.data_ptr(),
                                   n_last_seen=0 if last_seen is None else last_seen.numel(), now=now)
        self.d_out = abi.DispatchOut(**{k: t.data_ptr() for k, t in self.dbuf.items()},
                                     runs=self.dctrl.data_ptr() + self._CHEAD if self.d_runs_capacity else None,
                                     runs_capacity=self.d_runs_capacity)
        self.router.dispatch_device(self.d_in, n, self.d_out, self.dctrl.data_ptr())
        return self

    # ---- the joins: new senders get their ids between decode() and dispatch() (wq_ingest_join_device) ----
    def join(self, free_ids, id_next: int, id_limit: int, joined_capacity: int | None = None,
             runs_capacity: int | None = None) -> "IngestTick":
        """Enqueues wq_ingest_join_device on the arrays decode() left, before dispatch(): sender and flags are
        patched in place and the handle's sender table (Router.reserve_peers) takes the joins. free_ids: a
        uint32 device tensor in pop order, or None. The counters and j_uuid / j_id / j_frame
        (joined_capacity rows, default n) sit in the dispatch's control buffer, so process() still has one
        read-back: it leaves the counters in `join_counters`; read_join() fetches the rows. runs_capacity:
        what dispatch() will be given, when that is more than n + 1."""
        n = self.n
        jc = n if joined_capacity is None else joined_capacity
        self._join_n = None
        self._grow_ctrl(n + 1 if runs_capacity is None else runs_capacity, jc)
        o, base = self.out, self.dctrl.data_ptr() + self._j_at
        self.j_capacity = jc
        self.j_in = abi.JoinIn(instruction=o.instruction, world=o.world, sender_uuid=o.sender_uuid, flags=o.flags,
                               sender=o.sender, free_ids=None if free_ids is None or not free_ids.numel() else free_ids.data_ptr(),
                               n_free=0 if free_ids is None else free_ids.numel(), id_next=id_next, id_limit=id_limit)
        self.j_out = abi.JoinOut(j_id=base, j_frame=base + 4 * self.join_cap, j_uuid=base + 8 * self.join_cap,
                                 joined_capacity=jc)
        self.router.join_peers_device(self.j_in, n, self.j_out, self.dctrl.data_ptr() + abi.DISPATCH_COUNTERS_DTYPE.itemsize)
        self._join_n = n
        return self

    def read_join(self) -> dict:
        """The join's patched sender / flags, its rows and counters as numpy arrays shaped like join_peers_np's
        (synchronizes; for tests, and for the host's PeerIds.adopt in a tick with joins)."""
        import torch
        torch.cuda.synchronize()
        c0 = abi.DISPATCH_COUNTERS_DTYPE.itemsize
        cnt = join_counters(self.dctrl[c0:self._CHEAD].cpu().numpy())
        k = 0 if cnt["overflow"] or cnt["error"] & abi.JOIN_ERROR_NO_TABLE else cnt["n_joined"]
        a, J = self._j_at, self.join_cap
        raw = self.dctrl[a:a + 24 * J].cpu().numpy() if k else np.zeros(24 * J, np.uint8)
        n = self.n
        return dict(counters=cnt, j_id=raw[:4 * k].view(np.uint32).copy(), j_frame=raw[4 * J:4 * J + 4 * k].view(np.uint32).copy(),
                    j_uuid=raw[8 * J:8 * J + 16 * k].reshape(k, 16).copy(),
                    sender=self.buf["sender"][:4 * n].cpu().numpy().view(np.uint32),
                    flags=self.buf["flags"][:n].cpu().numpy())

    # ---- the leaves: the sweep between ticks (wq_ingest_leave_device, then wq_remove_peers_device) ----
    _LSPEC = dict(l_uuid=16, l_id=4, l_reason=1, l_param=abi.LEAVE_TEXT)

    def leave(self, last_seen, now: int, max_age: int, pinned_bits=None, leave_ids=None, free_ids=None,
              leave_capacity: int | None = None, free_capacity: int | None = None, remove: bool = True) -> "IngestTick":
        """Enqueues wq_ingest_leave_device and, with `remove`, wq_remove_peers_device on its bitmap and its
        n_left, back to back on the handle's stream; nothing is read back. last_seen: the uint32 device tensor
        the dispatch stamps (one entry per id, initialised to abi.SEEN_NEVER); pinned_bits, leave_ids, free_ids:
        uint32 device tensors or None. The outputs stay on the device, grow-only: `lbuf` holds l_uuid, l_id,
        l_reason, l_param, l_param_offsets (leave_capacity rows, default the ids' count), gone_bits and free_out
        (free_capacity entries, default the free list's length plus leave_capacity), `leave_counters_dev` the
        counters. l_param / l_param_offsets are what Router.build_frames_device takes for the PeerDisconnect
        frames. read_leave() fetches everything."""
        import torch
        n_ids = last_seen.numel()
        n_free = 0 if free_ids is None else free_ids.numel()
        n_leave = 0 if leave_ids is None else leave_ids.numel()
        lc = n_ids if leave_capacity is None else leave_capacity
        fc = n_free + lc if free_capacity is None else free_capacity
        words = (n_ids + 31) // 32
        need = dict(l_uuid=16 * lc, l_id=4 * lc, l_reason=lc, l_param=abi.LEAVE_TEXT * lc, l_param_offsets=8 * (lc + 1),
                    gone_bits=4 * words, free_out=4 * fc)
        if not hasattr(self, "lbuf"):
            self.lbuf = {}
            self.leave_counters_dev = torch.empty(abi.LEAVE_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        for k, b in need.items():
            if k not in self.lbuf or self.lbuf[k].numel() < b:
                # empty, not zeros: a fill would run on torch's stream, beside the call on the handle's
                self.lbuf[k] = torch.empty(max(2 * b, 8), dtype=torch.uint8, device=self.device)
        ptr = lambda t: None if t is None or not t.numel() else t.data_ptr()
        self.lv_n_ids, self.lv_capacity, self.lv_free_capacity = n_ids, lc, fc
        self.lv_in = abi.LeaveIn(last_seen=ptr(last_seen), pinned_bits=ptr(pinned_bits), leave_ids=ptr(leave_ids),
                                 free_ids=ptr(free_ids), n_ids=n_ids, now=now, max_age=max_age, n_leave=n_leave, n_free=n_free)
        self.lv_out = abi.LeaveOut(**{k: t.data_ptr() for k, t in self.lbuf.items()}, leave_capacity=lc, free_capacity=fc)
        self.lv_last_seen = last_seen
        cptr = self.leave_counters_dev.data_ptr()
        self.router.leave_peers_device(self.lv_in, self.lv_out, cptr)
        if remove:
            self.router.remove_peers_device(self.lbuf["gone_bits"].data_ptr(), n_ids,
                                            cptr + abi.LEAVE_COUNTERS_DTYPE.fields["n_left"][1])
        return self

    def read_leave(self) -> dict:
        """The last leave()'s outputs and counters as numpy arrays shaped like leave_peers_np's (synchronizes;
        for tests, and for the host's PeerIds.release_ids after a sweep with leavers)."""
        import torch
        torch.cuda.synchronize()
        cnt = leave_counters(self.leave_counters_dev.cpu().numpy())
        done = not cnt["overflow"] and not cnt["error"] & abi.LEAVE_ERROR_NO_TABLE
        k = cnt["n_left"] if done else 0
        raw = {name: self.lbuf[name][:k * w].cpu().numpy() for name, w in self._LSPEC.items()}
        return dict(counters=cnt, l_uuid=raw["l_uuid"].reshape(k, 16), l_id=raw["l_id"].view(np.uint32), l_reason=raw["l_reason"],
                    l_param=raw["l_param"],
                    l_param_offsets=self.lbuf["l_param_offsets"][:8 * (k + 1) if done else 0].cpu().numpy().view(np.uint64),
                    gone_bits=self.lbuf["gone_bits"][:4 * ((self.lv_n_ids + 31) // 32)].cpu().numpy().view(np.uint32),
                    free_out=self.lbuf["free_out"][:4 * cnt["n_free"] if done else 0].cpu().numpy().view(np.uint32),
                    last_seen=self.lv_last_seen.cpu().numpy().view(np.uint32).reshape(-1))

    def _read_ctrl(self):
        """The counters and the run table: one copy for tables of up to RUNS_FIRST_READ entries. Waits for
        the device first, as read() does: the handle's stream is not torch's."""
        import torch
        torch.cuda.synchronize()
        csize = self._CHEAD
        first = min(self.d_runs_capacity, self.RUNS_FIRST_READ)
        raw = self.dctrl[:csize + 20 * first].cpu().numpy()
        cnt = dispatch_counters(raw)
        # the join's counters of this tick, None without a join() since decode()
        self.join_counters = join_counters(raw[abi.DISPATCH_COUNTERS_DTYPE.itemsize:csize]) \
            if self._join_n is not None else None
        have = min(cnt["n_runs"] + 1, self.d_runs_capacity)
        if have > first:
            raw = self.dctrl[:csize + 20 * have].cpu().numpy()
        return cnt, raw[csize:csize + 20 * have].copy().view(abi.DISPATCH_RUN_DTYPE)

    def process(self, offsets, peers, route_counters=None):
        """Reads the counters and the run table (the tick's one read-back) and issues the runs in order on the
        router: Router.apply_ops_device on a table run's slice of the ops, Router.route_device and
        Router.route_global_device on a read run's slices of the LocalMessage and GlobalMessage rows.

        offsets, peers: the caller's CSR buffers, int32 device tensors. Every route call gets its own
        region of both, beginning at a multiple of four entries: rows + 1 offsets, and rows * K pairs, K =
        what `peers` holds beyond the alignment, divided evenly by the tick's rows. route_counters
        (nullable): a uint8 device tensor of 24 bytes per call (abi.COUNTERS_DTYPE), in call order.

        Returns (counters, runs, reads): the dispatch's counters, the run table, and per read run a dict of
        run, first_frame and, under "local" and "global", None or a dict of rows (begin, end in l_* / g_*),
        offsets (the region's first entry), peers (its first pair), capacity and call (its index in
        route_counters)."""
        cnt, runs = self._read_ctrl()
        if cnt["overflow"] & abi.DISPATCH_OVERFLOW_RUNS:
            raise ValueError(f"the run table holds {self.d_runs_capacity} entries, the tick needs {cnt['n_runs'] + 1}")
        spans = []
        for a, b in zip(runs[:-1], runs[1:]):
            if a["kind"] == abi.RUN_READ:
                spans += [s for s in ((int(a["l_begin"]), int(b["l_begin"])), (int(a["g_begin"]), int(b["g_begin"]))) if s[1] > s[0]]
        rows = cnt["n_local"] + cnt["n_global"]
        if offsets.numel() < rows + 4 * len(spans):
            raise ValueError(f"offsets: {rows + 4 * len(spans)} entries needed")
        per_row = max(peers.numel() - 4 * len(spans), 0) // max(rows, 1)
        if route_counters is not None and route_counters.numel() < 24 * len(spans):
            raise ValueError(f"route_counters: {24 * len(spans)} bytes needed")
        r, o = self.router, self.d_out
        at = dict(o=0, p=0, call=0)

        def region(lo, hi):
            n = hi - lo
            d = dict(rows=(lo, hi), offsets=at["o"], peers=at["p"], capacity=n * per_row, call=at["call"])
            at["o"] += -(-(n + 1) // 4) * 4
            at["p"] += -(-(n * per_row) // 4) * 4
            at["call"] += 1
            return d

        reads = []
        for k, (a, nxt) in enumerate(zip(runs[:-1], runs[1:])):
            if a["kind"] == abi.RUN_TABLE:
                lo, hi = int(a["op_begin"]), int(nxt["op_begin"])
                r.apply_ops_device(o.ops + 40 * lo, hi - lo)
                continue
            read = dict(run=k, first_frame=int(a["first_frame"]), local=None, **{"global": None})
            lo, hi = int(a["l_begin"]), int(nxt["l_begin"])
            if hi > lo:
                d = read["local"] = region(lo, hi)
                r.route_device(o.l_pos + 24 * lo, o.l_world + 4 * lo, o.l_sender + 4 * lo, o.l_repl + lo, hi - lo,
                               offsets.data_ptr() + 4 * d["offsets"], peers.data_ptr() + 4 * d["peers"], None, d["capacity"],
                               None if route_counters is None else route_counters.data_ptr() + 24 * d["call"])
            lo, hi = int(a["g_begin"]), int(nxt["g_begin"])
            if hi > lo:
                d = read["global"] = region(lo, hi)
                r.route_global_device(o.g_world + 4 * lo, o.g_sender + 4 * lo, o.g_repl + lo, hi - lo,
                                      offsets.data_ptr() + 4 * d["offsets"], peers.data_ptr() + 4 * d["peers"], None,
                                      d["capacity"], None if route_counters is None else route_counters.data_ptr() + 24 * d["call"])
            reads.append(read)
        return cnt, runs, reads

    # ---- the sends: one per-peer frame list from all the regions process() left (wq_tick_sends_device) ----
    def sends(self, reads, offsets, peers, n_peers: int, connected=None, extra=(), n_frames: int | None = None):
        """Enqueues wq_tick_sends_device on the regions process() left in `offsets` / `peers` (the tensors it was
        given; `reads` as it returned them): every read run's LocalMessage region maps its rows to frames
        through the dispatch's l_src, its GlobalMessage region through g_src. extra: further regions
        (abi.send_region tuples), e.g. unit rows with a frame_base behind the received frames; n_frames: the
        size of the frame index space, default the tick's frames. connected: a uint32 device tensor of
        ceil(n_peers / 32) words, or None. Nothing is read back. Returns (peer_offsets, frames_out): int32
        device tensors of n_peers + 1 entries and of the regions' capacities' sum, views of grow-only buffers;
        peer p's frames are frames_out[peer_offsets[p] : peer_offsets[p + 1]], ascending: what
        Router.peer_pack_device takes with the tick's received frames. read_sends() fetches them."""
        import torch
        rows = []
        for read in reads:
            for key, sel in (("local", 0), ("global", 1)):
                g = read[key]
                if g is not None:
                    lo, hi = g["rows"]
                    rows.append(abi.send_region(off_at=g["offsets"], peers_at=g["peers"], n_rows=hi - lo, capacity=g["capacity"],
                                                src_at=lo, src_sel=sel))
        rows += [tuple(e) for e in extra]
        reg = np.array(rows, dtype=abi.SEND_REGION_DTYPE) if rows else np.zeros(0, abi.SEND_REGION_DTYPE)
        n_elems = int(reg["capacity"].astype(np.int64).sum())
        if not hasattr(self, "sbuf"):
            self.sbuf = dict(counters=torch.empty(abi.TICK_SENDS_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=self.device))
        for k, need in (("peer_offsets", n_peers + 1), ("frames", n_elems)):   # grow-only; empty, not zeros (see above)
            if k not in self.sbuf or self.sbuf[k].numel() < need:
                self.sbuf[k] = torch.empty(max(2 * need, 8), dtype=torch.int32, device=self.device)
        have = hasattr(self, "dbuf")
        src = (self.dbuf["l_src"], self.dbuf["g_src"]) if have else (None, None)
        self.s_n_peers, self.s_n_elems = n_peers, n_elems
        self.router.tick_sends_device(reg, offsets.data_ptr() if offsets.numel() else None, offsets.numel(),
                                      peers.data_ptr() if peers.numel() else None, peers.numel(),
                                      [t.data_ptr() if have else None for t in src], [self.dcap if have else 0] * 2,
                                      None if connected is None else connected.data_ptr(), n_peers,
                                      self.n if n_frames is None else n_frames, self.sbuf["peer_offsets"].data_ptr(),
                                      self.sbuf["frames"].data_ptr() if n_elems else None, n_elems,
                                      self.sbuf["counters"].data_ptr())
        return self.sbuf["peer_offsets"][:n_peers + 1], self.sbuf["frames"][:n_elems]

    def read_sends(self) -> dict:
        """The last sends()'s outputs as numpy arrays shaped like interest.tick_sends_np's: peer_offsets, frames
        (the kept ones) and counters (synchronizes; for tests)."""
        import torch
        torch.cuda.synchronize()
        c = self.sbuf["counters"].cpu().numpy().view(abi.TICK_SENDS_COUNTERS_DTYPE)[0]
        po = self.sbuf["peer_offsets"][:self.s_n_peers + 1].cpu().numpy().view(np.uint32)
        return dict(peer_offsets=po, frames=self.sbuf["frames"][:int(po[-1])].cpu().numpy().view(np.uint32),
                    counters={k: int(c[k]) for k in abi.TICK_SENDS_COUNTERS_DTYPE.names if not k.endswith("_")})

    def read_dispatch(self) -> dict:
        """Every output of the dispatch and the counters as numpy arrays shaped like dispatch_np's
        (synchronizes; for tests and for the host's share of the tick: the side lists)."""
        import torch
        torch.cuda.synchronize()
        cnt, runs = self._read_ctrl()
        got = dict(counters=cnt, runs=runs)
        for k, w in self._DSPEC.items():
            rows = cnt["side_begin"][5] if k == "side_src" else cnt[self._DCOUNT[k]]
            a = self.dbuf[k][:rows * w].cpu().numpy().view(self._DTYPES[k])
            got[k] = a.reshape(rows, 3) if k == "l_pos" else a
        return got

    # ---- the record dispatch: the tick's record frames to store ops and queries (wq_records_dispatch_device) ----
    _RSPEC = dict(cls=(1, np.uint8), ops=(64, rec.REC_OP_DTYPE), op_ref=(32, abi.REC_OP_REF_DTYPE), q_src=(4, np.uint32),
                  q_world=(4, np.uint32), q_pos=(24, np.float64), q_after=(8, np.int64), defer=(8, abi.RECDISP_DEFER_DTYPE))
    _RCSIZE = abi.RECDISP_COUNTERS_DTYPE.itemsize

    def records_dispatch(self, frames, offsets, now_us: int, free_handles=None, handle_next: int = 0,
                         max_records: int | None = None, ops_capacity: int | None = None, defer_capacity: int | None = None,
                         runs_capacity: int | None = None, counters: dict | None = None) -> "IngestTick":
        """Enqueues wq_records_dispatch_device on the arrays decode() and dispatch() left: frames / offsets are the
        device tensors decode() took, db_src is the database segment of the dispatch's side_src, taken where it
        lies once the dispatch's counters are known (`counters`, else one read of them). free_handles: the
        handles the call's creates take first (a sequence of u32), then handle_next onwards. max_records
        defaults to frames.numel() // 4, which always suffices; the capacities default to what holds
        everything under that bound. The router needs an open record store. Nothing is read back here."""
        import torch
        cnt = counters if counters is not None else self._read_ctrl()[0]
        sb = cnt["side_begin"]
        n_db = sb[3] - sb[2]
        nb = frames.numel()
        limit = min(nb // 4, abi.RECDISP_MAX_RECORDS - 1) if max_records is None else int(max_records)
        caps = dict(ops=limit if ops_capacity is None else ops_capacity,
                    defer=limit + n_db if defer_capacity is None else defer_capacity,
                    runs=n_db + 1 if runs_capacity is None else runs_capacity)
        rows = dict(cls=n_db, ops=caps["ops"], op_ref=caps["ops"], q_src=n_db, q_world=n_db, q_pos=n_db, q_after=n_db,
                    defer=caps["defer"])
        if not hasattr(self, "rbuf"):
            self.rbuf, self.rctrl = {}, None
        for k, (w, _) in self._RSPEC.items():   # grow-only; empty, not zeros: a fill would run on torch's stream
            if k not in self.rbuf or self.rbuf[k].numel() < max(rows[k] * w, 8):
                self.rbuf[k] = torch.empty(max(2 * rows[k] * w, 8), dtype=torch.uint8, device=self.device)
        if self.rctrl is None or self.rctrl.numel() < self._RCSIZE + 16 * caps["runs"]:
            self.rctrl = torch.empty(self._RCSIZE + 32 * max(caps["runs"], 1), dtype=torch.uint8, device=self.device)
        free = np.ascontiguousarray(free_handles if free_handles is not None else [], dtype=np.uint32)
        # a copy from pageable host memory has landed when .to() returns, whatever stream it ran on
        self.r_free = torch.from_numpy(free.view(np.int32).copy()).to(self.device) if len(free) else None
        ptr = {k: (self.rbuf[k].data_ptr() if rows[k] or k in ("cls", "q_src", "q_world", "q_pos", "q_after") else None)
               for k in self._RSPEC}
        self.r_caps, self.r_rows, self.r_n_db = caps, rows, n_db
        o = self.out
        self.r_in = abi.RecDispatchIn(frames=frames.data_ptr() if nb else None, frame_offsets=offsets.data_ptr(),
                                      n_frames=self.n, n_frame_bytes=nb, msg=o.msg, world=o.world, flags=o.flags,
                                      db_src=self.d_out.side_src + 4 * sb[2], n_db=n_db, now_us=now_us,
                                      free_handles=None if self.r_free is None else self.r_free.data_ptr(), n_free=len(free),
                                      handle_next=handle_next, max_records=limit)
        self.r_out = abi.RecDispatchOut(**ptr, runs=self.rctrl.data_ptr() + self._RCSIZE if caps["runs"] else None,
                                        ops_capacity=caps["ops"], defer_capacity=caps["defer"], runs_capacity=caps["runs"])
        self.router.records_dispatch_device(self.r_in, self.r_out, self.rctrl.data_ptr())
        return self

    def read_records_ctrl(self):
        """The record dispatch's counters and run table: one copy. Waits for the device first."""
        import torch
        torch.cuda.synchronize()
        raw = self.rctrl[:self._RCSIZE + 16 * self.r_caps["runs"]].cpu().numpy()
        cnt = records_dispatch_counters(raw)
        have = min(cnt["n_runs"] + 1, self.r_caps["runs"])
        return cnt, raw[self._RCSIZE:self._RCSIZE + 16 * have].copy().view(abi.RECDISP_RUN_DTYPE)

    def read_records_rows(self, k: str, lo: int, hi: int) -> np.ndarray:
        """Rows [lo, hi) of the record dispatch's output k (after read_records_ctrl: the device has finished)."""
        w, dt = self._RSPEC[k]
        a = self.rbuf[k][lo * w:hi * w].cpu().numpy().view(dt)
        return a.reshape(-1, 3) if k == "q_pos" else a

    def read_records_dispatch(self) -> dict:
        """Every output of the record dispatch and the counters as numpy arrays shaped like
        records_dispatch_np's (synchronizes; for tests)."""
        cnt, runs = self.read_records_ctrl()
        n_ops = min(cnt["n_creates"] + cnt["n_deletes"], self.r_caps["ops"])
        n_def = min(cnt["n_deferred_records"] + cnt["n_read_deferred"], self.r_caps["defer"])
        have = dict(cls=cnt["n_db"], ops=n_ops, op_ref=n_ops, q_src=cnt["n_read"], q_world=cnt["n_read"], q_pos=cnt["n_read"],
                    q_after=cnt["n_read"], defer=n_def)
        got = {k: self.read_records_rows(k, 0, n) for k, n in have.items()}
        got.update(counters=cnt, runs=runs)
        return got

    def slab_store(self, frames, offsets, slab, n_ops: int) -> dict:
        """The payloads of the tick's created records into a records.DeviceRecordSlab, on the ops and
        references records_dispatch() left and the frames / offsets decode() took. n_ops: the accepted ops,
        n_creates + n_deletes of the record dispatch's counters (the rows behind them are an earlier tick's).
        Returns the slab's counters of the call that fitted (DeviceRecordSlab.store grows and retries)."""
        return slab.store(self.r_out.ops, self.r_out.op_ref, int(n_ops), frames.data_ptr() if frames.numel() else 0,
                          offsets.data_ptr(), self.n)

    INS_RECORD_REPLY = 12   # codec.INSTRUCTION_NAMES

    def build_record_frames(self, lo: int, hi: int, frames, offsets, row_offsets, handles, n_handles: int, slab_view,
                            flags: int = abi.FRAMES_SKIP_EMPTY):
        """The RecordReply frames of the query rows [lo, hi) records_dispatch() left, through
        Router.build_record_frames_device: row_offsets (i32[hi - lo + 1]) / handles (i32, None without any) are
        the device tensors wq_records_read_device filled for those rows, slab_view the abi.SlabView of the
        payload slab, frames / offsets the tensors decode() took. Every reply is Message { RecordReply, the
        query's world name as its frame held it (taken from the frames on the device), the row's records, the
        rest default }. A sizing call, one read of its counters, then the build. Returns (frames u8, sizes
        i32[hi - lo], recipients i32[hi - lo]: the decode's `sender` of each query) as device tensors;
        ValueError when the build reports an error bit."""
        import torch
        n, dev = hi - lo, self.device
        # where each query's world name lies, and who asked (torch's stream; waited for below)
        q_src = self.rbuf["q_src"][4 * lo:4 * hi].view(torch.int32).to(torch.int64)
        msg = self.buf["msg"][:self.n * 72].view(self.n, 72)[q_src]
        w_off = (offsets.view(torch.int64)[q_src] + msg[:, 48:52].contiguous().view(torch.int32).view(-1).to(torch.int64)).contiguous()
        w_len = msg[:, 52:56].contiguous().view(torch.int32).view(-1).contiguous()
        recipients = self.buf["sender"][:self.n * 4].view(torch.int32)[q_src].contiguous()
        src = abi.FramesSrc(instruction_all=self.INS_RECORD_REPLY)
        rec = abi.FramesRecSrc(row_offsets=row_offsets.data_ptr(), handles=handles.data_ptr() if handles is not None and n_handles else None,
                               n_handles=n_handles, slab=slab_view, world_bytes=frames.data_ptr() if frames.numel() else None,
                               world_off=w_off.data_ptr(), world_len=w_len.data_ptr(), n_world_bytes=frames.numel(), flags=flags)
        if not frames.numel():
            zero_world = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
            rec.world_bytes, src.world = None, zero_world.data_ptr()
        fo = torch.empty(n + 1, dtype=torch.int64, device=dev)
        sizes = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
        cnt = torch.empty(abi.FRAMES_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        self.router.build_record_frames_device(src, rec, n, None, 0, fo.data_ptr(), None, cnt.data_ptr())
        torch.cuda.synchronize()
        nbytes = int(cnt.cpu().numpy().view(abi.FRAMES_COUNTERS_DTYPE)[0]["bytes_need"])
        out = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        self.router.build_record_frames_device(src, rec, n, out.data_ptr(), nbytes, fo.data_ptr(), sizes.data_ptr(), cnt.data_ptr())
        torch.cuda.synchronize()
        c = cnt.cpu().numpy().view(abi.FRAMES_COUNTERS_DTYPE)[0]
        if int(c["error"]) or int(c["overflow"]):
            raise ValueError(f"record frames: error {int(c['error']):#x}, overflow {int(c['overflow'])}")
        return out[:nbytes], sizes, recipients

    def read_msg_rows(self, frames_idx) -> np.ndarray:
        """The decoder's msg structs of the given frames (after a read that waited for the device)."""
        import torch
        idx = torch.as_tensor(np.asarray(frames_idx, np.int64), device=self.device)
        return self.buf["msg"][:self.n * 72].view(self.n, 72)[idx].cpu().numpy().reshape(-1).view(codec.DECODED_DTYPE)


def deferred_event(frame: bytes, m, record: int) -> dict:
    """One entry of the record dispatch's deferred list as an event of records.RecordProcessor: the read
    (record == abi.RDEFER_READ) or the frame's create / delete with that one record, taken from a frame the
    decoder accepted (m: its msg struct)."""
    w0, p0 = int(m["world_off"]), int(m["param_off"])
    event = dict(instruction={_INS_CREATE: "RecordCreate", _INS_READ: "RecordRead", _INS_DELETE: "RecordDelete"}[int(m["instruction"])],
                 world_name=frame[w0:w0 + int(m["world_len"])].decode("utf-8"), sender_uuid=_uuid.UUID(bytes=bytes(m["sender_uuid"])),
                 parameter=frame[p0:p0 + int(m["param_len"])].decode("utf-8") if m["has_parameter"] else None,
                 position=tuple(float(c) for c in m["position"]) if m["has_position"] else None, records=[])
    if record != abi.RDEFER_READ:
        rd = _Reader(frame)
        vec, _ = rd.vec_range(rd.follow(rd.field(rd.visit_table(rd.follow(0)), _VT_RECORDS)), 4)
        t = rd.visit_table(rd.follow(vec + 4 * record))
        text = lambda r: None if r is None else frame[r[0]:r[0] + r[1]]   # noqa: E731
        u = parse_uuid_text(text(rd.field_bytes(t, _VT_REC_UUID)))
        at, data = rd.field_vec3(t, _VT_REC_POS), text(rd.field_bytes(t, _VT_REC_DATA))
        event["records"] = [dict(uuid=(u >> 64, u & ((1 << 64) - 1)), world_name=text(rd.field_bytes(t, _VT_REC_WORLD)).decode("utf-8"),
                                 position=struct.unpack_from("<3d", frame, at) if at else None,
                                 data=None if data is None else data.decode("utf-8"), flex=text(rd.field_bytes(t, _VT_REC_FLEX)))]
    return event
