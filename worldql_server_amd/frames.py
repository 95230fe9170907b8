"""Frame builder, the host side (include/wq_router.h, "frame builder"; kernels: csrc/wq_frames.hip).

`build_frames_np` is the definition of what wq_frames_build_device writes: it applies the call's
malformed-input rules to numpy inputs and hands the resulting flat messages to the host serializer
(codec.serialize_messages, the restatement of Message::serialize), so the device's frames are checked
byte for byte against the bytes every decoder and client already takes. `frame_size_np` is the size of
a flat frame in closed form. `world_table` lays a list of names out as wq_frames_set_worlds takes them
and `FramesSrc` is struct wq_frames_src. `build_record_frames_np` and `record_frame_size_np` are the same
two for messages that carry a `records` vector read from the payload slab (records.slab_store_np) through a
CSR of handles: the definition of what wq_frames_build_records_device writes (csrc/wq_reply.hip), and
`FramesRecSrc` is struct wq_frames_rec_src.
"""
from __future__ import annotations

import numpy as np

from .abi import (FRAMES_COUNTERS_DTYPE, FRAMES_ERROR_FLEX as ERROR_FLEX, FRAMES_ERROR_PARAM as ERROR_PARAM,  # noqa: F401
                  FRAMES_ERROR_TOO_LARGE as ERROR_TOO_LARGE, FRAMES_ERROR_WORLD as ERROR_WORLD,
                  FRAMES_HAS_FLEX as HAS_FLEX, FRAMES_HAS_PARAMETER as HAS_PARAMETER,
                  FRAMES_HAS_POSITION as HAS_POSITION, FRAME_MAX, FramesRecSrc, FramesSrc)


def world_table(names):
    """(bytes, offsets u32[n + 1]) of a list of world names (str or bytes), as wq_frames_set_worlds takes them."""
    raw = [n if isinstance(n, (bytes, bytearray)) else n.encode("utf-8") for n in names]
    off = np.zeros(len(raw) + 1, dtype=np.uint32)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return b"".join(raw), off


def _up4(v):
    return (v + 3) & ~3


def frame_size_np(has_position, instruction, replication, world_len, param_len=None, flex_len=None) -> int:
    """Size of the flat frame with these fields (param_len / flex_len None: the field is absent). Pieces in
    the order the builder pushes them, every one ending on a multiple of four: the parameter string
    (NUL and padding, then its length), the 36-character uuid (44), the world string, the two empty
    vectors (8), the flex vector; then the table (the offsets, the position's 24 bytes, one byte for
    each of replication and instruction that is not 0, padding, the soffset), the vtable of 18, 20 or
    22 bytes, padding, and the root offset."""
    size = 44 + _up4(int(world_len) + 1) + 4 + 8
    if param_len is not None:
        size += _up4(int(param_len) + 1) + 4
    if flex_len is not None:
        size += _up4(int(flex_len)) + 4
    table = 16 + (4 if flex_len is not None else 0) + (24 if has_position else 0) + (4 if param_len is not None else 0)
    table += (1 if replication else 0) + (1 if instruction else 0)
    table = _up4(table) + 4
    table += 22 if flex_len is not None else 20 if has_position else 18
    return size + _up4(table) + 4


def _per_message(v, n, name):
    if v is None or np.isscalar(v):
        return np.full(n, 0 if v is None else int(v), dtype=np.uint8)
    a = np.ascontiguousarray(v, dtype=np.uint8)
    if len(a) != n:
        raise ValueError(f"{name}: one byte per message")
    return a


def _range(off, i, n_bytes):
    """(start, length, ok) of payload i under the rules of a frame's range."""
    a, b = int(off[i]), int(off[i + 1])
    if a > b or b > n_bytes or b - a >= 1 << 32:
        return 0, 0, False
    return a, b - a, True


def build_frames_np(worlds, sender_uuid, world, instruction=0, replication=0, pos=None, param=None, param_offsets=None,
                    flex=None, flex_offsets=None, msg_flags=None, capacity=None, n_param_bytes=None, n_flex_bytes=None):
    """The definition of wq_frames_build_device: (frames u8[bytes_written], offsets u64[n + 1], sizes
    u32[n], counters) with counters a dict of n_frames, n_complete, bytes_need, bytes_written, overflow,
    error.

    worlds: the handle's table, a list of names (None or empty: no table). sender_uuid: n x 16 bytes;
    world: n ids; instruction / replication: one value for every message or n of them; pos: n x 3 f64 or
    None; param / param_offsets and flex / flex_offsets: payload bytes and u64 offsets[n + 1], or None;
    msg_flags: n bytes or None. A message has a field when its array is given and, with msg_flags, its
    bit is set. The rules: a world id outside the table gives an empty name (error bit 0); a payload
    range that descends, reaches past the payload's bytes or spans 2^32 or more is present and empty
    (bits 1, 2); a frame above 2^30 bytes is empty (bit 3). n_param_bytes / n_flex_bytes stand in for
    the payloads' lengths in a sizing call (capacity 0) that has no payload memory. Only the first
    `capacity` bytes are written (None: all). A parameter that is not UTF-8 raises, as the host
    serializer refuses it."""
    from . import codec
    world = np.ascontiguousarray(world, dtype=np.uint32)
    n = len(world)
    uu = np.ascontiguousarray(sender_uuid, dtype=np.uint8).reshape(-1, 16)
    if len(uu) != n:
        raise ValueError("sender_uuid: 16 bytes per message")
    if (param is None) != (param_offsets is None) or (flex is None) != (flex_offsets is None):
        raise ValueError("a payload and its offsets are given together or not at all")
    names = [w if isinstance(w, (bytes, bytearray)) else w.encode("utf-8") for w in (worlds or [])]
    ins, rep = _per_message(instruction, n, "instruction"), _per_message(replication, n, "replication")
    p3 = None if pos is None else np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    given = (HAS_POSITION if p3 is not None else 0) | (HAS_PARAMETER if param is not None else 0) | \
        (HAS_FLEX if flex is not None else 0)
    flags = np.full(n, given, np.uint8) if msg_flags is None else np.ascontiguousarray(msg_flags, np.uint8) & given
    pay = {}
    for key, data, off, nb in (("parameter", param, param_offsets, n_param_bytes), ("flex", flex, flex_offsets, n_flex_bytes)):
        if data is not None:
            data = np.ascontiguousarray(data, dtype=np.uint8)
            pay[key] = (data, np.ascontiguousarray(off, dtype=np.uint64), len(data) if nb is None else int(nb))
    sizing = capacity is not None and int(capacity) == 0
    error, msgs, sizes = 0, [], np.zeros(n, dtype=np.uint32)
    for i in range(n):
        w = int(world[i])
        if w >= len(names):
            error |= ERROR_WORLD
        m = dict(instruction=int(ins[i]), replication=int(rep[i]), sender_uuid=uu[i].tobytes(),
                 world_name=names[w] if w < len(names) else b"")
        lens = {}
        for key, bit, err in (("parameter", HAS_PARAMETER, ERROR_PARAM), ("flex", HAS_FLEX, ERROR_FLEX)):
            if flags[i] & bit:
                data, off, nb = pay[key]
                a, ln, ok = _range(off, i, nb)
                if not ok:
                    error |= err
                lens[key] = ln
                if not sizing:
                    m[key] = data[a:a + ln].tobytes()
        if flags[i] & HAS_POSITION:
            m["position"] = p3[i]
        size = frame_size_np(bool(flags[i] & HAS_POSITION), m["instruction"], m["replication"], len(m["world_name"]),
                             lens.get("parameter"), lens.get("flex"))
        if size > FRAME_MAX:
            error |= ERROR_TOO_LARGE
            continue
        sizes[i] = size
        msgs.append((i, m))
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(sizes, dtype=np.uint64, out=offsets[1:])
    need = int(offsets[n])
    cap = need if capacity is None else int(capacity)
    written = min(need, cap)
    frames = np.zeros(0, np.uint8)
    if not sizing:
        data, so = codec.serialize_messages([m for _, m in msgs])
        if not np.array_equal(np.diff(so).astype(np.uint32), sizes[[i for i, _ in msgs]]):
            raise AssertionError("frame_size_np disagrees with the host serializer")
        frames = data[:written].copy()  # the empty frames hold no bytes: the rest is already in order
    n_complete = int(np.count_nonzero(offsets[1:] <= cap))
    return frames, offsets, sizes, dict(n_frames=n, n_complete=n_complete, bytes_need=need, bytes_written=written,
                                        overflow=int(need > cap), error=error)


# ---- messages that carry records: RecordReply frames read from the payload slab ----
# Error bits beyond the flat builder's 0 - 3, and the flag of the call.
ERROR_HANDLE = 16        # bit 4: a handle >= n_entries or an entry that is not live: the record is left out
ERROR_ARENA = 32         # bit 5: an entry's payload range leaves the arena: that payload is present and empty
ERROR_ROWS = 64          # bit 6: row_offsets descend or pass n_handles: the row is clamped
SKIP_EMPTY = 1           # flags bit 0: a message without a record is an empty frame of size 0

_REC_VTABLE = (10, 12, 14, 14)   # by (data, flex): the record's highest slot decides


def record_shape(has_data, has_flex, has_position) -> int:
    """A record's shape, 0 .. 7: bit 0 data, bit 1 flex, bit 2 position. Its vtable depends on nothing else."""
    return (1 if has_data else 0) | (2 if has_flex else 0) | (4 if has_position else 0)


def record_frame_size_np(has_position, instruction, replication, world_len, param_len=None, flex_len=None, records=()) -> int:
    """Size of the frame of a message with these fields whose `records` are (shape, world_len, data_len,
    flex_len) in row order and whose entities are empty, in closed form. The records come after the world
    string, record 0 first, each as the builder pushes it: the uuid string (the only push whose padding
    depends on what came before: a vtable of 10 or 14 bytes leaves the fill at 2 mod 4 and the next align
    absorbs it), the world string, data, flex, the table (an offset per string, the position's 24 bytes, the
    soffset) and, at the shape's first occurrence in the frame only, the vtable. The offsets vector absorbs
    the last residue; the rest is frame_size_np's flat frame."""
    size, residue, seen = 0, 0, 0
    for shape, wl, dl, fl in records:
        size += (3 if residue == 0 else 1) + 37 + 4                   # align(37, 4), NUL + text, length
        size += _up4(int(wl) + 1) + 4
        if shape & 1:
            size += _up4(int(dl) + 1) + 4
        if shape & 2:
            size += _up4(int(fl)) + 4
        size += 4 * (2 + (shape & 1) + ((shape >> 1) & 1)) + (24 if shape & 4 else 0) + 4
        residue = 0
        if not seen >> shape & 1:
            seen |= 1 << shape
            vt = _REC_VTABLE[shape & 3]
            size += vt
            residue = vt & 3
    size += residue + 4 * len(records)                                 # the offsets vector: align(4 n, 4), n offsets
    return size + frame_size_np(has_position, instruction, replication, world_len, param_len, flex_len)


def clamp_rows_np(row_offsets, n_handles: int):
    """How the record builder reads row_offsets[n + 1] (u32) over n_handles handles, which is how the send side
    reads a CSR (interest._walk_rows): row i is the part of [off[i], off[i + 1]) inside [0, n_handles), empty when
    off[i + 1] < off[i], and the rows together are walked for at most n_handles elements. Returns ([(start,
    stop)], cut)."""
    from .interest import _walk_rows
    rows, _, err = _walk_rows(row_offsets, n_handles)
    return [(a, a + ln) for a, ln in rows], bool(err)


def build_record_frames_np(worlds, sender_uuid, world, row_offsets, handles, entries, payload, instruction=0, replication=0,
                           pos=None, param=None, param_offsets=None, flex=None, flex_offsets=None, msg_flags=None,
                           world_bytes=None, world_off=None, world_len=None, flags=0, capacity=None,
                           n_payload_bytes=None):
    """The definition of wq_frames_build_records_device: build_frames_np's message, plus per message the
    records of a CSR row of slab handles (row_offsets u32[n + 1], handles u32; entries abi.SLAB_ENTRY_DTYPE and
    payload u8: the slab of records.slab_store_np), entities empty. Returns build_frames_np's tuple.

    Beyond build_frames_np's rules: sender_uuid None is the nil uuid; world_bytes / world_off (u64[n]) /
    world_len (u32[n]) give every message's world name as bytes and replace `world` (a range that leaves
    world_bytes: an empty name, error bit 0); a handle outside the entries or whose entry is not live is left
    out of the frame (bit 4); data at [off, off + data_len) or flex at [off + data_len, off + data_len +
    flex_len) leaving the arena is present and empty (bit 5); rows are read as clamp_rows_np reads them (bit
    6); an entry's world id outside the table gives an empty name (bit 0); the same handle twice gives the
    record twice; with flags & SKIP_EMPTY a message that is left without a record is an empty frame.
    n_payload_bytes stands in for the arena's length in a sizing call (capacity 0) without arena memory."""
    from . import abi, codec
    n = len(row_offsets) - 1
    world = np.zeros(n, np.uint32) if world is None else np.ascontiguousarray(world, dtype=np.uint32)
    uu = np.zeros((n, 16), np.uint8) if sender_uuid is None else np.ascontiguousarray(sender_uuid, dtype=np.uint8).reshape(-1, 16)
    if len(world) != n or len(uu) != n:
        raise ValueError("one row, one world and 16 uuid bytes per message")
    if (param is None) != (param_offsets is None) or (flex is None) != (flex_offsets is None):
        raise ValueError("a payload and its offsets are given together or not at all")
    names = [w if isinstance(w, (bytes, bytearray)) else w.encode("utf-8") for w in (worlds or [])]
    ins, rep = _per_message(instruction, n, "instruction"), _per_message(replication, n, "replication")
    p3 = None if pos is None else np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    given = (HAS_POSITION if p3 is not None else 0) | (HAS_PARAMETER if param is not None else 0) | \
        (HAS_FLEX if flex is not None else 0)
    mflags = np.full(n, given, np.uint8) if msg_flags is None else np.ascontiguousarray(msg_flags, np.uint8) & given
    pay = {}
    for key, data, off in (("parameter", param, param_offsets), ("flex", flex, flex_offsets)):
        if data is not None:
            data = np.ascontiguousarray(data, dtype=np.uint8)
            pay[key] = (data, np.ascontiguousarray(off, dtype=np.uint64), len(data))
    handles = np.ascontiguousarray(handles, dtype=np.uint32)
    entries = np.ascontiguousarray(entries, dtype=abi.SLAB_ENTRY_DTYPE)
    arena = np.ascontiguousarray(payload if payload is not None else [], dtype=np.uint8)
    n_arena = len(arena) if n_payload_bytes is None else int(n_payload_bytes)
    wb = None if world_bytes is None else np.ascontiguousarray(world_bytes, dtype=np.uint8)
    sizing = capacity is not None and int(capacity) == 0
    rows, cut = clamp_rows_np(row_offsets, len(handles))
    error, msgs, sizes = ERROR_ROWS if cut else 0, [], np.zeros(n, dtype=np.uint32)
    for i in range(n):
        if wb is not None:
            a, ln = int(world_off[i]), int(world_len[i])
            if a + ln > len(wb):
                error |= ERROR_WORLD
                a = ln = 0
            name = wb[a:a + ln].tobytes()
        else:
            w = int(world[i])
            if w >= len(names):
                error |= ERROR_WORLD
            name = names[w] if w < len(names) else b""
        m = dict(instruction=int(ins[i]), replication=int(rep[i]), sender_uuid=uu[i].tobytes(), world_name=name)
        lens = {}
        for key, bit, err in (("parameter", HAS_PARAMETER, ERROR_PARAM), ("flex", HAS_FLEX, ERROR_FLEX)):
            if mflags[i] & bit:
                data, off, nb = pay[key]
                a, ln, ok = _range(off, i, nb)
                if not ok:
                    error |= err
                lens[key] = ln
                m[key] = data[a:a + ln].tobytes()
        if mflags[i] & HAS_POSITION:
            m["position"] = p3[i]
        recs, shapes = [], []
        for hd in handles[rows[i][0]:rows[i][1]]:
            if int(hd) >= len(entries) or not int(entries[int(hd)]["bits"]) & abi.SLAB_LIVE:
                error |= ERROR_HANDLE
                continue
            e = entries[int(hd)]
            bits, off, dl, fl = int(e["bits"]), int(e["off"]), int(e["data_len"]), int(e["flex_len"])
            if bits & abi.SLAB_DATA and off + dl > n_arena:
                error |= ERROR_ARENA
                d_at, d_len = 0, 0
            else:
                d_at, d_len = off, dl if bits & abi.SLAB_DATA else 0
            if bits & abi.SLAB_FLEX and off + dl + fl > n_arena:
                error |= ERROR_ARENA
                f_at, f_len = 0, 0
            else:
                f_at, f_len = off + dl, fl if bits & abi.SLAB_FLEX else 0
            w = int(e["world"])
            if w >= len(names):
                error |= ERROR_WORLD
            rname = names[w] if w < len(names) else b""
            shapes.append((record_shape(bits & abi.SLAB_DATA, bits & abi.SLAB_FLEX, bits & abi.SLAB_POSITION), len(rname), d_len, f_len))
            recs.append(dict(uuid=bytes(e["uuid"]), world_name=rname, position=tuple(e["pos"]) if bits & abi.SLAB_POSITION else None,
                             data=(b"" if sizing else arena[d_at:d_at + d_len].tobytes()) if bits & abi.SLAB_DATA else None,
                             flex=(b"" if sizing else arena[f_at:f_at + f_len].tobytes()) if bits & abi.SLAB_FLEX else None))
        if not recs and flags & SKIP_EMPTY:
            continue
        m["records"] = recs
        size = record_frame_size_np(bool(mflags[i] & HAS_POSITION), m["instruction"], m["replication"], len(name),
                                    lens.get("parameter"), lens.get("flex"), shapes)
        if size > FRAME_MAX:
            error |= ERROR_TOO_LARGE
            continue
        sizes[i] = size
        msgs.append((i, m))
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(sizes, dtype=np.uint64, out=offsets[1:])
    need = int(offsets[n])
    cap = need if capacity is None else int(capacity)
    written = min(need, cap)
    frames = np.zeros(0, np.uint8)
    if not sizing:
        data, so = codec.serialize_messages([m for _, m in msgs])
        if not np.array_equal(np.diff(so).astype(np.uint32), sizes[[i for i, _ in msgs]]):
            raise AssertionError("record_frame_size_np disagrees with the host serializer")
        frames = data[:written].copy()
    n_complete = int(np.count_nonzero(offsets[1:] <= cap))
    return frames, offsets, sizes, dict(n_frames=n, n_complete=n_complete, bytes_need=need, bytes_written=written,
                                        overflow=int(need > cap), error=error)
