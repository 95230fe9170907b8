"""Frame builder, the host side (include/wq_router.h, "frame builder"; kernels: csrc/wq_frames.hip).

`build_frames_np` is the definition of what wq_frames_build_device writes: it applies the call's
malformed-input rules to numpy inputs and hands the resulting flat messages to the host serializer
(codec.serialize_messages, the restatement of Message::serialize), so the device's frames are checked
byte for byte against the bytes every decoder and client already takes. `frame_size_np` is the size of
a flat frame in closed form. `world_table` lays a list of names out as wq_frames_set_worlds takes them
and `FramesSrc` is struct wq_frames_src.
"""
from __future__ import annotations

import numpy as np

from .abi import (FRAMES_COUNTERS_DTYPE, FRAMES_ERROR_FLEX as ERROR_FLEX, FRAMES_ERROR_PARAM as ERROR_PARAM,  # noqa: F401
                  FRAMES_ERROR_TOO_LARGE as ERROR_TOO_LARGE, FRAMES_ERROR_WORLD as ERROR_WORLD,
                  FRAMES_HAS_FLEX as HAS_FLEX, FRAMES_HAS_PARAMETER as HAS_PARAMETER,
                  FRAMES_HAS_POSITION as HAS_POSITION, FRAME_MAX, FramesSrc)


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

