"""Ingest, the host side (include/wq_router.h, "ingest"; kernels: csrc/wq_decode.hip).

`decode_frames_np` is the definition of what wq_frames_decode_device writes: the host decoder
(codec.decode_packed, the restatement of Message::deserialize) under the call's rules for frame
offsets, then per message what processing.py does one event at a time — "@global", the world-name
sanitizer (world_names.py), the world table, the sender table — plus the flags, the counters and
`flex_range`, which comes from a small walk of its own over a frame the decoder has already accepted.
`Router.set_ingest_peers` / `Router.decode_frames_device` (router.py) are the device call's bindings,
`abi.IngestOut` and `abi.INGEST_COUNTERS_DTYPE` its structs. `IngestTick` keeps the device arrays of a
tick and hands them to `Router.route_device` with nothing read back in between.
"""
from __future__ import annotations

import struct
import uuid as _uuid

import numpy as np

from . import abi, codec
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


class IngestTick:
    """The device arrays of one tick's decode, grow-only, and the step from received frames to
    Router.route_device: decode(frames, offsets) enqueues wq_frames_decode_device, route(...) the tick on
    the arrays it left, and nothing is read back or waited for between the two. read() is for tests and
    for the host's share of the tick (the counters, the unknown senders' uuids)."""

    _SPEC = dict(msg=(72, np.uint8), pos=(24, np.uint8), world=(4, np.uint8), sender=(4, np.uint8), repl=(1, np.uint8),
                 instruction=(1, np.uint8), sender_uuid=(16, np.uint8), flex_range=(8, np.uint8), flags=(1, np.uint8))

    def __init__(self, router, capacity: int = 1024, device: str = "cuda:0"):
        import torch
        self.router, self.device, self.cap, self.n = router, device, 0, 0
        self.buf: dict = {}
        self.counters = torch.zeros(INGEST_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=device)
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
