"""Table snapshots: the subscription table as a canonical op stream (include/wq_router.h,
wq_table_export), its host definition and the snapshot file.

`TableRef` is the definition of what a handle holds and exports: a plain-Python model that applies
ops in array order with the reference's semantics (processing/thread.rs:122-146) — for each (world,
cube, peer) the last op wins, a REMOVE_PEER op removes what its peer holds at that point, in one
world or in every world — and whose `export` gives the rows of wq_table_export: one SUBSCRIBE op
with key_is_raw = 1 per live (world, cube, peer), ascending by (world, key x, y, z as i64, peer).
Two tables holding the same set export the same bytes; importing is applying the rows to an empty
table. The quantiser is follow.coord_clamp (csrc/wq_device.hpp coord_clamp_dev op for op).

`save` / `load` keep one .npz: cube size, the rows, the follow reach and the follow state
(wq_follow_state_read / _load). `take` and `restore` move a Router's state through a `Snapshot`.
The ids in the rows mean something only together with the host maps that made them: see
subscriptions.WorldMap.snapshot / restore.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import abi
from .follow import coord_clamp


def _rows(world, peer, key) -> np.ndarray:
    """Export rows from parallel arrays (already in canonical order)."""
    n = len(world)
    out = np.zeros(n, dtype=abi.OP_DTYPE)  # zeroed: the padding bytes are part of the contract
    out["world"] = world
    out["peer"] = peer
    out["kind"] = abi.OP_SUBSCRIBE
    out["key_is_raw"] = 1
    out["key"] = np.asarray(key, dtype=np.int64).reshape(n, 3)
    return out


def _contiguous(rows) -> np.ndarray:
    """Export rows as one contiguous OP_DTYPE array with their bytes intact. numpy copies a structured
    array field by field, which leaves the padding bytes of the copy unset: such a copy starts from
    zeros here, as exported rows have them."""
    rows = np.asarray(rows)
    if rows.dtype == abi.OP_DTYPE and rows.flags.c_contiguous:
        return rows
    buf = np.zeros(len(rows), dtype=abi.OP_DTYPE)
    for name in ("world", "peer", "kind", "key_is_raw", "key"):
        buf[name] = rows[name]
    return buf


def sort_rows(rows: np.ndarray) -> np.ndarray:
    """Export rows (e.g. the concatenation of several shards' exports) in canonical order."""
    rows = _contiguous(rows)
    k = rows["key"]
    order = np.lexsort((rows["peer"], k[:, 2], k[:, 1], k[:, 0], rows["world"]))
    return np.ascontiguousarray(rows.view(np.uint8).reshape(-1, 40)[order]).reshape(-1).view(abi.OP_DTYPE)


class TableRef:
    """The subscription table on the host: {(world, kx, ky, kz): set of peers}."""

    def __init__(self, cube_size: int = 16):
        self.cube_size = cube_size
        self.cubes: dict = {}   # (world, kx, ky, kz) -> set of peers; emptied cubes are dropped
        self.held: dict = {}    # peer -> set of (world, kx, ky, kz)

    def apply(self, ops: np.ndarray) -> None:
        ops = np.ascontiguousarray(ops, dtype=abi.OP_DTYPE)
        if len(ops) == 0:
            return
        raw = ops["key_is_raw"] != 0
        keys = np.where(raw[:, None], ops["key"], coord_clamp(np.where(raw[:, None], 0.0, ops["pos"]), self.cube_size))
        for world, peer, kind, k in zip(ops["world"].tolist(), ops["peer"].tolist(), ops["kind"].tolist(),
                                        keys.tolist()):
            if kind == abi.OP_REMOVE_PEER:
                self.remove_peer(peer, None if world == abi.WORLD_INVALID else world)
                continue
            if world == abi.WORLD_INVALID:
                raise ValueError("the reserved world id in a subscribe / unsubscribe op")
            c = (world, k[0], k[1], k[2])
            if kind == abi.OP_SUBSCRIBE:
                self.cubes.setdefault(c, set()).add(peer)
                self.held.setdefault(peer, set()).add(c)
            elif kind == abi.OP_UNSUBSCRIBE:
                s = self.cubes.get(c)
                if s is not None and peer in s:
                    s.discard(peer)
                    if not s:
                        del self.cubes[c]
                    self.held[peer].discard(c)
            else:
                raise ValueError(f"unknown op kind {kind}")

    def remove_peer(self, peer: int, world: Optional[int] = None) -> None:
        mine = self.held.get(peer)
        if not mine:
            return
        for c in [c for c in mine if world is None or c[0] == world]:
            s = self.cubes[c]
            s.discard(peer)
            if not s:
                del self.cubes[c]
            mine.discard(c)

    def is_subscribed(self, world: int, peer: int, key) -> bool:
        return peer in self.cubes.get((world, int(key[0]), int(key[1]), int(key[2])), ())

    def counts(self) -> dict:
        return {"n_entries": sum(len(s) for s in self.cubes.values()), "n_cubes": len(self.cubes),
                "n_any": len({(c[0], p) for c, s in self.cubes.items() for p in s})}

    def export(self, world: Optional[int] = None, peers=None) -> np.ndarray:
        """The rows of wq_table_export: `world` None = every world, `peers` None = every peer, else
        exactly these ids (any order, duplicates and unknown ids allowed, may be empty)."""
        want = None if peers is None else {int(p) for p in peers}
        w, p, k = [], [], []
        for c in sorted(self.cubes):
            if world is not None and c[0] != world:
                continue
            for peer in sorted(self.cubes[c]):
                if want is None or peer in want:
                    w.append(c[0])
                    p.append(peer)
                    k.append(c[1:])
        return _rows(np.array(w, np.uint32), np.array(p, np.uint32), np.array(k, np.int64).reshape(-1, 3))

    def subscriptions_of(self, peer: int) -> np.ndarray:
        return self.export(peers=[peer])


@dataclass
class Snapshot:
    cube_size: int
    ops: np.ndarray                       # abi.OP_DTYPE, canonical order
    follow_reach: int = 1
    follow_world: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint32))
    follow_pos: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.float64))


def save(path, snap: Snapshot) -> None:
    """One .npz; the rows are stored as their raw bytes (the union layout of OP_DTYPE included)."""
    ops = _contiguous(snap.ops)
    with open(path, "wb") as f:
        np.savez(f, cube_size=np.uint32(snap.cube_size), ops=ops.view(np.uint8),
                 follow_reach=np.uint32(snap.follow_reach),
                 follow_world=np.ascontiguousarray(snap.follow_world, dtype=np.uint32),
                 follow_pos=np.ascontiguousarray(snap.follow_pos, dtype=np.float64).reshape(-1, 3))


def load(path, cube_size: Optional[int] = None) -> Snapshot:
    """Reads a snapshot; with `cube_size` (the target's) one taken on another grid is refused: raw
    keys of another cube size are meaningless."""
    with np.load(path) as z:
        snap = Snapshot(int(z["cube_size"]), z["ops"].copy().view(abi.OP_DTYPE), int(z["follow_reach"]),
                        z["follow_world"].copy(), z["follow_pos"].copy())
    if cube_size is not None and cube_size != snap.cube_size:
        raise ValueError(f"snapshot of cube_size {snap.cube_size} cannot be loaded into a table of cube_size {cube_size}")
    return snap


def take(router, follow_reach: int = 1) -> Snapshot:
    """The whole state of a Router: every subscription and the follow state. The reach is the
    caller's (the handle has no getter for it)."""
    w, p = router.follow_state()
    return Snapshot(router.cube_size, router.export_table(), follow_reach, w, p)


def restore(router, snap: Snapshot, sharded: bool = False) -> None:
    """Into an empty Router of the same cube size: the rows through the ordinary apply (every shard
    of a sharded set is given the same rows: sharded=True), then the reach and the follow state."""
    if snap.cube_size != router.cube_size:
        raise ValueError(f"snapshot of cube_size {snap.cube_size} cannot be loaded into a table of cube_size "
                         f"{router.cube_size}")
    if len(snap.ops):
        (router.sharded_apply_ops if sharded else router.apply_ops)(snap.ops)
    router.follow_set_reach(snap.follow_reach)
    if len(snap.follow_world):
        router.follow_state_load(snap.follow_world, snap.follow_pos)
