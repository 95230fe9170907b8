"""Host reference of the follow path (include/wq_router.h, wq_follow_peers): the subscription ops
that follow from "peer i is now in world w at position p", in plain numpy.

Semantics: with cube size s and reach r the neighbourhood of (w, p) is the set
of cubes from_vector3(p + s*d), d in {-r..r}^3 (one f64 add per axis). A follow call turns the
stored state (O = its neighbourhood, empty if not followed) and the new state (N, empty for
WORLD_INVALID) of every peer into UNSUBSCRIBE ops for O \\ N and SUBSCRIBE ops for N \\ O: an exact
set difference, per axis, with no shortcut for peers whose own cell did not change. The op stream
is ascending in the peer id; within a peer the unsubscribes come first, then the subscribes, each
in lexicographic (dx, dy, dz) order over the first offset that yields each distinct cube. Ops carry
the offset position (key_is_raw = 0), as a host handler would send them. `follow_ops_np` produces
the byte stream the GPU path (csrc/wq_follow.hip) must produce.

The quantiser here restates csrc/wq_device.hpp coord_clamp_dev op for op; it is the package's own
(the product path imports nothing from the test infrastructure).
"""
from __future__ import annotations

import numpy as np

from . import abi

MAX_REACH = 2

_I64_MAX = np.iinfo(np.int64).max
_I64_MIN = np.iinfo(np.int64).min


def _sat_i64(x: np.ndarray) -> np.ndarray:
    """Rust `f64 as i64` (wq_device.hpp sat_i64): toward zero, saturating, NaN -> 0."""
    nan = np.isnan(x)
    hi = x >= 9223372036854775808.0
    lo = x <= -9223372036854775808.0
    t = np.where(nan | hi | lo, 0.0, x)
    v = np.trunc(t).astype(np.int64)
    v = np.where(hi, _I64_MAX, v)
    return np.where(lo, _I64_MIN, v)


def coord_clamp(c, cube_size: int) -> np.ndarray:
    """wq_device.hpp coord_clamp_dev over an array of coordinates (any shape), as int64."""
    c = np.asarray(c, dtype=np.float64)
    sf = np.float64(cube_size)
    si = np.uint64(cube_size)
    with np.errstate(all="ignore"):
        a = np.abs(c)
        q = a / sf
        is_mult = (np.fmod(a, sf) == 0.0) & (c != 0.0)  # fmod is exact; inf / NaN give NaN: false
        r = np.where(a == 0.0, sf, np.ceil(q) * sf)
        res = _sat_i64(np.where(is_mult, c, r))
        add = ~is_mult & ~(r > c)
        res = np.where(add, (res.view(np.uint64) + si).view(np.int64), res)
        neg = ~is_mult & (c < 0.0)
        res = np.where(neg, (np.uint64(0) - res.view(np.uint64)).view(np.int64), res)
    return res.astype(np.int64)


def _axis_masks(vo, vn, old_ok, new_ok, same):
    """Per axis: which offsets are the first to yield their value (distinct), and which of those
    values the other side's list holds too (present). vo, vn: (n, R) quantised values."""
    R = vo.shape[1]
    d_o = np.ones(vo.shape, bool)
    d_n = np.ones(vn.shape, bool)
    for j in range(1, R):
        d_o[:, j] = ~(vo[:, j, None] == vo[:, :j]).any(1)
        d_n[:, j] = ~(vn[:, j, None] == vn[:, :j]).any(1)
    d_o &= old_ok[:, None]
    d_n &= new_ok[:, None]
    i_o = d_o & (vo[:, :, None] == vn[:, None, :]).any(2) & same[:, None]
    i_n = d_n & (vn[:, :, None] == vo[:, None, :]).any(2) & same[:, None]
    return d_o, i_o, d_n, i_n


def follow_ops_np(old_world, old_pos, new_world, new_pos, cube_size: int, reach: int = 1) -> np.ndarray:
    """The ops of one follow call over peers 0 .. n-1 (abi.OP_DTYPE, in stream order)."""
    if not 0 <= reach <= MAX_REACH:
        raise ValueError("reach must be 0, 1 or 2")
    ow = np.ascontiguousarray(old_world, dtype=np.uint32)
    nw = np.ascontiguousarray(new_world, dtype=np.uint32)
    n = len(nw)
    op_ = np.ascontiguousarray(old_pos, dtype=np.float64).reshape(-1, 3)
    np_ = np.ascontiguousarray(new_pos, dtype=np.float64).reshape(-1, 3)
    if not (len(ow) == len(op_) == len(np_) == n):
        raise ValueError("old and new state must cover the same peers")
    if n == 0:
        return np.zeros(0, abi.OP_DTYPE)
    R = 2 * reach + 1
    step = float(cube_size) * np.arange(-reach, reach + 1, dtype=np.float64)   # s*d, exact
    old_ok = ow != abi.WORLD_INVALID
    new_ok = nw != abi.WORLD_INVALID
    same = old_ok & new_ok & (ow == nw)
    with np.errstate(all="ignore"):
        po = op_[:, :, None] + step[None, None, :]                             # (n, 3, R)
        pn = np_[:, :, None] + step[None, None, :]
    m = [_axis_masks(coord_clamp(po[:, ax], cube_size), coord_clamp(pn[:, ax], cube_size), old_ok, new_ok, same)
         for ax in range(3)]

    def grid(k):  # (n, R, R, R): axis masks combined over (dx, dy, dz)
        return m[0][k][:, :, None, None] & m[1][k][:, None, :, None] & m[2][k][:, None, None, :]

    un = (grid(0) & ~grid(1)).reshape(n, -1)
    su = (grid(2) & ~grid(3)).reshape(n, -1)
    parts = []
    for mask, world, p, kind in ((un, ow, po, abi.OP_UNSUBSCRIBE), (su, nw, pn, abi.OP_SUBSCRIBE)):
        peer, flat = np.nonzero(mask)                                          # peer, then (dx, dy, dz)
        ix, iy, iz = flat // (R * R), (flat // R) % R, flat % R
        pos = np.stack([p[peer, 0, ix], p[peer, 1, iy], p[peer, 2, iz]], 1)
        parts.append(abi.ops_array(world[peer], peer.astype(np.uint32), np.full(len(peer), kind, np.uint8), pos=pos))
    ops = abi.concat_ops(parts)
    # ascending peer; within a peer the unsubscribes (the first part) before the subscribes
    order = np.argsort(ops["peer"].astype(np.int64) * 2 + (ops["kind"] == abi.OP_SUBSCRIBE), kind="stable")
    # reordered as raw 40-byte records: indexing the structured array would not carry the padding
    return np.ascontiguousarray(ops.view(np.uint8).reshape(-1, 40)[order]).reshape(-1).view(abi.OP_DTYPE)


class FollowState:
    """The handle's follow state on the host: feed it the arrays of each follow call, get the ops."""

    def __init__(self, cube_size: int = 16, reach: int = 1):
        self.cube_size = cube_size
        self.reach = reach
        self.world = np.zeros(0, np.uint32)
        self.pos = np.zeros((0, 3), np.float64)

    def reset(self) -> None:
        self.world = np.zeros(0, np.uint32)
        self.pos = np.zeros((0, 3), np.float64)

    def n_followed(self) -> int:
        return int((self.world != abi.WORLD_INVALID).sum())

    def follow(self, world, pos) -> np.ndarray:
        world = np.ascontiguousarray(world, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        n = len(world)
        if n > len(self.world):  # peers never seen are not followed
            grow = n - len(self.world)
            self.world = np.concatenate([self.world, np.full(grow, abi.WORLD_INVALID, np.uint32)])
            self.pos = np.concatenate([self.pos, np.zeros((grow, 3))])
        ops = follow_ops_np(self.world[:n], self.pos[:n], world, pos, self.cube_size, self.reach)
        self.world[:n] = world
        self.pos[:n] = pos
        return ops
