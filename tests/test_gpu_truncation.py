"""What a tick writes when its pairs exceed the caller's `capacity` (wq_route_tick[_device],
wq_route_global[_device]): a guard-checked capacity sweep over every tick shape.

Bars, all bit-exact against the CPU oracle (COracle.route / route_radius / route_global):
  - offsets[0 .. M] are complete whatever the capacity (offsets[M] = P, not clipped);
  - peers / msgs hold exactly the first min(P, capacity) pairs of the full result;
  - nothing is written at or past `capacity`: the buffers are filled with a canary word that is no
    peer id and no message index, and are P + 4096 words long whatever the capacity, so a kernel
    that ignored `capacity` would fail an assertion here, never touch foreign memory;
  - the counters carry the full P and F, overflow = (P > capacity), error = 0, and wq_route_health
    reports the overflow once.

The workload (one world, cube size 16, 40 light cubes on both sides of the inline boundary, one
hot cube of 700 peers, 6 * 256 + 77 messages planned per 256-message block) makes every block class
of every emit shape appear in one small tick; `check_workload` asserts that from the oracle's result
alone (tests/test_truncation_workload.py runs it without a GPU). The capacities come from the
oracle's offsets: buffer ends, block starts, window edges of the emit kernels, quad-aligned image
edges, and the middle of a long, a short and an OnlySelf message.

The production form of a long tick (two 256-message tiles per workgroup, WQ_DEBUG_COUNT_TPB /
WQ_DEBUG_EMIT_BPB) and the tick that writes the caller's counters itself (WQ_TICK_OUTCNT) are read
from the environment once per process: they run in child processes, one per row.
"""
import ctypes
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle as orc
from worldql_server_amd import abi, interest, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CANARY = 0xA5A5A5A5   # no peer id (< 2^16 here) and no message index
SLACK = 4096          # words behind P in peers / msgs, whatever the capacity
OFF_GUARD = 64        # words behind offsets[M]
CUBE = 16
KINLINE = 24          # csrc kInline: peers held inside a cube's record
BLOCK = 256
SEED = 26
RADIUS = 9.0

LIGHT = [1, 3, 8, 12, 23, 24, 25, 40]
N_LIGHT, N_HOT = 40, 700
HOT, EMPTY = N_LIGHT, N_LIGHT + 1   # cube indices along the row
M_TOTAL = 6 * BLOCK + 77
UNKNOWN_PEER = 5000                 # an id nobody holds
UNKNOWN_WORLD = 1


# ---- workload (CPU only) ------------------------------------------------------------------

def workload(seed=SEED, repl_codes=(0, 1, 2)):
    """Subscriptions and one tick of messages; see the module docstring and check_workload."""
    rng = synth.SplitMix64(0x7B0C0000 + seed)
    per = [LIGHT[i % len(LIGHT)] for i in range(N_LIGHT)] + [N_HOT, 0]   # ... the hot cube, the empty cube
    first = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)   # cube i holds peers first[i] .. first[i + 1]
    n_peers = int(first[-1])
    cube_of = np.repeat(np.arange(len(per)), per)
    sub_pos = np.stack([16.0 * cube_of + 8.0, np.full(n_peers, 8.0), np.full(n_peers, -8.0)], 1)
    ops = abi.ops_array(np.zeros(n_peers, np.uint32), np.arange(n_peers, dtype=np.uint32),
                        np.zeros(n_peers, np.uint8), pos=sub_pos)
    per = np.asarray(per)
    light = np.arange(N_LIGHT)
    le8, mid, ge23 = light[per[:N_LIGHT] <= 8], light[(per[:N_LIGHT] == 12) | (per[:N_LIGHT] == 23)], \
        light[per[:N_LIGHT] >= 23]

    def pick(pool, n):
        return pool[rng.below(len(pool), n)]

    cube = np.empty(M_TOTAL, np.int64)
    world = np.zeros(M_TOTAL, np.uint32)
    cube[0:256] = pick(le8, 256)                       # block 0: <= 8 peers
    cube[256:512] = pick(mid, 256)                     # block 1: 12 or 23 peers
    cube[512:768] = EMPTY                              # block 2: nobody receives ...
    world[512:768:2] = UNKNOWN_WORLD                   # ... an unknown world / a cube without subscriber
    cube[768:1024] = pick(ge23, 256)                   # block 3: >= 23 peers
    cube[1024:1280] = pick(le8, 256)                   # block 4: <= 8 peers, every fifth the hot cube
    cube[1024:1280:5] = HOT
    cube[1280:1536] = HOT                              # block 5: the hot cube only
    cube[1536:] = pick(ge23, M_TOTAL - 1536)           # block 6 (77 messages): >= 23 peers
    pos = np.stack([16.0 * cube + rng.uniform(0.5, 15.5, M_TOTAL), rng.uniform(0.5, 15.5, M_TOTAL),
                    -rng.uniform(0.5, 15.5, M_TOTAL)], 1)
    # two senders in three subscribe to the cube they write to, the rest are an id nobody holds
    n_in = np.maximum(per[cube], 1)
    member = first[cube] + (rng.next_u64(M_TOTAL) % n_in.astype(np.uint64)).astype(np.int64)
    inside = (rng.below(3, M_TOTAL) < 2) & (per[cube] > 0)
    sender = np.where(inside, member, UNKNOWN_PEER).astype(np.uint32)
    codes = np.asarray(repl_codes, dtype=np.uint8)
    repl = codes[rng.below(len(codes), M_TOTAL)]
    peer_pos = sub_pos + rng.uniform(-7.0, 7.0, 3 * n_peers).reshape(n_peers, 3)
    keys = orc.quantize_np(pos, CUBE)
    return SimpleNamespace(ops=ops, pos=pos, keys=keys, world=world, sender=sender, repl=repl, peer_pos=peer_pos,
                           n_peers=n_peers, M=M_TOTAL, cube=cube, per=per)


def _ref(offs, peers, F):
    offs = np.ascontiguousarray(offs, dtype=np.uint32)
    M = len(offs) - 1
    e = np.diff(offs.astype(np.int64))
    g0 = offs[0:M:BLOCK].astype(np.int64)
    T = np.diff(np.concatenate([g0, [int(offs[M])]]))
    return SimpleNamespace(offs=offs, peers=np.ascontiguousarray(peers, dtype=np.uint32),
                           msgs=np.repeat(np.arange(M, dtype=np.uint32), e), F=F, P=int(offs[M]), M=M, e=e, g0=g0, T=T)


def oracle_refs(w):
    """The oracle's results for the workload: plain and with the radius filter."""
    o = orc.COracle(CUBE)
    o.apply_ops(w.ops)
    plain = _ref(*o.route(w.pos, w.world, w.sender, w.repl))
    by_key = _ref(*o.route(None, w.world, w.sender, w.repl, keys=w.keys))
    radius = _ref(*o.route_radius(w.pos, w.world, w.sender, w.repl, w.peer_pos, RADIUS))
    return SimpleNamespace(plain=plain, by_key=by_key, radius=radius, oracle=o)


def check_workload(w, refs):
    """The conditions that keep the sweep from silently missing a path, from the oracle alone."""
    r = refs.plain
    L = np.where(w.world == 0, w.per[w.cube], 0)  # the list behind each message (0: unknown world, empty cube)
    assert r.P == len(r.peers) and (refs.by_key.offs == r.offs).all() and (refs.by_key.peers == r.peers).all()
    T = r.T
    assert len(T) == 7 and T.sum() == r.P
    assert (T == 0).any()
    assert ((T > 0) & (T <= 2048)).any()
    assert ((T > 3072) & (T <= 4096)).any()       # overflows every single-launch image, two windows of emit_map<8>
    assert ((T > 4096) & (T <= 8192)).any()
    assert (T > 8192).any()
    blk = np.arange(w.M) // BLOCK
    queued = (L > KINLINE) & (r.e >= KINLINE)     # a list outside the record, not reduced to OnlySelf
    assert any(0 < T[b] <= 2560 and queued[blk == b].any() for b in range(7))   # the queue inside a fitting image
    rem = set((r.g0 % 4).tolist())
    assert 0 in rem and len(rem - {0}) >= 2 and r.P % 4 != 0
    only_self = (w.repl == abi.REPL_ONLY_SELF) & (r.e == 1)
    assert (r.e == 0).any() and only_self.any()
    assert ((r.e > 1) & (r.e <= KINLINE) & (L <= KINLINE)).any() and (r.e > KINLINE).any()
    assert r.peers.max() < 1 << 16 and r.F > r.P
    q = refs.radius
    assert 0 < q.P < r.P and q.P % 4 != 0
    assert any(q.T[b] > 4096 and (L[blk == b] > 256).any() for b in range(7))   # windows + the re-filter loop
    assert ((q.T > 0) & (q.T <= 4096)).any()


def _kinds(w, r):
    """One message of each kind: e > 24, 1 < e <= 24, OnlySelf with e = 1."""
    only_self = np.flatnonzero((w.repl == abi.REPL_ONLY_SELF) & (r.e == 1))
    long_ = np.flatnonzero(r.e > KINLINE)
    short = np.flatnonzero((r.e > 1) & (r.e <= 12))   # from an inline record
    return [int(a[len(a) // 2]) for a in (long_, short, only_self) if len(a)]


def capacities(r, kinds=()):
    """The full capacity list, from the oracle's offsets (sorted, distinct, >= 0): the buffer's ends, every
    block start g0 - 1 .. g0 + 5 and middle, the window edges of the two emit_map forms (g0 + 2048, g0 + 4096)
    and the quad-aligned image edge of blocks past 4096 outputs, and the start, start + 1 and middle of
    the messages `kinds`."""
    P = r.P
    caps = [0, 1, 2, 3, 4, 5, 7, 8] + [P + d for d in (-5, -4, -3, -1, 0, 1, 7)]
    for g0, T in zip(r.g0.tolist(), r.T.tolist()):
        if T > 0:
            caps += [g0 + d for d in range(-1, 6)] + [g0 + T // 2, g0 + T // 2 + 1]
        if T > 4096:
            for d in (-1, 0, 1):
                caps += [g0 + 2048 + d, g0 + 4096 + d, (g0 & ~3) + 4096 + d]
    for m in kinds:
        caps += [int(r.offs[m]), int(r.offs[m]) + 1, int(r.offs[m]) + int(r.e[m]) // 2]
    return sorted({c for c in caps if c >= 0})


def short_capacities(r):
    """The first eight, the P group, and the block starts of one block per class."""
    P = r.P
    caps = [0, 1, 2, 3, 4, 5, 7, 8] + [P + d for d in (-5, -4, -3, -1, 0, 1, 7)]
    T = r.T
    for lo, hi in ((-1, 0), (0, 2048), (3072, 4096), (4096, 8192), (8192, 1 << 40)):
        b = np.flatnonzero((T > lo) & (T <= hi))
        if len(b):
            caps += [int(r.g0[b[0]]) + d for d in range(-1, 6)]
    return sorted({c for c in caps if c >= 0})


def alternate(caps, P):
    """The capacities in an order that alternates truncated and full ticks."""
    short = [c for c in caps if c < P]
    full = [c for c in caps if c >= P] or [P]
    out = []
    for i, c in enumerate(short):
        out += [c, full[i % len(full)]]
    return out + [c for c in full if c not in out]


# ---- harness (GPU) ------------------------------------------------------------------------

def _i32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.uint32 else a


class Tick:
    """The workload's inputs on the device and guarded output buffers sized for `P` pairs."""

    def __init__(self, w, P, keys=False):
        import torch
        self.torch = torch
        dev = torch.device("cuda:0")
        self.M = len(w.world)
        self.pos = None if keys else torch.from_numpy(np.ascontiguousarray(w.pos)).to(dev)
        self.keys = torch.from_numpy(np.ascontiguousarray(w.keys)).to(dev) if keys else None
        self.world, self.sender, self.repl = (torch.from_numpy(_i32(x)).to(dev) for x in (w.world, w.sender, w.repl))
        self.offs = torch.empty(self.M + 1 + OFF_GUARD, dtype=torch.int32, device=dev)
        self.peers = torch.empty(P + SLACK, dtype=torch.int32, device=dev)
        self.msgs = torch.empty(P + SLACK, dtype=torch.int32, device=dev)
        self.cnt = torch.empty(24, dtype=torch.uint8, device=dev)
        assert self.peers.data_ptr() % 16 == 0 and self.msgs.data_ptr() % 16 == 0
        self.fill()

    def fill(self):
        c = int(np.uint32(CANARY).view(np.int32))
        for t in (self.offs, self.peers, self.msgs):
            t.fill_(c)
        self.cnt.fill_(0xEE)
        self.torch.cuda.synchronize()

    def inputs(self):
        return (self.pos.data_ptr() if self.pos is not None else None, self.world.data_ptr(), self.sender.data_ptr(),
                self.repl.data_ptr(), self.M)

    def read(self):
        self.torch.cuda.synchronize()
        h = [t.cpu().numpy().view(np.uint32) for t in (self.offs, self.peers, self.msgs)]
        return h[0], h[1], h[2], self.cnt.cpu().numpy().view(abi.COUNTERS_DTYPE)[0]


def _same(got, want, what, ctx):
    if got.shape != want.shape or not (got == want).all():
        bad = np.flatnonzero(got != want) if got.shape == want.shape else [-1]
        raise AssertionError(f"{what} differ from the oracle at {ctx}: first at index {int(bad[0])} of {len(want)}, "
                             f"{len(bad)} in all")


def _untouched(a, start, what, ctx):
    tail = a[start:]
    if not (tail == CANARY).all():
        bad = np.flatnonzero(tail != CANARY)
        raise AssertionError(f"{what} written at or past its limit at {ctx}: index {start + int(bad[0])} "
                             f"(limit {start}), {len(bad)} words in all")


def check_outputs(offs, peers, msgs, ref, cap, ctx, with_msgs=True):
    """Complete offsets, the exact prefix and untouched canaries, on host copies of the guarded buffers."""
    M, n = ref.M, min(ref.P, cap)
    _same(offs[:M + 1], ref.offs, "offsets", ctx)
    _untouched(offs, M + 1, "offsets", ctx)
    _same(peers[:n], ref.peers[:n], "peers", ctx)
    _untouched(peers, n, "peers", ctx)   # from `capacity` on, and with P < capacity from P on
    if with_msgs:
        _same(msgs[:n], ref.msgs[:n], "msgs", ctx)
        _untouched(msgs, n, "msgs", ctx)
    else:
        _untouched(msgs, 0, "msgs (not passed)", ctx)


def run_tick(r, t, ref, cap, ctx, with_msgs=True, F=None, glob=False):
    """One device tick into the guarded buffers at `cap`: check_outputs, the counters and wq_route_health. Returns the counters.
    F: the expected n_candidates (None: not compared — the caller compares it between capacities)."""
    t.fill()
    msgs_ptr = t.msgs.data_ptr() if with_msgs else None
    if glob:
        r.route_global_device(t.world.data_ptr(), t.sender.data_ptr(), t.repl.data_ptr(), t.M, t.offs.data_ptr(),
                              t.peers.data_ptr(), msgs_ptr, cap, t.cnt.data_ptr())
    else:
        pos, world, sender, repl, M = t.inputs()
        r.route_device(pos, world, sender, repl, M, t.offs.data_ptr(), t.peers.data_ptr(), msgs_ptr, cap,
                       t.cnt.data_ptr(), keys_ptr=t.keys.data_ptr() if t.keys is not None else None)
    offs, peers, msgs, c = t.read()
    check_outputs(offs, peers, msgs, ref, cap, ctx, with_msgs)
    got = (int(c["n_pairs"]), int(c["overflow"]), int(c["error"]))
    assert got == (ref.P, int(ref.P > cap), 0), (ctx, got)
    if F is not None:
        assert int(c["n_candidates"]) == F, (ctx, int(c["n_candidates"]), F)
    assert r.route_health() == (0, int(ref.P > cap)), ctx
    assert r.route_health() == (0, 0), ctx
    return c


def sweep(r, t, ref, caps, tag, with_msgs=True, F=None, glob=False):
    """Every capacity of `caps` on one handle, truncated and full ticks alternating. With F None
    n_candidates must still be one value, that of a full-capacity tick."""
    seen = set()
    for cap in alternate(caps, ref.P):
        c = run_tick(r, t, ref, cap, f"{tag}, capacity {cap} (P = {ref.P})", with_msgs, F, glob)
        seen.add(int(c["n_candidates"]))
    assert len(seen) == 1, (tag, "n_candidates depends on the capacity", sorted(seen))
    return seen.pop()


def mk_router(w):
    from worldql_server_amd.router import Router
    r = Router(CUBE, 0)
    r.apply_ops(w.ops)
    return r


@pytest.fixture(scope="module")
def base():
    """The workload, its oracle results and capacity lists, computed once and left unchanged."""
    w = workload()
    refs = oracle_refs(w)
    check_workload(w, refs)
    kinds = _kinds(w, refs.plain)
    assert len(kinds) == 3
    w3 = workload(repl_codes=(3, 4, 255))
    o = orc.COracle(CUBE)
    o.apply_ops(w3.ops)
    ref3 = _ref(*o.route(w3.pos, w3.world, w3.sender, w3.repl))
    assert ref3.P > 8192 and ref3.P != refs.plain.P
    return SimpleNamespace(w=w, refs=refs, ref=refs.plain, caps=capacities(refs.plain, kinds),
                           short=short_capacities(refs.plain), w3=w3, ref3=ref3)


def _n_configs():
    from worldql_server_amd.router import load_library
    return int(load_library().wq_debug_route_config_count())


# ---- every config -----------------------------------------------------------------------

@pytest.mark.parametrize("cfg", range(14))
def test_every_config_full_capacity_list(base, cfg):
    """Config `cfg` (the table in csrc/wq_route.hip) over the full capacity list, msgs on, positions."""
    assert _n_configs() == 14, "a route config was added or removed: extend the parametrisation to match"
    r = mk_router(base.w)
    r.set_route_config(cfg)
    sweep(r, Tick(base.w, base.ref.P), base.ref, base.caps, f"config {cfg}", F=base.ref.F)
    r.close()


# ---- shorter cases ----------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [0, 1, 7, 10])
def test_without_msgs(base, cfg):
    """d_msgs = NULL (the kernels' `if (o.msgs)` branches): the msgs buffer stays canary throughout."""
    r = mk_router(base.w)
    r.set_route_config(cfg)
    sweep(r, Tick(base.w, base.ref.P), base.ref, base.short, f"config {cfg}, no msgs", with_msgs=False, F=base.ref.F)
    r.close()


@pytest.mark.parametrize("cfg", [0, 10])
def test_raw_keys(base, cfg):
    """Raw cube keys instead of positions (the RAW_KEYS instantiations)."""
    r = mk_router(base.w)
    r.set_route_config(cfg)
    sweep(r, Tick(base.w, base.ref.P, keys=True), base.refs.by_key, base.short, f"config {cfg}, raw keys",
          F=base.refs.by_key.F)
    r.close()


@pytest.mark.parametrize("cfg", [0, 10])
def test_unknown_replication_codes(base, cfg):
    """Codes 3, 4 and 255: every one is ExceptSelf (replication.rs:40)."""
    r = mk_router(base.w3)
    r.set_route_config(cfg)
    sweep(r, Tick(base.w3, base.ref3.P), base.ref3, short_capacities(base.ref3), f"config {cfg}, codes 3/4/255",
          F=base.ref3.F)
    r.close()


# ---- heavy shapes -------------------------------------------------------------------------

@pytest.mark.parametrize("chunks", [0, 2, 3])
def test_heavy_shape_and_pipelined_chunks(base, chunks):
    """Config 0 under wq_set_fanout_hint(40) (count / scan / emit_map), plain and in 2 and 3 pipelined
    chunks (each chunk's emit offsets its msgs by the chunk's first message), against the oracle."""
    r = mk_router(base.w)
    r.set_fanout_hint(40.0)
    assert r.route_shape() == (True, False)
    n_count = (base.w.M + BLOCK - 1) // BLOCK
    assert n_count == 7 and n_count >= 2 * chunks   # wq_route.hip: the pipelined path is taken from 2 tiles per chunk
    r.set_route_chunks(chunks)
    sweep(r, Tick(base.w, base.ref.P), base.ref, base.caps, f"heavy shape, chunks {chunks}", F=base.ref.F)
    r.close()


# ---- radius -------------------------------------------------------------------------------

def test_radius_filter(base):
    """count_radius / emit_kernel<RADIUS>: several image windows and the block-wide re-filter of a
    700-peer list, capacities from the radius oracle's offsets; then the radius off again."""
    w, ref = base.w, base.refs.radius
    r = mk_router(w)
    r.set_peer_positions(w.peer_pos)
    r.set_radius(RADIUS)
    t = Tick(w, base.ref.P)
    F = sweep(r, t, ref, capacities(ref, _kinds(w, ref)), "radius 9")
    assert F >= ref.P
    r.set_radius(0.0)
    run_tick(r, t, base.ref, base.ref.P, "radius off again", F=base.ref.F)
    r.close()


# ---- global -------------------------------------------------------------------------------

def _global_case():
    world = np.array([0, 0, UNKNOWN_WORLD, 0, 0, 0], np.uint32)
    sender = np.array([5, UNKNOWN_PEER, 7, 900, UNKNOWN_PEER, 40], np.uint32)   # inside and outside the world
    repl = np.array([abi.REPL_EXCEPT_SELF, 7, abi.REPL_INCLUDING_SELF, abi.REPL_ONLY_SELF, abi.REPL_ONLY_SELF,
                     abi.REPL_INCLUDING_SELF], np.uint8)
    return SimpleNamespace(world=world, sender=sender, repl=repl, pos=np.zeros((6, 3)), keys=np.zeros((6, 3), np.int64))


def _global_ref(o, g):
    offs, peers = o.route_global(g.world, g.sender, g.repl)
    return _ref(offs, peers, None)


def _global_caps(ref):
    P = ref.P
    caps = [0, 1, P - 1, P, P + 1] + [int(x) + d for x in ref.offs for d in (-1, 0, 1)]
    return sorted({c for c in caps if c >= 0})


def test_global_device(base):
    """wq_route_global_device (global_copy_kernel): all three replication modes and an unknown code,
    senders inside and outside the world, an unknown world; every offset +- 1 as the capacity."""
    g = _global_case()
    ref = _global_ref(base.refs.oracle, g)
    n = base.w.n_peers
    assert ref.offs.tolist() == [0, n - 1, 2 * n - 1, 2 * n - 1, 2 * n, 2 * n, 3 * n]
    r = mk_router(base.w)
    sweep(r, Tick(g, ref.P), ref, _global_caps(ref), "global", glob=True)
    r.close()


# ---- host forms ---------------------------------------------------------------------------

def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_tick(r, w, ref, cap, ctx, glob=False, keys=False):
    """lib.wq_route_tick / wq_route_global on guarded numpy buffers (Router.route retries or raises)."""
    offs = np.full(ref.M + 1 + OFF_GUARD, CANARY, np.uint32)
    peers = np.full(ref.P + SLACK, CANARY, np.uint32)
    msgs = np.full(ref.P + SLACK, CANARY, np.uint32)
    n = ctypes.c_size_t(12345)
    world, sender, repl = (np.ascontiguousarray(x) for x in (w.world, w.sender, w.repl))
    if glob:
        rc = r.lib.wq_route_global(r.h, _p(world), _p(sender), _p(repl), ref.M, _p(offs), _p(peers), _p(msgs), cap,
                                   ctypes.byref(n))
    else:
        pos = None if keys else np.ascontiguousarray(w.pos, dtype=np.float64)
        k = np.ascontiguousarray(w.keys, dtype=np.int64) if keys else None
        rc = r.lib.wq_route_tick(r.h, _p(pos), _p(k), _p(world), _p(sender), _p(repl), ref.M, _p(offs), _p(peers),
                                 _p(msgs), cap, ctypes.byref(n))
    assert rc == (abi.WQ_E_CAPACITY if ref.P > cap else abi.WQ_OK), (ctx, rc)
    assert n.value == ref.P, (ctx, n.value)
    check_outputs(offs, peers, msgs, ref, cap, ctx)
    assert r.route_health() == (0, int(ref.P > cap)), ctx


def _host_caps(ref):
    b = int(np.argmax(ref.T))
    return alternate([0, 3, 5, int(ref.g0[b]) + int(ref.T[b]) // 2 + 1, ref.P - 1, ref.P], ref.P)


@pytest.mark.parametrize("hint", [0.0, 40.0])
def test_host_form_local(base, hint):
    """wq_route_tick: WQ_E_CAPACITY exactly when P > capacity, *n_pairs = P, complete offsets, the
    exact prefix, nothing at or past `capacity` (read_back) — single launch and heavy shape."""
    r = mk_router(base.w)
    r.set_fanout_hint(hint)
    for cap in _host_caps(base.ref):
        host_tick(r, base.w, base.ref, cap, f"host form, hint {hint}, capacity {cap}")
    host_tick(r, base.w, base.refs.by_key, base.ref.P // 2 + 1, "host form, raw keys", keys=True)
    r.close()


def test_host_form_global(base):
    g = _global_case()
    ref = _global_ref(base.refs.oracle, g)
    r = mk_router(base.w)
    for cap in _host_caps(ref):
        host_tick(r, g, ref, cap, f"global host form, capacity {cap}", glob=True)
    r.close()


# ---- one handle over several sub-handles --------------------------------------------------

@pytest.mark.parametrize("mode", ["cube", "replicate"])
def test_multi_handle(base, mode):
    """Router.multi over two sub-handles (shard_copy_back): the prefix and the guards as above. The
    device form is synchronous and reports like the single-GPU one (WQ_OK, counters.overflow,
    n_candidates = P as include/wq_router.h states); the host form returns WQ_E_CAPACITY when short.
    Either way wq_route_health shows the overflow exactly when the caller's capacity was short."""
    from worldql_server_amd.router import Router
    w, ref = base.w, base.ref
    r = Router.multi(CUBE, [0, 0], mode)
    r.apply_ops(w.ops)
    t = Tick(w, ref.P)
    caps = alternate([0, 1, (ref.P // 2) | 1, ref.P - 1, ref.P], ref.P)
    for cap in caps:
        # rc == WQ_OK even when short: Router.route_device raises on any other code (wq_router.hip maps
        # the multi tick's WQ_E_CAPACITY to WQ_OK for the device form; the counters carry the overflow)
        run_tick(r, t, ref, cap, f"multi {mode}, device form, capacity {cap}", F=ref.P)
    for cap in caps:
        host_tick(r, w, ref, cap, f"multi {mode}, host form, capacity {cap}")
    r.close()


# ---- a truncated tick into the diff -------------------------------------------------------

def test_truncated_tick_into_csr_diff(base):
    """wq_csr_diff_device consumes a really truncated tick: the device arrays as the route left them,
    new_capacity = the tick's capacity; expected: the host reference on the clamped oracle CSR."""
    import torch
    from test_gpu_csr_diff import Dev, _bytes_equal
    w, old = base.w, base.ref
    r = mk_router(w)
    t_old, t_new = Tick(w, old.P), Tick(w, old.P)
    run_tick(r, t_old, old, old.P, "old tick", F=old.F)
    # the hot cube loses every seventh peer and gains 40 new ones, a light cube gains one
    hot0 = int(np.cumsum(np.concatenate([[0], w.per]))[HOT])
    gone = np.arange(hot0, hot0 + N_HOT, 7, dtype=np.uint32)
    new = np.arange(w.n_peers, w.n_peers + 41, dtype=np.uint32)
    pos = np.tile([[16.0 * HOT + 8.0, 8.0, -8.0]], (len(gone) + len(new), 1))
    pos[-1, 0] = 16.0 * 3 + 8.0
    ops = abi.ops_array(np.zeros(len(pos), np.uint32), np.concatenate([gone, new]),
                        np.concatenate([np.full(len(gone), abi.OP_UNSUBSCRIBE), np.full(len(new), abi.OP_SUBSCRIBE)]),
                        pos=pos)
    o = orc.COracle(CUBE)
    o.apply_ops(w.ops)
    o.apply_ops(ops)
    r.apply_ops(ops)
    cur = _ref(*o.route(w.pos, w.world, w.sender, w.repl))
    assert cur.P <= old.P + SLACK // 2
    cap = 2 * cur.P // 3
    run_tick(r, t_new, cur, cap, "new tick, truncated", F=cur.F)
    c_no, c_np, cut = interest.clamp_csr_np(cur.offs, cur.peers[:cap], cap)
    assert cut
    want = interest.csr_diff_np(old.offs, old.peers, c_no, c_np)
    full = interest.csr_diff_np(old.offs, old.peers, cur.offs, cur.peers)
    assert len(want[1]) > 0 and len(want[3]) > len(full[3]) > 0   # the cut rows "leave" too
    M = w.M
    d_eo, d_ep, d_lo, d_lp = Dev(n=M + 1), Dev(n=cap), Dev(n=M + 1), Dev(n=old.P)
    cnt = torch.zeros(24, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    r.csr_diff_device(M, t_old.offs.data_ptr(), t_old.peers.data_ptr(), old.P, t_new.offs.data_ptr(),
                      t_new.peers.data_ptr(), cap, d_eo.ptr, d_ep.ptr, cap, d_lo.ptr, d_lp.ptr, old.P, cnt.data_ptr())
    torch.cuda.synchronize()
    c = cnt.cpu().numpy().view(abi.DIFF_COUNTERS_DTYPE)[0]
    outs = []
    for d in (d_eo, d_ep, d_lo, d_lp):
        a, ok = d.read()
        assert ok, "a guard word next to a diff output was overwritten"
        outs.append(a)
    assert (int(c["error"]), int(c["overflow"])) == (abi.DIFF_ERROR_ROWS, 0)
    assert (int(c["n_entered"]), int(c["n_left"])) == (len(want[1]), len(want[3]))
    _bytes_equal((outs[0], outs[1][:len(want[1])], outs[2], outs[3][:len(want[3])]), want)
    # the diff read its inputs only: the truncated tick's buffers are as the route left them
    offs, peers, msgs, _ = t_new.read()
    check_outputs(offs, peers, msgs, cur, cap, "after the diff")
    r.close()


# ---- forms the library reads from the environment once per process ---------------------------

# count_kernel and emit_map_kernel stride over the 7 tiles by gridDim.x (route_count.hpp, route_emit.hpp).
CHILD_ROWS = {
    # 4 workgroups take tiles {0,4} {1,5} {2,6} {3}: ragged trip counts under the loops' barriers; one
    # workgroup runs the empty block 2, then the 77-message tail block
    "two_tiles": (dict(WQ_DEBUG_COUNT_TPB="2", WQ_DEBUG_EMIT_BPB="2"), (10, 13)),
    # 3 workgroups take {0,3,6} {1,4} {2,5}: three trips against two; the empty block 2, then the hot block 5
    "three_tiles": (dict(WQ_DEBUG_COUNT_TPB="3", WQ_DEBUG_EMIT_BPB="3"), (10, 13)),
    "outcnt": (dict(WQ_TICK_OUTCNT="1"), (0, 12)),   # the tick's last block writes the caller's counters itself
}
_child_failed = []   # the first row whose child failed, faulted or ran out of time: no child is started after it


def child_sweep(row):
    """Runs in a fresh process whose environment holds the row's variables (read once by the library).
    The library has no query for the form a tick took: that these variables select it is read from
    wq_route.hip (getenv of exactly these names at the launch), not observed here — a renamed variable
    would leave the rows passing on the default form."""
    env, cfgs = CHILD_ROWS[row]
    for k, v in env.items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    w = workload()
    refs = oracle_refs(w)
    check_workload(w, refs)
    ref = refs.plain
    for cfg in cfgs:
        r = mk_router(w)
        r.set_route_config(cfg)
        sweep(r, Tick(w, ref.P), ref, short_capacities(ref), f"{row}, config {cfg}", F=ref.F)
        r.close()
    print(f"child {row} ok")


@pytest.mark.parametrize("row", sorted(CHILD_ROWS))
def test_environment_selected_forms(row):
    """One child process per row, each under its own time limit. After the first child that fails,
    faults or is killed at its limit the remaining rows fail at once without starting a child: the rows
    share their kernels, and nothing more is started on a GPU that one of them may have hung."""
    assert not _child_failed, f"not started: the child of row {_child_failed[0]!r} failed before"
    env = dict(os.environ)
    for k in ("WQ_DEBUG_COUNT_TPB", "WQ_DEBUG_EMIT_BPB", "WQ_TICK_OUTCNT", "WQ_ROUTE_CHUNKS"):
        env.pop(k, None)
    env.update(CHILD_ROWS[row][0])
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_gpu_truncation as t; t.child_sweep({row!r})")
    _child_failed.append(row)   # until the child has ended well (a TimeoutExpired leaves it set too)
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (row, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert f"child {row} ok" in p.stdout
    _child_failed.remove(row)
