"""What a tick leaves when its pairs exceed what u32 CSR offsets address (P > 2^32 - 1), in every tick
shape: the contract of include/wq_router.h (wq_route_tick_device), on guarded buffers.

For an over-limit tick: counters.n_pairs is the exact P (u64), n_candidates the exact F, error = 2,
overflow = 1; wq_route_health shows bit 2 once, then (0, 0); offsets[0 .. M] are written and nothing
behind them; nothing at index >= capacity is written in peers / msgs (with capacity 0 nothing at all);
the host forms return WQ_E_CAPACITY with *n_pairs = P and leave their arrays alone; the next tick on
the handle is exact. P = 2^32 - 1 is an ordinary tick. On every handle legal and over-limit ticks
alternate, ending with a legal one, and every legal tick is held to the whole truncation contract of
tests/test_gpu_truncation.py (whose harness this file uses) against a closed-form reference.

The workload (one world, cube size 16): cube A holds peers 0 .. 65,536, B peers 0 .. 65,535, C one
peer, D peers 0 .. 8,199; world 1's any-set holds 65,537 peers (the global ticks). All messages of a
tick go into one cube (first_over adds one message at C), so the reference is closed-form from the
CPU oracle's list of that cube (one COracle.route of a single message per cube): offsets are the
running sum of e in u64, the first `capacity` pairs are that list repeated, minus the sender for
ExceptSelf. The oracle is never asked for 4e9 pairs; tests/test_pair_limit_workload.py checks the
products and the closed form against it without a GPU. No buffer is ever sized for P: the device
buffers are capacity + 4096 canary words, capacities are {0, 4099}, and two_wraps also runs at 2^24,
which lies above its P mod 2^32 = 9,020,008 — the case in which a wrapped P looks like a complete tick.

two_wraps has 4,097 tiles of 256 messages: more than twice the 2,048 workgroups of the default
single-launch tick that one MI355X holds at once (20.3 KB of LDS per workgroup: 8 per CU, 256 CUs —
from the kernel's resource usage, not measured), so later blocks look back on prefixes that earlier,
finished generations published, and the multi-block tile scan (from 2,048 tiles) runs.

Every store of every emit shape sits behind `index < capacity` with the index computed in 64 bits from
a u32 prefix, or from the exact 40-bit prefix in the single-launch tick (route_emit.hpp emit_direct,
emit_row_img, emit_map_kernel; route_tick.hpp copy_image_out; wq_global.hip global_copy_kernel, which
writes nothing in an over-limit tick); the loads are row-local and do not depend on the prefix.

The radius filter runs at capacity 0 only: its windowed emit re-filters every long list once per
4,096-output window, hours at this fan-out. Forms that the library reads from the environment once per
process (WQ_TICK_OUTCNT, WQ_SCAN_MULTI=0) run in child processes, one per row, under the rule of
tests/test_gpu_truncation.py: after the first child that fails or times out, none is started.

Out of scope here: a multi-handle tick whose slices are each legal but sum past the limit (it needs
tens of GB of staging); the hub / RCCL entry points called directly; P beyond 2^40.
"""
import ctypes
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle as orc
from worldql_server_amd import abi
from test_gpu_truncation import (CANARY, OFF_GUARD, SLACK, Tick, _p, _same, _untouched, check_outputs, mk_router,
                                 run_tick)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CUBE = 16
LIMIT = 0xFFFFFFFF                      # pairs that u32 offsets address
CUBE_A, CUBE_B, CUBE_C, CUBE_D = 0, 1, 2, 3   # cube indices along the x axis
N_A, N_B, N_D = 65537, 65536, 8200
C_PEER = 7
W_WORLD = 1                             # the global ticks' world: any-set = peers 0 .. 65,536
CAPS = (0, 4099)
CAP_WRAP = 1 << 24                      # above two_wraps' P mod 2^32
PREFIX = 8192                           # pairs of the closed form that a reference holds (prefix_of)
RADIUS = 64.0                           # every peer position (all at A's centre) is in range of A and C
INCL, EXCEPT = abi.REPL_INCLUDING_SELF, abi.REPL_EXCEPT_SELF

# name -> [(cube, messages, replication)]; expected P in EXPECTED_P
TICKS = {
    "last_legal": [(CUBE_A, 65535, INCL)],
    "first_over": [(CUBE_A, 65535, INCL), (CUBE_C, 1, INCL)],
    "square": [(CUBE_B, 65536, INCL)],
    "except_legal": [(CUBE_A, 65535, EXCEPT)],
    "except_over": [(CUBE_A, 65537, EXCEPT)],
    "two_wraps": [(CUBE_D, 4096 * 256 + 77, INCL)],
    "small_legal": [(CUBE_D, 300, INCL)],   # the legal tick between two_wraps ticks
}
EXPECTED_P = {
    "last_legal": (1 << 32) - 1, "first_over": 1 << 32, "square": 1 << 32, "except_legal": (1 << 32) - 65536,
    "except_over": (1 << 32) + 65536, "two_wraps": 8598954600, "small_legal": 300 * 8200,
    "global_legal": (1 << 32) - 1, "global_over": (1 << 32) + 65536,
}
GLOBAL_TICKS = {"global_legal": 65535, "global_over": 65536}

# the tag-wrap test's light cubes: 64 cubes of 1 .. 3 peers from cube index 10 on
LIGHT0, N_LIGHT, LIGHT_PEER0 = 10, 64, 70000


# ---- workload (CPU only) ------------------------------------------------------------------

def _centres(cube):
    cube = np.asarray(cube, dtype=np.float64)
    return np.stack([16.0 * cube + 8.0, np.full(len(cube), 8.0), np.full(len(cube), -8.0)], 1)


def subscriptions():
    """The op batch: cubes A, B, C, D in world 0, cube A's peers again in world 1, the light cubes."""
    light_per = 1 + np.arange(N_LIGHT) % 3
    world = np.concatenate([np.zeros(N_A + N_B + 1 + N_D, np.uint32), np.full(N_A, W_WORLD, np.uint32),
                            np.zeros(int(light_per.sum()), np.uint32)])
    peer = np.concatenate([np.arange(N_A), np.arange(N_B), [C_PEER], np.arange(N_D), np.arange(N_A),
                           LIGHT_PEER0 + np.arange(int(light_per.sum()))]).astype(np.uint32)
    cube = np.concatenate([np.full(N_A, CUBE_A), np.full(N_B, CUBE_B), [CUBE_C], np.full(N_D, CUBE_D),
                           np.full(N_A, CUBE_A), np.repeat(LIGHT0 + np.arange(N_LIGHT), light_per)])
    return abi.ops_array(world, peer, np.zeros(len(peer), np.uint8), pos=_centres(cube))


def messages(cube, repl):
    """One tick: message m at a point inside cube[m]; senders are members of A (sender = m modulo A's
    65,537 peers, so ExceptSelf drops exactly one recipient per message at A)."""
    cube = np.asarray(cube, dtype=np.int64)
    M = len(cube)
    m = np.arange(M)
    pos = np.stack([16.0 * cube + 0.5 + (m % 15), 0.5 + (m % 13), -0.5 - (m % 11)], 1).astype(np.float64)
    return SimpleNamespace(pos=pos, keys=orc.quantize_np(pos, CUBE), world=np.zeros(M, np.uint32),
                           sender=(m % N_A).astype(np.uint32), repl=np.asarray(repl, dtype=np.uint8), cube=cube, M=M)


def make_tick(name):
    parts = TICKS[name]
    return messages(np.concatenate([np.full(n, c) for c, n, _ in parts]),
                    np.concatenate([np.full(n, rp, np.uint8) for _, n, rp in parts]))


def make_global_tick(name):
    M = GLOBAL_TICKS[name]
    return SimpleNamespace(world=np.full(M, W_WORLD, np.uint32), sender=(np.arange(M) % N_A).astype(np.uint32),
                           repl=np.full(M, INCL, np.uint8), pos=np.zeros((M, 3)), keys=np.zeros((M, 3), np.int64), M=M)


def oracle_lists(o):
    """The oracle's recipients of one IncludingSelf message into each cube, and of one to world 1."""
    lists = {}
    for c in (CUBE_A, CUBE_B, CUBE_C, CUBE_D):
        w = messages([c], [INCL])
        offs, peers, F = o.route(w.pos, w.world, w.sender, w.repl)
        assert F == len(peers) == offs[1]
        lists[c] = peers
    g = make_global_tick("global_legal")
    offs, peers = o.route_global(g.world[:1], g.sender[:1], g.repl[:1])
    lists["W"] = peers
    return lists


def closed_form(key, lists, sender, repl, prefix):
    """The reference of a tick whose message m reads the list lists[key[m]] (the oracle's, ascending): e,
    the offsets as a u64 running sum, P, F, and the first `prefix` pairs."""
    key, sender = np.asarray(key), np.asarray(sender)
    M = len(key)
    L = np.zeros(M, np.uint64)
    member = np.zeros(M, bool)
    for k in np.unique(key):
        x, sel = lists[k.item()], key == k
        L[sel] = len(x)
        at = np.minimum(np.searchsorted(x, sender[sel]), len(x) - 1)
        member[sel] = x[at] == sender[sel]
    is_except = np.asarray(repl) != INCL
    e = L - (is_except & member).astype(np.uint64)   # ExceptSelf drops the sender where it is a recipient
    offs64 = np.concatenate([[0], np.cumsum(e, dtype=np.uint64)]).astype(np.uint64)
    P = int(offs64[-1])
    n = min(P, prefix)
    k = int(np.searchsorted(offs64, n, side="left"))   # the first k messages hold the first n pairs
    rows = [lists[c.item()] for c in key[:k]]
    rows = [x[x != s] if ex else x for x, s, ex in zip(rows, sender[:k], is_except[:k])]
    peers = np.concatenate(rows)[:n].astype(np.uint32) if k else np.zeros(0, np.uint32)
    msgs = np.repeat(np.arange(k, dtype=np.uint32), e[:k].astype(np.int64))[:n]
    return SimpleNamespace(offs64=offs64, offs=(offs64 & np.uint64(LIMIT)).astype(np.uint32), e=e, P=P, F=int(L.sum()),
                           M=M, peers=peers, msgs=msgs)


def prefix_of(name):
    """Pairs that the tick's reference holds: every capacity it runs at lies below (small_legal: its whole P)."""
    return CAP_WRAP if name in ("two_wraps", "small_legal") else PREFIX


def reference(name, w, lists):
    key = np.full(w.M, "W") if name in GLOBAL_TICKS else w.cube
    return closed_form(key, lists, w.sender, w.repl, prefix_of(name))


def light_tick(kind):
    """The tag-wrap test's ticks over the light cubes. "even": 4,096 blocks, message m into cube m mod 64
    (every block the same total); "blocks": 4,096 blocks, block b wholly into cube b mod 64 (block totals
    of 256, 512 and 768 pairs: another prefix at every block); "one": a single block."""
    M = 4096 * 256 if kind != "one" else 100
    m = np.arange(M)
    cube = LIGHT0 + ((m // 256) % N_LIGHT if kind == "blocks" else m % N_LIGHT)
    w = messages(cube, np.full(M, INCL, np.uint8))
    w.sender[:] = LIGHT_PEER0   # a member of the first light cube only
    w.repl[1::2] = EXCEPT
    return w


@functools.lru_cache(maxsize=1)
def build_base():
    """The subscriptions, the oracle, every tick and its closed-form reference: computed once per process
    and left unchanged."""
    ops = subscriptions()
    o = orc.COracle(CUBE)
    o.apply_ops(ops)
    lists = oracle_lists(o)
    ticks = {name: make_tick(name) for name in TICKS}
    ticks.update({name: make_global_tick(name) for name in GLOBAL_TICKS})
    refs = {name: reference(name, w, lists) for name, w in ticks.items()}
    return SimpleNamespace(w=SimpleNamespace(ops=ops), ops=ops, oracle=o, lists=lists, ticks=ticks, refs=refs)


def check_base(b):
    """The products, from the oracle's list lengths alone."""
    n = {c: len(x) for c, x in b.lists.items()}
    assert (n[CUBE_A], n[CUBE_B], n[CUBE_C], n[CUBE_D], n["W"]) == (N_A, N_B, 1, N_D, N_A)
    for name, ref in b.refs.items():
        assert ref.P == EXPECTED_P[name], (name, ref.P)
    P = {name: ref.P for name, ref in b.refs.items()}
    assert P["last_legal"] == n[CUBE_A] * 65535 == LIMIT and P["global_legal"] == n["W"] * 65535 == LIMIT
    assert P["first_over"] == P["last_legal"] + n[CUBE_C] == LIMIT + 1
    assert P["square"] == n[CUBE_B] * 65536 == LIMIT + 1
    assert P["except_legal"] == (n[CUBE_A] - 1) * 65535 <= LIMIT < P["except_over"] == (n[CUBE_A] - 1) * 65537
    assert P["two_wraps"] == n[CUBE_D] * (4096 * 256 + 77) and P["two_wraps"] >> 32 == 2
    assert P["two_wraps"] % (1 << 32) == 9020008 < CAP_WRAP   # a wrapped P would look complete at this capacity
    assert P["two_wraps"] // 2 > LIMIT                          # each half of a two-device handle is over alone
    assert (b.ticks["two_wraps"].M + 255) // 256 > 2 * 2048     # more than twice the resident workgroups
    assert P["global_over"] > LIMIT and P["small_legal"] < LIMIT
    for name, ref in b.refs.items():
        assert len(ref.peers) == len(ref.msgs) == min(ref.P, prefix_of(name))
        assert ref.F >= ref.P and len(ref.peers) >= max(CAPS)
        assert ref.peers.max() < 1 << 17 and (ref.offs64[-1] >> 40) == 0
    # first_over's last message is the one at C; the legal ticks' last offset is exact in u32
    assert b.refs["first_over"].e[-1] == 1 and b.refs["last_legal"].offs[-1] == LIMIT


@pytest.fixture(scope="module")
def base():
    b = build_base()
    check_base(b)
    return b


# ---- harness (GPU) ------------------------------------------------------------------------

def router(b, cfg=None):
    r = mk_router(b.w)
    if cfg is not None:
        r.set_route_config(cfg)
    return r


def device_tick(r, t, cap, glob=False):
    t.fill()
    if glob:
        r.route_global_device(t.world.data_ptr(), t.sender.data_ptr(), t.repl.data_ptr(), t.M, t.offs.data_ptr(),
                              t.peers.data_ptr(), t.msgs.data_ptr(), cap, t.cnt.data_ptr())
    else:
        pos, world, sender, repl, M = t.inputs()
        r.route_device(pos, world, sender, repl, M, t.offs.data_ptr(), t.peers.data_ptr(), t.msgs.data_ptr(), cap,
                       t.cnt.data_ptr(), keys_ptr=t.keys.data_ptr() if t.keys is not None else None)
    return t.read()


def check_over_outputs(offs, peers, msgs, ref, cap, ctx):
    """Guards of an over-limit tick on host copies: offsets[0 .. M] written (their values are not
    specified; the true offsets modulo 2^32 hold the canary word as often as counted here), nothing
    behind them, nothing in peers / msgs from `cap` on."""
    M = ref.M
    assert int((offs[:M + 1] == CANARY).sum()) <= int((ref.offs == CANARY).sum()), (ctx, "offsets left unwritten")
    _untouched(offs, M + 1, "offsets", ctx)
    _untouched(peers, cap, "peers", ctx)
    _untouched(msgs, cap, "msgs", ctx)


def run_over(r, t, ref, cap, ctx, glob=False):
    """One over-limit device tick into guarded buffers of cap + SLACK words."""
    assert ref.P > LIMIT and cap + SLACK == len(t.peers)
    offs, peers, msgs, c = device_tick(r, t, cap, glob)
    check_over_outputs(offs, peers, msgs, ref, cap, ctx)
    got = (int(c["n_pairs"]), int(c["overflow"]), int(c["error"]))
    assert got == (ref.P, 1, 2), (ctx, got, ref.P)
    assert int(c["n_candidates"]) == ref.F, (ctx, int(c["n_candidates"]), ref.F)
    assert r.route_health() == (2, 1), ctx
    assert r.route_health() == (0, 0), ctx


def run_legal(r, t, ref, cap, ctx, glob=False):
    assert ref.P <= LIMIT and cap + SLACK == len(t.peers)
    run_tick(r, t, ref, cap, ctx, F=ref.F, glob=glob)


class Ticks:
    """Device inputs and guarded buffers per (tick, capacity), made once per test."""

    def __init__(self, b, keys=False):
        self.b, self.keys, self.t = b, keys, {}

    def get(self, name, cap):
        if (name, cap) not in self.t:
            self.t[name, cap] = Tick(self.b.ticks[name], cap, keys=self.keys)
        return self.t[name, cap]


def alternate(r, b, legal, overs, caps, tag, keys=False, glob=False):
    """legal, over, legal, over, ..., legal on one handle, over every (over-limit tick, capacity)."""
    ts = Ticks(b, keys)
    for over in overs:
        for cap in caps:
            run_legal(r, ts.get(legal, cap), b.refs[legal], cap, f"{tag}: {legal}, capacity {cap}", glob)
            run_over(r, ts.get(over, cap), b.refs[over], cap, f"{tag}: {over}, capacity {cap}", glob)
    run_legal(r, ts.get(legal, caps[-1]), b.refs[legal], caps[-1], f"{tag}: {legal} at the end", glob)


def _n_configs():
    from worldql_server_amd.router import load_library
    return int(load_library().wq_debug_route_config_count())


# ---- every config -------------------------------------------------------------------------

def test_first_over_default_config_offsets_only(base):
    """Config 0, first_over at capacity 0 (no emit runs), between two last_legal ticks: the smallest row."""
    r = router(base, 0)
    alternate(r, base, "last_legal", ["first_over"], [0], "config 0")
    r.close()


@pytest.mark.parametrize("cfg", range(14))
def test_every_config(base, cfg):
    """Config `cfg` x {last_legal, first_over, except_over} x capacities {0, 4099}."""
    assert _n_configs() == 14, "a route config was added or removed: extend the parametrisation to match"
    r = router(base, cfg)
    alternate(r, base, "last_legal", ["first_over", "except_over"], CAPS, f"config {cfg}")
    r.close()


@pytest.mark.parametrize("cfg", [0, 1, 10])
def test_square_and_except_legal(base, cfg):
    """65,536 messages x 65,536 peers = 2^32 exactly, against the largest legal ExceptSelf tick."""
    r = router(base, cfg)
    alternate(r, base, "except_legal", ["square"], CAPS, f"config {cfg}")
    r.close()


@pytest.mark.parametrize("cfg", [0, 1, 7, 10, 12])
def test_two_wraps(base, cfg):
    """P = 8,598,954,600 over 4,097 blocks: the one-launch tick across more than two generations of
    resident workgroups (0, 12), the multi-block tile scan (1, 7, 10); at capacity 2^24 a P taken modulo
    2^32 (9,020,008) would pass for a complete tick."""
    r = router(base, cfg)
    alternate(r, base, "small_legal", ["two_wraps"], CAPS + (CAP_WRAP,), f"config {cfg}")
    r.close()


@pytest.mark.parametrize("chunks", [2, 3])
def test_two_wraps_pipelined_chunks(base, chunks):
    """Config 10 in 2 and 3 pipelined chunks: {P, F} carried from chunk to chunk in 64 bits."""
    r = router(base, 10)
    n_count = (base.ticks["two_wraps"].M + 255) // 256
    assert n_count >= 2 * chunks and (n_count + chunks - 1) // chunks <= 8192   # wq_route.hip: the chunked path is taken
    r.set_route_chunks(chunks)
    alternate(r, base, "small_legal", ["two_wraps"], CAPS, f"config 10, chunks {chunks}")
    r.close()


@pytest.mark.parametrize("cfg", [0, 10])
def test_raw_keys(base, cfg):
    """Raw cube keys instead of positions (the RAW_KEYS instantiations)."""
    r = router(base, cfg)
    alternate(r, base, "last_legal", ["first_over"], CAPS, f"config {cfg}, raw keys", keys=True)
    r.close()


def test_radius_filter(base):
    """count_radius with every peer in range (all peer positions at A's centre, radius 64), at capacity 0:
    the windowed radius emit at this fan-out is no test of a few seconds (module docstring)."""
    r = router(base)
    r.set_peer_positions(np.tile(_centres([CUBE_A]), (LIGHT_PEER0 + 3 * N_LIGHT, 1)))
    r.set_radius(RADIUS)
    ts = Ticks(base)
    ll, fo = base.refs["last_legal"], base.refs["first_over"]
    run_legal(r, ts.get("last_legal", 0), ll, 0, "radius: last_legal")
    run_over(r, ts.get("first_over", 0), fo, 0, "radius: first_over")
    run_legal(r, ts.get("last_legal", 0), ll, 0, "radius: last_legal again")
    r.set_radius(0.0)
    run_legal(r, ts.get("last_legal", 4099), ll, 4099, "radius off again")
    r.close()


# ---- global -------------------------------------------------------------------------------

def test_global_device(base):
    """wq_route_global_device: 65,535 and 65,536 messages to a world of 65,537 peers. n_candidates is the
    any-set's size per message (global_count_kernel), as for a local tick the list's."""
    r = router(base)
    alternate(r, base, "global_legal", ["global_over"], CAPS, "global", glob=True)
    r.close()


# ---- host forms ---------------------------------------------------------------------------

def host_tick(r, w, ref, cap, ctx, glob=False):
    """lib.wq_route_tick / wq_route_global on canary-filled numpy arrays of cap + SLACK words."""
    offs = np.full(ref.M + 1 + OFF_GUARD, CANARY, np.uint32)
    peers = np.full(cap + SLACK, CANARY, np.uint32)
    msgs = np.full(cap + SLACK, CANARY, np.uint32)
    n = ctypes.c_size_t(12345)
    world, sender, repl = (np.ascontiguousarray(x) for x in (w.world, w.sender, w.repl))
    if glob:
        rc = r.lib.wq_route_global(r.h, _p(world), _p(sender), _p(repl), ref.M, _p(offs), _p(peers), _p(msgs), cap,
                                   ctypes.byref(n))
    else:
        pos = np.ascontiguousarray(w.pos, dtype=np.float64)
        rc = r.lib.wq_route_tick(r.h, _p(pos), None, _p(world), _p(sender), _p(repl), ref.M, _p(offs), _p(peers),
                                 _p(msgs), cap, ctypes.byref(n))
    assert rc == (abi.WQ_E_CAPACITY if ref.P > cap else abi.WQ_OK), (ctx, rc)
    return offs, peers, msgs, n.value


def host_over(r, w, ref, cap, ctx, glob=False, exact=True):
    offs, peers, msgs, n = host_tick(r, w, ref, cap, ctx, glob)
    assert n == ref.P if exact else n > LIMIT, (ctx, n)
    for a, what in ((offs, "offsets"), (peers, "peers"), (msgs, "msgs")):
        _untouched(a, 0, what + " (host array)", ctx)


def host_legal(r, w, ref, cap, ctx, glob=False):
    offs, peers, msgs, n = host_tick(r, w, ref, cap, ctx, glob)
    assert n == ref.P, (ctx, n)
    check_outputs(offs, peers, msgs, ref, cap, ctx)
    assert r.route_health() == (0, int(ref.P > cap)), ctx


def test_host_form_local(base):
    """wq_route_tick: WQ_E_CAPACITY, *n_pairs = P and untouched arrays past the limit; the copied prefix
    of last_legal. (From its second tick on the handle has taken the heavy shape by itself.)"""
    r = router(base)
    tk, rf = base.ticks, base.refs
    for over in ("first_over", "except_over"):
        for cap in CAPS:
            host_legal(r, tk["last_legal"], rf["last_legal"], 4099, f"host form: last_legal before {over}")
            host_over(r, tk[over], rf[over], cap, f"host form: {over}, capacity {cap}")
            assert r.route_health() == (2, 1) and r.route_health() == (0, 0)
    host_legal(r, tk["last_legal"], rf["last_legal"], 0, "host form: last_legal, capacity 0")
    r.close()


def test_host_form_global(base):
    r = router(base)
    tk, rf = base.ticks, base.refs
    for cap in CAPS:
        host_legal(r, tk["global_legal"], rf["global_legal"], 4099, "global host form: global_legal", glob=True)
        host_over(r, tk["global_over"], rf["global_over"], cap, f"global host form: capacity {cap}", glob=True)
        assert r.route_health() == (2, 1) and r.route_health() == (0, 0)
    host_legal(r, tk["global_legal"], rf["global_legal"], 0, "global host form: capacity 0", glob=True)
    r.close()


def test_router_route_raises_at_once(base):
    """Router.route(capacity=None) answers WQ_E_CAPACITY by asking again with room for P: past the limit it
    raises after the first tick instead (one route call, no 17 GB buffer)."""
    from worldql_server_amd.router import WQError
    r = router(base)
    w = base.ticks["first_over"]
    before = r.route_calls()
    with pytest.raises(WQError) as ei:
        r.route(w.pos, w.world, w.sender, w.repl)
    assert ei.value.code == abi.WQ_E_CAPACITY and r.route_calls() == before + 1
    assert r.route_health() == (2, 1)
    w = base.ticks["small_legal"]   # the same call still grows its buffer for a legal tick
    offs, peers, _ = r.route(w.pos, w.world, w.sender, w.repl, capacity=None)
    ref = base.refs["small_legal"]
    assert len(peers) == ref.P > max(1024, 16 * w.M)   # the first call's capacity was short
    _same(offs, ref.offs, "offsets", "Router.route, small_legal")
    _same(peers, ref.peers, "peers", "Router.route, small_legal")
    r.close()


# ---- one handle over two sub-handles -------------------------------------------------------

@pytest.mark.parametrize("mode", ["cube", "replicate"])
def test_multi_handle(base, mode):
    """Router.multi over devices (0, 0), two_wraps: each half alone is over the limit. Both forms return
    WQ_E_CAPACITY (counters.n_pairs / *n_pairs >= 2^32); nothing is written at or past `capacity`; a
    small legal tick afterwards is exact (the multi handle reports F as P)."""
    from worldql_server_amd.router import Router, WQError
    r = Router.multi(CUBE, [0, 0], mode)
    r.apply_ops(base.ops)
    ts = Ticks(base)
    w, ref = base.ticks["two_wraps"], base.refs["two_wraps"]
    small, sref = base.ticks["small_legal"], base.refs["small_legal"]
    multi_ref = SimpleNamespace(**{**vars(sref), "F": sref.P})
    for cap in CAPS:
        ctx = f"multi {mode}, capacity {cap}"
        run_legal(r, ts.get("small_legal", cap), multi_ref, cap, ctx + ": small_legal")
        t = ts.get("two_wraps", cap)
        t.fill()
        pos, world, sender, repl, M = t.inputs()
        with pytest.raises(WQError) as ei:
            r.route_device(pos, world, sender, repl, M, t.offs.data_ptr(), t.peers.data_ptr(), t.msgs.data_ptr(), cap,
                           t.cnt.data_ptr())
        assert ei.value.code == abi.WQ_E_CAPACITY, ctx
        offs, peers, msgs, c = t.read()
        assert int(c["n_pairs"]) > LIMIT and (int(c["overflow"]), int(c["error"])) == (1, 2), (ctx, c)
        _untouched(offs, M + 1, "offsets", ctx)
        _untouched(peers, cap, "peers", ctx)
        _untouched(msgs, cap, "msgs", ctx)
        err, _ = r.route_health()
        assert err & 2 and r.route_health() == (0, 0), ctx
        host_over(r, w, ref, cap, ctx + ", host form", exact=False)
        err, _ = r.route_health()
        assert err & 2 and r.route_health() == (0, 0), ctx
    run_legal(r, ts.get("small_legal", 4099), multi_ref, 4099, f"multi {mode}: small_legal at the end")
    host_legal(r, small, sref, 4099, f"multi {mode}: small_legal, host form")
    r.close()


# ---- the granule tags' wrap ----------------------------------------------------------------

def test_tick_granule_tags_wrap(base):
    """The single-launch tick tags its look-back granules with the call counter modulo 2^22 - 1 and must
    zero them when the tags wrap: a 4,096-block tick, one period minus one later a one-block tick, then a
    4,096-block tick with other block totals that carries the first tick's tag. Without the zeroing its
    blocks 1 .. 4,095 read the first tick's prefixes as their own. Exact against the oracle."""
    r = router(base, 0)
    o = base.oracle

    def tick(kind):
        w = light_tick(kind)
        offs, peers, F = o.route(w.pos, w.world, w.sender, w.repl)
        M = w.M
        e = np.diff(offs.astype(np.int64))
        ref = SimpleNamespace(offs=offs, peers=peers, msgs=np.repeat(np.arange(M, dtype=np.uint32), e), F=F,
                              P=int(offs[M]), M=M)
        run_tick(r, Tick(w, ref.P), ref, ref.P, f"tag wrap: {kind}", F=F)
        return ref

    c0 = r.route_calls()
    a = tick("even")
    assert r.route_calls() == c0 + 1
    r.set_route_calls(c0 + abi.TICK_TAG_PERIOD - 1)
    tick("one")
    assert r.route_calls() == c0 + abi.TICK_TAG_PERIOD   # the next tick's tag is the first tick's
    b = tick("blocks")
    T = lambda ref: np.diff(ref.offs[0::256].astype(np.int64))
    assert len(set(T(a).tolist())) == 1 and len(set(T(b).tolist())) >= 3   # other prefixes at every block
    r.close()


# ---- forms the library reads from the environment once per process -------------------------

CHILD_ROWS = {
    "outcnt": (dict(WQ_TICK_OUTCNT="1"), 0),      # the tick's last block writes the caller's counters itself
    "scan_rocprim": (dict(WQ_SCAN_MULTI="0"), 1),  # rocPRIM's scan + tile_finish_kernel from 2,048 tiles on
}
_child_failed = []   # the first row whose child failed, faulted or ran out of time: no child is started after it


def child_row(row):
    """Runs in a fresh process whose environment holds the row's variables (read once by the library:
    wq_route.hip, route_scan.hpp)."""
    env, cfg = CHILD_ROWS[row]
    for k, v in env.items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    b = build_base()
    r = router(b, cfg)
    alternate(r, b, "small_legal", ["two_wraps"], CAPS + (CAP_WRAP,), f"{row}, config {cfg}")
    r.close()
    print(f"child {row} ok")


@pytest.mark.parametrize("row", sorted(CHILD_ROWS))
def test_environment_selected_forms(row):
    """One child process per row, each under its own time limit; after the first child that fails, faults
    or is killed at its limit the remaining rows fail at once without starting a child."""
    assert not _child_failed, f"not started: the child of row {_child_failed[0]!r} failed before"
    env = dict(os.environ)
    for k in ("WQ_TICK_OUTCNT", "WQ_SCAN_MULTI", "WQ_SCAN_MULTI_MIN", "WQ_ROUTE_CHUNKS", "WQ_DEBUG_COUNT_TPB",
              "WQ_DEBUG_EMIT_BPB"):
        env.pop(k, None)
    env.update(CHILD_ROWS[row][0])
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_gpu_pair_limit as t; t.child_row({row!r})")
    _child_failed.append(row)   # until the child has ended well (a TimeoutExpired leaves it set too)
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (row, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert f"child {row} ok" in p.stdout
    _child_failed.remove(row)
