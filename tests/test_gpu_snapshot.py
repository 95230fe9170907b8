"""Table snapshots on the GPU (wq_table_export*, wq_follow_state_*; csrc/wq_table_export.hip): every
export is compared byte for byte with snapshot.TableRef.export, the host definition."""
import ctypes
import threading

import numpy as np
import pytest

from oracle import oracle as orc
from worldql_server_amd import abi, snapshot, synth
from worldql_server_amd.snapshot import TableRef

pytestmark = pytest.mark.gpu

S, U, R = abi.OP_SUBSCRIBE, abi.OP_UNSUBSCRIBE, abi.OP_REMOVE_PEER
BIG_WORLD = (1 << 24) + 5
CANARY = 0xA5


def mk_router(cube_size=16, **kw):
    from worldql_server_amd.router import Router
    return Router(cube_size, 0, **kw)


def subs(world, peers, key=None, pos=None, kind=S):
    peers = np.asarray(peers, dtype=np.uint32)
    n = len(peers)
    if key is not None:
        return abi.ops_array(np.full(n, world, np.uint32), peers, np.full(n, kind, np.uint8),
                             key=np.tile(np.asarray(key, np.int64), (n, 1)))
    return abi.ops_array(np.full(n, world, np.uint32), peers, np.full(n, kind, np.uint8),
                         pos=np.tile(np.asarray(pos, np.float64), (n, 1)))


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def dev_export(r, capacity, world=None, peers=None):
    """export_table_device into a canaried buffer: (rc, n, the rows written as bytes)."""
    import torch
    buf = torch.full((capacity * 40 + 64,), CANARY, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc, n = r.export_table_device(buf.data_ptr(), capacity, world=world, peers=peers)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    kept = min(n, capacity)
    assert (host[kept * 40:] == CANARY).all(), "rows past the capacity (or the count) were written"
    return rc, n, host[: kept * 40].tobytes()


def edge_ops(cs):
    """One table with every list-length edge, extreme keys and the keys without a packed form."""
    parts, nxt = [], 0
    for i, n in enumerate([1, 24, 25, 63, 64, 65, 257, 1025, 5000]):
        parts.append(subs(i % 2, np.arange(nxt, nxt + n), key=(cs * (i - 4), -cs * i, cs * 3)))
        nxt += n // 2  # lists overlap: peers sit in several cubes
    far = (1 << 23) - 1
    parts.append(subs(0, [7, 3], key=(far * cs, -far * cs, far * cs)))
    parts.append(subs(0, [5], key=(-far * cs, far * cs, -far * cs)))
    parts.append(subs(0, [9, 2, 4], key=(7, 1, 1)))                       # off grid: raw key only
    parts.append(subs(BIG_WORLD, [1, 0], key=(0, cs, 0)))                 # world without a packed form
    parts.append(subs(1, [11], pos=(np.nan, 1.0, -1.0)))                  # NaN position
    parts.append(subs(0, [20, 21, 22], key=(cs * 9, 0, 0)))               # emptied below
    parts.append(subs(0, [20, 21, 22], key=(cs * 9, 0, 0), kind=U))
    parts.append(subs(0, [30], pos=(0.5 * cs, -0.5 * cs, 2.5 * cs)))
    return abi.concat_ops(parts)


@pytest.fixture(scope="module")
def edges():
    """(ops, TableRef export, a router holding them) at cube size 16, shared read-only."""
    ops = edge_ops(16)
    t = TableRef(16)
    t.apply(ops)
    r = mk_router(16)
    r.apply_ops(ops)
    yield ops, t, r
    r.close()


@pytest.mark.parametrize("cs", [16, 10])
def test_list_length_edges(cs, edges):
    if cs == 16:
        ops, t, r = edges
    else:
        ops = edge_ops(cs)
        t = TableRef(cs)
        t.apply(ops)
        r = mk_router(cs)
        r.apply_ops(ops)
    want = t.export()
    assert len(want) > 6000
    got = r.export_table()
    assert got.dtype == abi.OP_DTYPE and got.tobytes() == want.tobytes()
    rc, n, raw = dev_export(r, len(want))
    assert (rc, n) == (0, len(want)) and raw == want.tobytes()
    st = r.stats()
    assert st["n_entries"] == len(want) and st["n_cubes"] == t.counts()["n_cubes"]


def history_case():
    rng = np.random.default_rng(5)
    nc = 600
    ck = rng.choice(40 * 40, nc, replace=False)
    keys = np.stack([(ck // 40 - 20) * 16, (ck % 40 - 20) * 16, rng.integers(-2, 3, nc) * 16], 1)
    cw = rng.integers(0, 2, nc)
    base = abi.concat_ops([subs(int(cw[i]), rng.choice(500, int(rng.integers(1, 13)), replace=False), key=keys[i])
                           for i in range(nc)])
    X, Y, E1, E2 = (1600, 0, 0), (1616, 0, 0), (1632, 0, 0), (1648, 0, 0)
    first = abi.concat_ops([base, subs(0, np.arange(100, 120), key=X), subs(0, np.arange(200, 260), key=Y),
                            subs(1, [1, 2, 3], key=E1), subs(1, [4, 5, 6], key=E2)])
    churn = base[rng.choice(len(base), 60, replace=False)].copy()
    churn["kind"] = U
    back = churn.copy()
    back["kind"] = S
    steps = [subs(0, np.arange(120, 130), key=X),                  # 20 -> 30: leaves the inline words
             subs(0, np.arange(260, 290), key=Y),                  # 60 -> 90: past its capacity, relocated
             subs(1, [1, 2, 3], key=E1, kind=U), subs(1, [4, 5, 6], key=E2, kind=U), churn, back]
    return first, steps


@pytest.fixture(scope="module")
def history():
    first, steps = history_case()
    t = TableRef(16)
    t.apply(first)
    for s in steps:
        t.apply(s)
    return first, steps, t.export()


def test_history_one_batch_and_incremental(history):
    first, steps, want = history
    r = mk_router()
    r.apply_ops(want)
    assert r.export_table().tobytes() == want.tobytes()
    r.close()
    r = mk_router()
    r.apply_ops(first)
    for s in steps:
        assert len(s) * 4 <= len(first)
        r.apply_ops(s)
    inc, fb = r.update_counts()
    assert inc >= 4, (inc, fb)
    assert r.export_table().tobytes() == want.tobytes()
    r.close()


def test_history_remove_peers_in_place(history):
    first, steps, want = history
    rng = np.random.default_rng(6)
    extra = np.arange(9000, 9010)
    cubes = want[rng.choice(len(want), 40, replace=False)]
    more = abi.concat_ops([subs(int(c["world"]), extra, key=c["key"]) for c in cubes])
    r = mk_router()
    r.apply_ops(abi.concat_ops([want, more]))
    assert r.stats()["n_entries"] > len(want)
    r.remove_peers(extra)
    assert r.export_table().tobytes() == want.tobytes()
    r.close()


@pytest.mark.parametrize("how", ["hash_bits", "record_slack"])
def test_history_table_shape(history, how):
    _, _, want = history
    r = mk_router(hash_bits=8) if how == "hash_bits" else mk_router()
    if how == "record_slack":
        r.set_record_slack(2)
    r.apply_ops(want)
    assert r.export_table().tobytes() == want.tobytes()
    rc, n, raw = dev_export(r, len(want))
    assert rc == 0 and raw == want.tobytes()
    r.close()


def test_history_device_batch_without_synchronise(history):
    _, _, want = history
    perm = np.random.default_rng(7).permutation(len(want))
    rows = want.view(np.uint8).reshape(-1, 40)[perm].reshape(-1).view(abi.OP_DTYPE)
    cut = len(rows) - len(rows) // 5
    r = mk_router()
    r.apply_ops(rows[:cut])
    d = to_dev(rows[cut:])
    import torch
    torch.cuda.synchronize()
    r.apply_ops_device(d.data_ptr(), len(rows) - cut)
    got = r.export_table()  # right behind the asynchronous batch
    assert got.tobytes() == want.tobytes()
    assert r.update_counts()[0] == 1
    r.close()


def test_capacity(edges):
    _, t, r = edges
    want = t.export().tobytes()
    n = len(want) // 40
    rc, got_n, raw = dev_export(r, 0)
    assert (rc, got_n, raw) == (abi.WQ_E_CAPACITY, n, b"")
    cnt = ctypes.c_size_t()
    assert r.lib.wq_table_export(r.h, None, None, 0, ctypes.byref(cnt)) == abi.WQ_E_CAPACITY and cnt.value == n
    for cap in (n - 1, 64, 65, 1):
        rc, got_n, raw = dev_export(r, cap)
        assert (rc, got_n) == (abi.WQ_E_CAPACITY, n) and raw == want[: cap * 40], cap
        out = np.zeros(cap + 1, abi.OP_DTYPE)
        out.view(np.uint8)[:] = CANARY
        rc = r.lib.wq_table_export(r.h, None, out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(cnt))
        assert (rc, cnt.value) == (abi.WQ_E_CAPACITY, n)
        assert out.view(np.uint8)[: cap * 40].tobytes() == want[: cap * 40] and (out.view(np.uint8)[cap * 40:] == CANARY).all()
    rc, got_n, raw = dev_export(r, n + 100)
    assert (rc, got_n) == (0, n) and raw == want


def test_filters(edges):
    _, t, r = edges
    top = int(t.export()["peer"].max())
    cases = [dict(world=1), dict(peers=[3, 6000, top + 1000]), dict(peers=[top, 0, 0, 2600]),
             dict(world=0, peers=[3, 6000, top + 1000]), dict(peers=[]), dict(world=77), dict(world=BIG_WORLD),
             dict(peers=[0xFFFFFFFE]), dict(world=1, peers=np.arange(0, top + 1, 3))]
    assert 6000 > top or not (t.export()["peer"] == 6000).any()
    for kw in cases:
        want = t.export(**kw).tobytes()
        n = len(want) // 40
        assert r.export_table(**kw).tobytes() == want, kw
        rc, got_n, raw = dev_export(r, n + 3, **kw)
        assert (rc, got_n) == (0, n) and raw == want, kw
        for cap in {n // 2, max(n - 1, 0), min(n, 65)} - {n}:
            rc, got_n, raw = dev_export(r, cap, **kw)
            assert (rc, got_n) == (abi.WQ_E_CAPACITY, n) and raw == want[: cap * 40], (kw, cap)
    assert len(t.export(world=1)) > 0 and len(t.export(peers=[3, 6000, top + 1000])) > 0


def test_round_trip_routes_the_same(history):
    first, steps, want = history
    a = mk_router()
    a.apply_ops(first)
    for s in steps:
        a.apply_ops(s)
    rows = a.export_table()
    assert rows.tobytes() == want.tobytes()
    b = mk_router()
    b.apply_ops(rows)
    assert b.export_table().tobytes() == want.tobytes()
    sa, sb = a.stats(), b.stats()
    assert [sa[k] for k in ("n_entries", "n_cubes", "n_any")] == [sb[k] for k in ("n_entries", "n_cubes", "n_any")]
    o = orc.COracle(16)
    o.apply_ops(first)
    for s in steps:
        o.apply_ops(s)
    rng = np.random.default_rng(8)
    M = 2000
    pick = want[rng.integers(0, len(want), M)]
    k = pick["key"].astype(np.float64)
    pos = k - np.where(k > 0, 1.0, -1.0) * rng.uniform(0.0, 16.0, (M, 3))  # inside a held cube (no axis 0)
    world = pick["world"].copy()
    sender = rng.integers(0, 500, M).astype(np.uint32)
    repl = rng.integers(0, 3, M).astype(np.uint8)
    o_offs, o_peers, _ = o.route(pos, world, sender, repl)
    assert o_offs[-1] > M
    for r in (a, b):
        offs, peers, _ = r.route(pos, world, sender, repl)
        assert (offs == o_offs).all() and (peers == o_peers).all()
    a.close()
    b.close()


@pytest.mark.parametrize("mode", ["cube", "replicate"])
@pytest.mark.parametrize("G", [1, 2, 3])
def test_multi_gpu_handles(G, mode, edges):
    from worldql_server_amd.router import Router
    ops, t, _ = edges
    want = t.export().tobytes()
    n = len(want) // 40
    r = Router.multi(16, [0] * G, mode)
    r.apply_ops(ops)
    assert r.export_table().tobytes() == want
    rc, got_n, raw = dev_export(r, n)
    assert (rc, got_n) == (0, n) and raw == want
    rc, got_n, raw = dev_export(r, 65)
    assert (rc, got_n) == (abi.WQ_E_CAPACITY, n) and raw == want[: 65 * 40]
    kw = dict(world=1, peers=np.arange(0, 4000, 2))
    assert r.export_table(**kw).tobytes() == t.export(**kw).tobytes()
    r.close()


def _hub_run(G, body):
    from worldql_server_amd.router import Hub, Router
    hub = Hub(G)
    routers = [Router(16, 0) for _ in range(G)]
    results, errors = [None] * G, []

    def run(rank):
        try:
            routers[rank].attach_hub(hub, rank)
            results[rank] = body(routers[rank], rank)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=run, args=(k,)) for k in range(G)]
    for x in th:
        x.start()
    for x in th:
        x.join(300)
    assert not errors, errors
    for r in routers:
        r.close()
    hub.close()
    return results


def test_shards_export_what_they_own_and_import(edges):
    from tests.test_gpu_sharded_native import _check, _slice, _tick
    import torch
    ops, t, _ = edges
    want = t.export()

    def body2(r, rank):
        r.sharded_apply_ops(ops)
        return r.export_table()

    parts = _hub_run(2, body2)
    assert all(len(p) for p in parts) and sum(len(p) for p in parts) == len(want)
    assert all(p.tobytes() == snapshot.sort_rows(p).tobytes() for p in parts)
    assert snapshot.sort_rows(abi.concat_ops(parts)).tobytes() == want.tobytes()

    # the same rows on a G = 3 hub route a sharded tick to the one-table CSR
    w = synth.uniform_box(9, 300, 3000, 96.0, neighbourhood=True, repl_mode="mixed", n_worlds=2)
    one = TableRef(16)
    one.apply(w.ops)
    rows = one.export()
    M, G = len(w.world), 3
    dev = torch.device("cuda:0")

    def body3(r, rank):
        r.sharded_apply_ops(rows)
        lo, hi = _slice(M, G, rank)
        return _tick(r, w, lo, hi, dev), r.export_table()

    res = _hub_run(G, body3)
    o = orc.COracle(16)
    o.apply_ops(w.ops)
    for rank in range(G):
        lo, hi = _slice(M, G, rank)
        offs, peers, _ = o.route(w.pos[lo:hi], w.world[lo:hi], w.sender[lo:hi], w.repl[lo:hi])
        _check(res[rank][0], (offs, peers), hi - lo)
    assert snapshot.sort_rows(abi.concat_ops([x[1] for x in res])).tobytes() == rows.tobytes()


def test_follow_state_makes_the_restored_handle_go_on():
    rng = np.random.default_rng(9)
    n = 2000
    world = rng.integers(0, 2, n).astype(np.uint32)
    world[rng.random(n) < 0.05] = abi.WORLD_INVALID
    pos = rng.uniform(-200.0, 200.0, (n, 3))
    a = mk_router()
    a.follow_set_reach(1)
    for _ in range(3):
        a.follow_peers(world, pos)
        pos = pos + rng.uniform(-12.0, 12.0, (n, 3))
    rows = a.export_table()
    fw, fp = a.follow_state()
    assert len(fw) == n and (fw == world).all() and (fp[fw == abi.WORLD_INVALID] == 0.0).all()
    t = TableRef(16)
    t.apply(rows)
    assert t.export().tobytes() == rows.tobytes()

    b, b2 = mk_router(), mk_router()
    for r in (b, b2):
        r.apply_ops(rows)
    b.follow_set_reach(1)
    b.follow_state_load(fw, fp)
    world4 = world.copy()
    world4[:50] = abi.WORLD_INVALID  # some stop being followed
    ra = a.follow_peers(world4, pos)
    rb = b.follow_peers(world4, pos)
    rb2 = b2.follow_peers(world4, pos)
    assert ra == rb and ra["n_unsubscribe"] > 0
    assert a.follow_last_ops().tobytes() == b.follow_last_ops().tobytes()
    after = a.export_table()
    assert b.export_table().tobytes() == after.tobytes()
    fa, fb = a.follow_state(), b.follow_state()
    assert fa[0].tobytes() == fb[0].tobytes() and fa[1].tobytes() == fb[1].tobytes()
    # without the state every peer subscribes its whole neighbourhood again and never leaves the
    # cubes it has left since: more subscribes, a larger table
    assert rb2["n_subscribe"] > ra["n_subscribe"] and rb2["n_unsubscribe"] == 0
    assert len(b2.export_table()) > len(after)
    for r in (a, b, b2):
        r.close()


def test_errors(edges):
    _, t, r = edges
    lib = r.lib
    n = ctypes.c_size_t()
    assert lib.wq_table_export(None, None, None, 0, ctypes.byref(n)) == abi.WQ_E_INVALID
    assert lib.wq_table_export_device(None, None, None, 0, ctypes.byref(n)) == abi.WQ_E_INVALID
    assert lib.wq_table_export(r.h, None, None, 0, None) == abi.WQ_E_INVALID
    assert lib.wq_table_export_device(r.h, None, None, 0, None) == abi.WQ_E_INVALID
    assert lib.wq_table_export(r.h, None, None, 5, ctypes.byref(n)) == abi.WQ_E_INVALID
    # a null peers pointer is "every peer", whatever n_peers says
    f = abi.ExportFilter(1, 7, None)
    want = t.export(world=1)
    out = np.zeros(len(want), abi.OP_DTYPE)
    assert lib.wq_table_export(r.h, ctypes.byref(f), out.ctypes.data_as(ctypes.c_void_p), len(out), ctypes.byref(n)) == 0
    assert n.value == len(want) and out.tobytes() == want.tobytes()
    # follow state
    assert lib.wq_follow_state_read(None, None, None, 0, ctypes.byref(n)) == abi.WQ_E_INVALID
    assert lib.wq_follow_state_load(None, None, None, 0) == abi.WQ_E_INVALID
    q = mk_router()
    assert q.export_table().tobytes() == b"" and len(q.follow_state()[0]) == 0
    w = np.array([0, abi.WORLD_INVALID, 1], np.uint32)
    p = np.array([[1.0, 2.0, 3.0], [9.0, 9.0, 9.0], [-1.0, -2.0, -3.0]])
    q.follow_state_load(w, p)
    gw, gp = q.follow_state()
    assert (gw == w).all() and gp.tolist() == [[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -3.0]]
    ow, op_ = np.full(3, 7, np.uint32), np.full((3, 3), 7.0)
    rc = lib.wq_follow_state_read(q.h, ow.ctypes.data_as(ctypes.c_void_p), op_.ctypes.data_as(ctypes.c_void_p), 2,
                                  ctypes.byref(n))
    assert (rc, n.value) == (abi.WQ_E_CAPACITY, 3)
    assert ow.tolist() == [0, abi.WORLD_INVALID, 7] and op_[2].tolist() == [7.0, 7.0, 7.0]
    from worldql_server_amd.router import WQError
    with pytest.raises(WQError) as e:  # two peers are followed now
        q.follow_state_load(w, p)
    assert e.value.code == abi.WQ_E_INVALID
    res = q.follow_peers(np.full(3, abi.WORLD_INVALID, np.uint32), p)  # n_followed counted from the load
    assert res["n_followed"] == 0 and res["n_unsubscribe"] == 2 * 27
    q.follow_state_load(w, p)
    q.close()


def test_processor_snapshot_restore():
    from tests.seq_reference import random_events
    from worldql_server_amd.processing import DISCONNECT, Message, SubscriptionProcessor
    from worldql_server_amd.subscriptions import CubeArea, WorldMap
    events = random_events(4000, seed=3, n_peers=300)
    p1 = SubscriptionProcessor(WorldMap(16, device=0))
    for i in range(0, 3000, 250):
        p1.process_tick(events[i:i + 250])
    w1 = p1.world_map
    live = [u for u in w1.peer_ids.snapshot()["peers"] if u is not None]
    p1.process_tick([Message(DISCONNECT, u) for u in live[3:8]])  # ids on the free list at the snapshot
    p2 = SubscriptionProcessor.restore(p1.snapshot())
    w2 = p2.world_map
    assert w2.router is not w1.router
    assert w2.peer_ids.snapshot() == w1.peer_ids.snapshot() and len(w1.peer_ids.snapshot()["free"]) > 0
    assert [w2.worlds.name(i) for i in range(len(w2.worlds))] == [w1.worlds.name(i) for i in range(len(w1.worlds))]
    assert w2.router.export_table().tobytes() == w1.router.export_table().tobytes()
    some = 0
    for i in range(3000, 4000, 100):
        r1, r2 = p1.process_tick(events[i:i + 100]), p2.process_tick(events[i:i + 100])
        assert r1 == r2
        some += sum(1 for x in r1 if isinstance(x, list) and x)
    assert some > 50
    rows = w1.router.export_table()
    assert w2.router.export_table().tobytes() == rows.tobytes() and len(rows) > 0
    # the per-peer listing through the façade
    pid, wid = int(rows["peer"][0]), int(rows["world"][0])
    am = w1.get(w1.worlds.name(wid))
    mine = rows[(rows["peer"] == pid) & (rows["world"] == wid)]
    assert am.subscriptions_of(w1.peer_ids.peer(pid)) == [CubeArea(*k) for k in mine["key"].tolist()]
    assert am.subscriptions_of("nobody") == []


def test_cpp_mirror_export_and_restore(tmp_path):
    """tests/cpp/test_snapshot.cpp: WorldMap::export_ops and AreaMap::subscriptions_of of
    cpp/world_map.hpp against hand-written expectations, then a restore."""
    import os
    import subprocess
    from worldql_server_amd.build import LIB
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "test_snapshot")
    libdir = os.path.dirname(LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(root, "include"),
                           "-I", os.path.join(root, "worldql_server_amd", "cpp"),
                           os.path.join(root, "tests", "cpp", "test_snapshot.cpp"), "-o", out,
                           "-L", libdir, "-lwq_router", f"-Wl,-rpath,{libdir}",
                           "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
