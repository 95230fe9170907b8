"""Follow moving peers on the GPU (wq_follow_peers*, csrc/wq_follow.hip): the handle turns world
ids and positions into the subscribe / unsubscribe ops of each move and applies them.

Bars: the op stream (`follow_last_ops`) is byte-identical to the host reference
(`worldql_server_amd/follow.py` follow_ops_np); the table it leaves routes exactly like the oracle
fed the reference's ops.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from worldql_server_amd import abi, follow, synth, synth_ext

from test_follow_host import edge_cases

pytestmark = pytest.mark.gpu

INV = abi.WORLD_INVALID


def mk_router(cube_size=16):
    from worldql_server_amd.router import Router
    return Router(cube_size, 0)


def _same(got, want):
    assert (got[0] == want[0]).all()
    assert (got[1] == want[1]).all()
    return len(want[1])


def _route(r, pos, w, s, rp):
    # room for every pair at once: a capacity retry would leave the overflow word set
    return r.route(pos, w, s, rp, capacity=256 * max(len(w), 16))


def _clean(r):
    assert r.route_health() == (0, 0)
    r.close()


def _follow_exact(r, st, world, pos):
    """One follow call on the router and on the host state: byte-identical streams, same counts."""
    want = st.follow(world, pos)
    res = r.follow_peers(world, pos)
    got = r.follow_last_ops()
    n_un = int((want["kind"] == abi.OP_UNSUBSCRIBE).sum())
    assert (res["n_unsubscribe"], res["n_subscribe"]) == (n_un, len(want) - n_un)
    assert res["n_followed"] == st.n_followed()
    assert len(got) == len(want)
    assert got.tobytes() == want.tobytes()
    return want


@pytest.mark.parametrize("cube_size", [16, 10])
@pytest.mark.parametrize("reach", [0, 1, 2])
def test_exact_op_stream(cube_size, reach):
    for n in (1, 63, 64, 65, 257, 4000):
        rng = np.random.default_rng(100 + n)
        r = mk_router(cube_size)
        r.follow_set_reach(reach)
        st = follow.FollowState(cube_size, reach)
        o = orc.COracle(cube_size)
        world = (np.arange(n) % 3).astype(np.uint32)
        pos = rng.uniform(-100.0, 100.0, (n, 3))
        ops = _follow_exact(r, st, world, pos)                         # first call: all subscribes
        assert (ops["kind"] == abi.OP_SUBSCRIBE).all() and len(ops) > 0
        o.apply_ops(ops)
        pos = pos + rng.uniform(-6.0, 6.0, (n, 3))
        o.apply_ops(_follow_exact(r, st, world, pos))                  # a move
        world = world.copy()
        world[::4] = 7
        o.apply_ops(_follow_exact(r, st, world, pos))                  # a world change for some
        world[1::5] = INV
        o.apply_ops(_follow_exact(r, st, world, pos + 1.0))            # a stop for some (and a move)
        m = max(1, n // 2)                                             # a smaller n: later peers stay
        o.apply_ops(_follow_exact(r, st, world[:m], pos[:m] + 20.0))
        o.apply_ops(_follow_exact(r, st, world, pos + 1.0))            # ... and are still where they were
        s = r.stats()
        assert (s["n_entries"], s["n_cubes"]) == o.counts()
        _clean(r)


@pytest.mark.parametrize("cube_size", [16, 10])
@pytest.mark.parametrize("reach", [0, 1, 2])
def test_exact_op_stream_edge_values(cube_size, reach):
    """0.0, -0.0, +-8, +-16 and their neighbours, 24, +-32, 1e300, NaN on every axis: cell edges where
    the neighbourhood shrinks, and keys without a packed form."""
    ow, old, nw, new = edge_cases()
    r = mk_router(cube_size)
    r.follow_set_reach(reach)
    st = follow.FollowState(cube_size, reach)
    o = orc.COracle(cube_size)
    o.apply_ops(_follow_exact(r, st, ow, old))
    o.apply_ops(_follow_exact(r, st, nw, new))
    s = r.stats()
    assert (s["n_entries"], s["n_cubes"]) == o.counts()
    _clean(r)


def test_cell_edge_moves_shrink_the_neighbourhood():
    r = mk_router()
    st = follow.FollowState(16, 1)
    old = np.array([[8.0, 8.0, 8.0], [8.0, 8.0, 8.0], [8.0, 8.0, 8.0], [24.0, 8.0, 8.0]])
    new = np.array([[16.0, 8.0, 8.0], [0.0, 8.0, 8.0], [-0.0, 8.0, 8.0], [np.nextafter(16.0, 32.0), 8.0, 8.0]])
    w = np.zeros(4, np.uint32)
    _follow_exact(r, st, w, old)
    ops = _follow_exact(r, st, w, new)
    assert len(ops) == 36 and (ops["kind"] == abi.OP_UNSUBSCRIBE).all()
    assert r.stats()["n_entries"] == 4 * 18
    _clean(r)


def test_c5_shape_follow_only():
    c5 = synth_ext.config_c5(scale=0.004)
    n = c5.n
    r, o = mk_router(), orc.COracle(16)
    st = follow.FollowState(16, 1)
    r.set_radius(c5.radius)
    world = np.zeros(n, np.uint32)
    for tick in range(4):
        o.apply_ops(st.follow(world, c5.pos))
        r.follow_peers(world, c5.pos)
        r.set_peer_positions(c5.pos)
        pos, w, s, _ = c5.messages()
        rp = synth.stream(5, 70 + tick).below(3, len(w)).astype(np.uint8)
        P = _same(_route(r, pos, w, s, rp), o.route_radius(pos, w, s, rp, c5.pos, c5.radius))
        assert P > 0
        assert r.stats()["n_entries"] == o.counts()[0]
        c5.step()  # the entities move; the generator's own ops are not used
    assert r.update_counts()[0] >= 1
    _clean(r)


def test_c4_shape_follow_only():
    c4 = synth_ext.config_c4(scale=0.01, worlds=range(4))
    r, o = mk_router(), orc.COracle(16)
    st = follow.FollowState(16, 1)
    o.apply_ops(st.follow(c4.world, c4.pos))
    r.follow_peers(c4.world, c4.pos)
    for tick in range(3):
        _, pos, w, s, rp = c4.step(move_frac=0.05)
        o.apply_ops(st.follow(c4.world, c4.pos))
        r.follow_peers(c4.world, c4.pos)
        assert r.stats()["n_entries"] == o.counts()[0]
        assert _same(_route(r, pos, w, s, rp), o.route(pos, w, s, rp)) > 0
    _clean(r)


def test_irregular_peers_take_the_rebuild():
    rng = np.random.default_rng(17)
    n = 300
    r, o = mk_router(), orc.COracle(16)
    st = follow.FollowState(16, 1)
    world = np.zeros(n, np.uint32)
    pos = rng.uniform(-60.0, 60.0, (n, 3))

    def tick(world, pos):
        o.apply_ops(_follow_exact(r, st, world, pos))
        mpos = np.concatenate([pos, rng.uniform(-60.0, 60.0, (200, 3))])
        mw = np.concatenate([world, np.zeros(200, np.uint32)])
        mw[mw == INV] = 0
        ms = rng.integers(0, n, len(mw)).astype(np.uint32)
        mr = rng.integers(0, 3, len(mw)).astype(np.uint8)
        assert _same(_route(r, mpos, mw, ms, mr), o.route(mpos, mw, ms, mr)) > 0
        s = r.stats()
        assert (s["n_entries"], s["n_cubes"]) == o.counts()

    tick(world, pos)                       # the table is built
    fb0 = r.update_counts()[1]
    world, pos = world.copy(), pos.copy()
    pos[5] = [1e300, 3.0, 4.0]             # no packed key: huge
    pos[6] = [np.nan, 3.0, 4.0]            # NaN
    world[7] = 1 << 24                     # world id past the packed range
    tick(world, pos)
    assert r.update_counts()[1] > fb0      # the incremental update gave the batch to the rebuild
    tick(world, pos + rng.uniform(-5.0, 5.0, (n, 3)))   # a normal tick after it
    _clean(r)


def test_device_form_then_route_without_synchronise():
    import torch
    rng = np.random.default_rng(23)
    n = 3000
    dev = torch.device("cuda:0")
    world = (np.arange(n) % 2).astype(np.uint32)
    p0 = rng.uniform(-80.0, 80.0, (n, 3))
    # small moves: ~3 ops per peer, a batch under 1/4 of the 81,000 entries, so the update is the
    # incremental one, which the device form leaves in flight
    p1 = p0 + rng.uniform(-2.0, 2.0, (n, 3))
    sender = rng.integers(0, n, n).astype(np.uint32)
    repl = rng.integers(0, 3, n).astype(np.uint8)
    # the synchronised result: host forms
    a = mk_router()
    a.follow_peers(world, p0)
    a.follow_peers(world, p1)
    want = _route(a, p1, world, sender, repl)
    want_ops = a.follow_last_ops()
    # device form, then the tick at once on the same stream
    b = mk_router()
    d_w = torch.from_numpy(world.view(np.int32)).to(dev)
    d_p0 = torch.from_numpy(p0).to(dev)
    d_p1 = torch.from_numpy(p1).to(dev)
    d_s = torch.from_numpy(sender.view(np.int32)).to(dev)
    d_r = torch.from_numpy(repl).to(dev)
    cap = len(want[1]) + 64
    d_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    d_peers = torch.empty(cap, dtype=torch.int32, device=dev)
    cnt = torch.zeros(24, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    res0 = b.follow_peers_device(d_w.data_ptr(), d_p0.data_ptr(), n)
    assert res0["n_unsubscribe"] == 0 and res0["n_followed"] == n
    res1 = b.follow_peers_device(d_w.data_ptr(), d_p1.data_ptr(), n)
    b.route_device(d_p1.data_ptr(), d_w.data_ptr(), d_s.data_ptr(), d_r.data_ptr(), n, d_off.data_ptr(),
                   d_peers.data_ptr(), None, cap, cnt.data_ptr())
    assert res1["n_unsubscribe"] + res1["n_subscribe"] == len(want_ops)
    assert b.follow_last_ops().tobytes() == want_ops.tobytes()   # (synchronises the handle's stream)
    c = cnt.cpu().numpy().view(abi.COUNTERS_DTYPE)[0]
    assert int(c["n_pairs"]) == len(want[1]) and c["overflow"] == 0 and c["error"] == 0
    assert (d_off.cpu().numpy().view(np.uint32) == want[0]).all()
    assert (d_peers[:len(want[1])].cpu().numpy().view(np.uint32) == want[1]).all()
    assert b.update_counts()[0] >= 1
    _clean(a)
    _clean(b)


@pytest.mark.parametrize("mode", ["cube", "replicate"])
def test_multi_gpu_handles_follow(mode):
    from worldql_server_amd.router import Router
    rng = np.random.default_rng(29)
    n = 2000
    world = (np.arange(n) % 3).astype(np.uint32)
    p0 = rng.uniform(-70.0, 70.0, (n, 3))
    p1 = p0 + rng.uniform(-6.0, 6.0, (n, 3))
    w1 = world.copy()
    w1[::50] = INV
    sender = rng.integers(0, n, n).astype(np.uint32)
    repl = rng.integers(0, 3, n).astype(np.uint8)
    mw = np.where(w1 == INV, 0, w1).astype(np.uint32)
    single, multi = mk_router(), Router.multi(16, (0, 0), mode=mode)
    st = follow.FollowState(16, 1)
    for r in (single, multi):
        r.follow_peers(world, p0)
        r.follow_peers(w1, p1)
    st.follow(world, p0)
    want_ops = st.follow(w1, p1)
    assert multi.follow_last_ops().tobytes() == want_ops.tobytes()
    want = _route(single, p1, mw, sender, repl)
    assert _same(_route(multi, p1, mw, sender, repl), want) > 0
    assert multi.stats()["n_entries"] == single.stats()["n_entries"]
    assert multi.route_health()[0] == 0
    multi.close()
    _clean(single)


def test_errors():
    from worldql_server_amd.router import WQError
    r = mk_router()
    with pytest.raises(WQError) as e:
        r.follow_set_reach(3)
    assert e.value.code == abi.WQ_E_INVALID
    r.follow_set_reach(2)
    r.follow_set_reach(1)
    r.follow_peers(np.zeros(3, np.uint32), np.ones((3, 3)))
    with pytest.raises(WQError) as e:
        r.follow_set_reach(0)
    assert e.value.code == abi.WQ_E_INVALID
    assert r.stats()["n_entries"] == 3 * 27
    r.follow_reset()
    r.follow_set_reach(0)                        # accepted: nobody is followed
    res = r.follow_peers(np.zeros(3, np.uint32), np.ones((3, 3)))
    assert res["n_unsubscribe"] == 0 and res["n_subscribe"] == 3 and res["n_followed"] == 3   # reset emitted nothing
    with pytest.raises(WQError) as e:
        r.follow_peers_device(0, 0, 5)           # null arrays with n > 0
    assert e.value.code == abi.WQ_E_INVALID
    assert r.follow_peers_device(0, 0, 0)["n_followed"] == 3
    _clean(r)
