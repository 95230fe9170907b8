"""Table snapshots on the host: snapshot.TableRef (the definition of wq_table_export's rows), the
snapshot file and the host maps' snapshot / restore. No GPU."""
import numpy as np
import pytest

from oracle import oracle as orc
from worldql_server_amd import abi, snapshot
from worldql_server_amd.snapshot import TableRef
from worldql_server_amd.subscriptions import PeerIds

S, U, R = abi.OP_SUBSCRIBE, abi.OP_UNSUBSCRIBE, abi.OP_REMOVE_PEER
BIG_WORLD = (1 << 24) + 5  # no packed form on the device (>= 2^24 - 1)


def ops_of(rows):
    """rows: (world, peer, kind, key) with a raw key, or (world, peer, kind, None, pos)."""
    return np.array([abi.make_op(r[0], r[1], r[2], key=r[3]) if r[3] is not None
                     else abi.make_op(r[0], r[1], r[2], pos=r[4] if len(r) > 4 else None) for r in rows],
                    dtype=abi.OP_DTYPE)


def triples(rows):
    return [(int(r["world"]), tuple(int(v) for v in r["key"]), int(r["peer"])) for r in rows]


def ref_of(rows, cube_size=16):
    t = TableRef(cube_size)
    t.apply(ops_of(rows))
    return t


def test_rows_are_raw_subscribes_with_zero_padding():
    out = ref_of([(1, 2, S, (16, -32, 48))]).export()
    assert out.dtype == abi.OP_DTYPE and len(out) == 1
    b = out.view(np.uint8)
    assert b[8] == abi.OP_SUBSCRIBE and b[9] == 1 and not b[10:16].any()
    assert triples(out) == [(1, (16, -32, 48), 2)]


def test_order_negative_axes_two_worlds_and_off_grid_key():
    rows = [(1, 5, S, (16, 0, 0)), (0, 9, S, (16, 0, 0)), (0, 3, S, (-16, 32, 0)), (0, 3, S, (-16, -32, 0)),
            (0, 3, S, (-32, 0, 0)), (0, 7, S, (16, 0, 0)), (0, 4, S, (7, 1, 1)),  # off grid: between -16.. and 16
            (0, 4, S, (16, 0, -16)), (BIG_WORLD, 1, S, (0, 0, 0)), (0, 2, S, None, (1.0, -1.0, 0.0))]
    got = triples(ref_of(rows).export())
    assert got == [
        (0, (-32, 0, 0), 3), (0, (-16, -32, 0), 3), (0, (-16, 32, 0), 3), (0, (7, 1, 1), 4),
        (0, (16, -16, 16), 2),  # from_vector3((1, -1, 0)) at cube size 16
        (0, (16, 0, -16), 4), (0, (16, 0, 0), 7), (0, (16, 0, 0), 9), (1, (16, 0, 0), 5), (BIG_WORLD, (0, 0, 0), 1)]
    # signed order on i64, unsigned on world and peer
    t = ref_of([(0, 0xFFFFFFFE, S, (-(1 << 62), 0, 0)), (0, 1, S, (1 << 62, 0, 0)), (0xFFFFFFFE, 0, S, (0, 0, 0)),
                (0, 1, S, (-(1 << 62), 0, 0))])
    assert triples(t.export()) == [(0, (-(1 << 62), 0, 0), 1), (0, (-(1 << 62), 0, 0), 0xFFFFFFFE),
                                    (0, (1 << 62, 0, 0), 1), (0xFFFFFFFE, (0, 0, 0), 0)]


def test_last_op_wins_and_emptied_cube():
    k, k2 = (16, 16, 16), (32, 16, 16)
    t = ref_of([(0, 1, S, k), (0, 1, U, k), (0, 2, S, k2), (0, 2, U, k2), (0, 2, S, k2), (0, 3, U, k), (0, 1, S, k),
                (0, 1, S, k), (0, 4, S, (48, 0, 0)), (0, 4, U, (48, 0, 0))])
    assert triples(t.export()) == [(0, k, 1), (0, k2, 2)]
    assert t.counts() == {"n_entries": 2, "n_cubes": 2, "n_any": 2}  # the emptied cube is gone


def test_remove_peer_one_world_and_every_world():
    base = [(0, 1, S, (0, 0, 0)), (1, 1, S, (0, 0, 0)), (0, 2, S, (0, 0, 0)), (1, 2, S, (16, 0, 0))]
    one = ref_of(base + [(1, 1, R, (0, 0, 0)), (1, 1, S, (32, 0, 0))])
    assert triples(one.export()) == [(0, (0, 0, 0), 1), (0, (0, 0, 0), 2), (1, (16, 0, 0), 2), (1, (32, 0, 0), 1)]
    every = ref_of(base + [(abi.WORLD_INVALID, 1, R, (0, 0, 0))])
    assert triples(every.export()) == [(0, (0, 0, 0), 2), (1, (16, 0, 0), 2)]


def test_filters():
    t = ref_of([(0, 1, S, (0, 0, 0)), (0, 2, S, (0, 0, 0)), (1, 1, S, (0, 0, 0)), (1, 3, S, (16, 0, 0)),
                (2, 2, S, (0, 0, 0))])
    assert triples(t.export(world=1)) == [(1, (0, 0, 0), 1), (1, (16, 0, 0), 3)]
    assert triples(t.export(peers=[3, 1, 1, 77])) == [(0, (0, 0, 0), 1), (1, (0, 0, 0), 1), (1, (16, 0, 0), 3)]
    assert triples(t.export(world=1, peers=[1, 2])) == [(1, (0, 0, 0), 1)]
    assert len(t.export(peers=[])) == 0 and t.export(peers=[]).dtype == abi.OP_DTYPE
    assert len(t.export(peers=[77, 0xFFFFFFFE])) == 0
    assert len(t.export(world=9)) == 0
    assert triples(t.subscriptions_of(2)) == [(0, (0, 0, 0), 2), (2, (0, 0, 0), 2)]
    assert t.export().tobytes() == snapshot.sort_rows(t.export()[::-1]).tobytes()


def random_ops(n, seed, cube_size=16):
    rng = np.random.default_rng(seed)
    world = rng.integers(0, 3, n).astype(np.uint32)
    peer = rng.integers(0, 40, n).astype(np.uint32)
    kind = rng.choice([S, S, S, U, U, R], n).astype(np.uint8)
    pos = rng.uniform(-40.0, 40.0, (n, 3))
    ops = abi.ops_array(world, peer, kind, pos=pos)
    raw = rng.random(n) < 0.3  # raw keys, some off the grid
    ops["key_is_raw"][raw] = 1
    ops["key"][raw] = rng.integers(-3, 4, (int(raw.sum()), 3)) * cube_size + (rng.random((int(raw.sum()), 3)) < 0.1)
    ops["world"][(kind == R) & (rng.random(n) < 0.5)] = abi.WORLD_INVALID
    return ops


def test_cross_check_with_the_oracle_on_random_ops():
    ops = random_ops(5000, 11)
    t = TableRef(16)
    t.apply(ops)
    o = orc.COracle(16)
    o.apply_ops(ops)
    out = t.export()
    c = t.counts()
    assert (c["n_entries"], c["n_cubes"]) == o.counts() and len(out) == c["n_entries"]
    assert out.tobytes() == snapshot.sort_rows(out).tobytes() and len(set(triples(out))) == len(out)
    for r in out:  # every exported row is a subscription of the oracle's ...
        assert o.is_subscribed(int(r["world"]), int(r["peer"]), True, r["key"])
    held = set(triples(out))  # ... and every (world, cube, peer) an op ever named agrees
    named = TableRef(16)
    sub = ops[ops["kind"] != R].copy()
    sub["kind"] = S
    named.apply(sub)
    probes = triples(named.export())
    assert len(probes) > len(out)
    for w, k, p in probes:
        assert o.is_subscribed(w, p, True, np.array(k, np.int64)) == ((w, k, p) in held)
    # a rebuild from the rows is the same table
    again = TableRef(16)
    again.apply(out)
    assert again.export().tobytes() == out.tobytes()


def test_snapshot_file_round_trip_and_cube_size_check(tmp_path):
    t = TableRef(10)
    t.apply(random_ops(400, 3, 10))
    fw = np.array([0, abi.WORLD_INVALID, 2], np.uint32)
    fp = np.array([[1.5, -2.0, 3.0], [0.0, 0.0, 0.0], [np.nan, 1e300, -0.0]])
    snap = snapshot.Snapshot(10, t.export(), 2, fw, fp)
    path = tmp_path / "table.npz"
    snapshot.save(path, snap)
    got = snapshot.load(path, cube_size=10)
    assert got.cube_size == 10 and got.follow_reach == 2
    assert got.ops.dtype == abi.OP_DTYPE and got.ops.tobytes() == snap.ops.tobytes()
    assert got.follow_world.tobytes() == fw.tobytes() and got.follow_pos.tobytes() == fp.tobytes()
    assert snapshot.load(path).cube_size == 10
    with pytest.raises(ValueError, match="cube_size"):
        snapshot.load(path, cube_size=16)

    class FakeRouter:
        cube_size = 16

    with pytest.raises(ValueError, match="cube_size"):
        snapshot.restore(FakeRouter(), got)


def test_peer_ids_snapshot_keeps_ids_and_free_list():
    a = PeerIds()
    for u in "abcdef":
        a.id(u)
    a.release("b")
    a.release("e")
    b = PeerIds.restore(a.snapshot())
    assert b.high_water == a.high_water == 6 and len(b) == 4
    assert [b.lookup(u) for u in "abcdef"] == [0, None, 2, 3, None, 5]
    assert b.peer(3) == "d" and b.peer(1) is None
    # the next ids come off the free list in the same order on both
    assert [a.id(u) for u in ("x", "y", "z")] == [b.id(u) for u in ("x", "y", "z")] == [4, 1, 6]
    bad = a.snapshot()
    bad["free"] = [0]
    with pytest.raises(ValueError):
        PeerIds.restore(bad)
