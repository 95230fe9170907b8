"""The follow path's host reference (worldql_server_amd/follow.py), without a GPU.

`follow_ops_np` is the normative semantics of wq_follow_peers in numpy: an exact per-axis set
difference of the old and new neighbourhoods. Here it is pinned against a brute force that quantises
every offset position with the oracle's quantiser, against the benchmarks' generator
(`synth_ext._moves_to_ops`) where that one is right, and against the C oracle's table state.
"""
import itertools

import numpy as np
import pytest

from oracle import oracle as orc
from worldql_server_amd import abi, follow, synth_ext

INV = abi.WORLD_INVALID
UP, DN = np.inf, -np.inf
EDGES = [0.0, -0.0, 8.0, -8.0, 16.0, -16.0, np.nextafter(16.0, UP), -np.nextafter(16.0, UP),
         np.nextafter(16.0, 0.0), -np.nextafter(16.0, 0.0), 24.0, 32.0, -32.0, 1e300, np.nan]


def brute_force(ow, op, nw, npos, s, reach):
    """{(kind, world, peer, cube)} by quantising all (2r+1)^3 offset positions of both states."""
    offs = np.array(list(itertools.product(range(-reach, reach + 1), repeat=3)), np.float64)
    out = set()
    for i in range(len(nw)):
        with np.errstate(all="ignore"):
            O = set() if ow[i] == INV else {(int(ow[i]),) + tuple(k) for k in orc.quantize_np(op[i] + s * offs, s).tolist()}
            N = set() if nw[i] == INV else {(int(nw[i]),) + tuple(k) for k in orc.quantize_np(npos[i] + s * offs, s).tolist()}
        out |= {(abi.OP_UNSUBSCRIBE, c[0], i, c[1:]) for c in O - N}
        out |= {(abi.OP_SUBSCRIBE, c[0], i, c[1:]) for c in N - O}
    return out


def op_set(ops, s):
    assert (ops["key_is_raw"] == 0).all()
    with np.errstate(all="ignore"):
        k = orc.quantize_np(ops["pos"], s)
    t = [(int(a), int(b), int(c), tuple(d)) for a, b, c, d in zip(ops["kind"], ops["world"], ops["peer"], k.tolist())]
    assert len(set(t)) == len(t), "an op appears twice"
    return set(t)


def check_order(ops):
    """Ascending peers; within a peer the unsubscribes before the subscribes."""
    key = ops["peer"].astype(np.int64) * 2 + (ops["kind"] == abi.OP_SUBSCRIBE)
    assert (np.diff(key) >= 0).all()


def edge_cases():
    """Old and new positions from the edge values: every (old, new) pair on one axis, then random
    picks on all three; with moves, starts, stops and world changes mixed in."""
    rng = np.random.default_rng(3)
    E = np.array(EDGES)
    pairs = np.array(list(itertools.product(range(len(E)), repeat=2)))
    old = np.full((len(pairs), 3), 8.0)
    new = np.full((len(pairs), 3), 8.0)
    ax = np.arange(len(pairs)) % 3
    old[np.arange(len(pairs)), ax] = E[pairs[:, 0]]
    new[np.arange(len(pairs)), ax] = E[pairs[:, 1]]
    n_r = 400
    old = np.concatenate([old, E[rng.integers(0, len(E), (n_r, 3))]])
    new = np.concatenate([new, E[rng.integers(0, len(E), (n_r, 3))]])
    n = len(old)
    ow = np.zeros(n, np.uint32)
    nw = np.zeros(n, np.uint32)
    kind = rng.integers(0, 8, n)
    ow[kind == 5] = INV          # start
    nw[kind == 6] = INV          # stop
    nw[kind == 7] = 3            # world change
    return ow, old, nw, new


@pytest.mark.parametrize("cube_size", [16, 10])
@pytest.mark.parametrize("reach", [0, 1, 2])
def test_brute_force_edges(cube_size, reach):
    ow, old, nw, new = edge_cases()
    ops = follow.follow_ops_np(ow, old, nw, new, cube_size, reach)
    check_order(ops)
    assert op_set(ops, cube_size) == brute_force(ow, old, nw, new, cube_size, reach)
    assert (ops.view(np.uint8).reshape(-1, 40)[:, 10:16] == 0).all()


@pytest.mark.parametrize("a,b", [(8.0, 16.0), (8.0, 0.0), (8.0, -0.0), (24.0, np.nextafter(16.0, 32.0))])
def test_cell_edge_moves_the_generator_misses(a, b):
    """The own cell stays (16), the neighbourhood shrinks from 27 to 18 cubes: 9 unsubscribes."""
    old = np.array([[a, 8.0, 8.0]])
    new = np.array([[b, 8.0, 8.0]])
    w = np.zeros(1, np.uint32)
    ops = follow.follow_ops_np(w, old, w, new, 16, 1)
    assert int((ops["kind"] == abi.OP_UNSUBSCRIBE).sum()) == 9
    assert int((ops["kind"] == abi.OP_SUBSCRIBE).sum()) == 0
    assert op_set(ops, 16) == brute_force(w, old, w, new, 16, 1)
    # the benchmarks' generator skips the peer: its own cell did not change
    assert len(synth_ext._moves_to_ops(w, np.zeros(1, np.uint32), old, new, 16)) == 0


def test_random_moves_match_the_generator():
    rng = np.random.default_rng(1)
    n = 2000
    old = rng.uniform(-100.0, 100.0, (n, 3))
    new = old + rng.uniform(-4.0, 4.0, (n, 3))
    w = np.zeros(n, np.uint32)
    ops = follow.follow_ops_np(w, old, w, new, 16, 1)
    gen = synth_ext._moves_to_ops(w, np.arange(n, dtype=np.uint32), old, new, 16)
    assert len(ops) == len(gen) == 12350
    assert op_set(ops, 16) == op_set(gen, 16)
    check_order(ops)


def test_oracle_state_after_start_move_world_change_stop():
    rng = np.random.default_rng(7)
    n, s = 60, 16
    st = follow.FollowState(s, 1)
    o = orc.COracle(s)
    nb = np.array(list(itertools.product((-1.0, 0.0, 1.0), repeat=3)))
    pos = rng.uniform(-64.0, 64.0, (n, 3))
    pos[0] = [8.0, 16.0, -0.0]
    pos[1] = [np.nextafter(16.0, 32.0), -16.0, 32.0]
    world = np.zeros(n, np.uint32)
    seen = set()

    def step(world, pos):
        o.apply_ops(st.follow(world, pos))
        want = set()
        for i in range(len(world)):
            if world[i] != INV:
                want |= {(int(world[i]), i) + tuple(k) for k in orc.quantize_np(pos[i] + s * nb, s).tolist()}
        seen.update(want)
        assert o.counts()[0] == len(want)
        for c in seen:  # every cube ever involved: subscribed iff in the final neighbourhoods
            assert o.is_subscribed(c[0], c[1], True, np.array(c[2:], np.int64)) == (c in want)

    step(world, pos)                                            # start
    pos = pos + rng.uniform(-12.0, 12.0, (n, 3))
    pos[0] = [16.0, 8.0, 0.0]
    step(world, pos)                                            # move
    world = world.copy()
    world[::3] = 2
    step(world, pos)                                            # world change
    world[1::4] = INV
    step(world, pos + 1.0)                                      # stop (and a small move)
    step(np.full(n, INV, np.uint32), pos)                       # everybody stops
    assert o.counts() == (0, 0)
    assert st.n_followed() == 0


def test_stream_is_deterministic_and_padded_with_zeros():
    ow, old, nw, new = edge_cases()
    a = follow.follow_ops_np(ow, old, nw, new, 16, 2)
    b = follow.follow_ops_np(ow.copy(), old.copy(), nw.copy(), new.copy(), 16, 2)
    assert a.tobytes() == b.tobytes()
    raw = a.view(np.uint8).reshape(-1, 40)
    assert (raw[:, 10:16] == 0).all() and len(a) > 0


def test_reach_is_checked():
    z = np.zeros(1, np.uint32)
    with pytest.raises(ValueError):
        follow.follow_ops_np(z, np.zeros((1, 3)), z, np.zeros((1, 3)), 16, 3)
