"""CPU: the ingest joins' definition (worldql_server_amd/ingest.py join_peers_np, drop_peers_np) and the
shared case list of the mirror (tests/test_ingest_join_cpp_mirror.py) and GPU (tests/test_gpu_ingest_join.py)
tests.

  - every named case against a straight restatement: the frames one at a time, a subscribe that passes the
    reference's checks asks the allocator for the sender's id exactly as SubscriptionProcessor._apply_run
    asks PeerIds.id, every other frame looks the sender up as _sender_id does;
  - the overflow cases change nothing and say what was needed;
  - 300 random small ticks through a real PeerIds: after join_peers_np the dispatch defers nothing when
    every world resolves, and j_id is what PeerIds.id hands out in arrival order; PeerIds.adopt leaves the
    host map equal to the sequential one;
  - the leave side, and PeerIds.adopt's refusals."""
import functools
import uuid

import numpy as np
import pytest

from worldql_server_amd import abi, ingest
from worldql_server_amd.subscriptions import PeerIds

OK, POS, ATG, WK, SK = (abi.INGEST_OK, abi.INGEST_HAS_POSITION, abi.INGEST_WORLD_GLOBAL, abi.INGEST_WORLD_KNOWN,
                        abi.INGEST_SENDER_KNOWN)
NO_PEER, W_GLOBAL, W_INVALID = abi.INGEST_NO_PEER, abi.WORLD_GLOBAL, abi.WORLD_INVALID
HB, SUB, UNSUB, GLOBAL, LOCAL = 0, 4, 5, 6, 7
ONES = (1 << 128) - 1
HI = 1 << 64                      # one step of the key's high half
FIELDS = ("sender", "flags", "j_uuid", "j_id", "j_frame")


def U(k: int) -> bytes:
    return uuid.UUID(int=k).bytes


def frames(rows, table):
    """The decode's arrays from (instruction, uuid int, kind) rows under a sender table {uuid bytes: id}. kind:
    "ok" a position and a resolved world; "noworld" / "atglobal" / "nopos" lack one thing; "bad" did not
    decode (but carries the uuid's bytes, which the decoder would have zeroed: the call must not look)."""
    n = len(rows)
    d = dict(instruction=np.zeros(n, np.uint8), flags=np.zeros(n, np.uint8), world=np.full(n, W_INVALID, np.uint32),
             sender=np.full(n, NO_PEER, np.uint32), repl=np.zeros(n, np.uint8), pos=np.zeros((n, 3), np.float64),
             sender_uuid=np.zeros((n, 16), np.uint8))
    for i, (ins, k, kind) in enumerate(rows):
        u = U(k)
        d["sender_uuid"][i] = np.frombuffer(u, np.uint8)
        d["repl"][i], d["pos"][i] = i % 3, (i + 0.25, -1.0 * i, 3.0)
        if kind == "bad":
            continue
        d["instruction"][i] = ins
        f = OK | (0 if kind == "nopos" else POS)
        if kind == "atglobal":
            f, d["world"][i] = f | ATG, W_GLOBAL
        elif kind != "noworld":
            f, d["world"][i] = f | WK, i % 5
        if u in table:
            f, d["sender"][i] = f | SK, table[u]
        d["flags"][i] = f
    return d


def case(rows, table=None, free=(), id_next=None, id_limit=None, capacity=None, joined_capacity="n"):
    """table: {uuid int: id}. id_next defaults to one above the table's and the free list's ids, id_limit to
    room for every frame, capacity to the table and every frame."""
    table = {U(k): v for k, v in (table or {}).items()}
    d = frames(rows, table)
    top = max(list(table.values()) + list(free) + [-1]) + 1
    id_next = top if id_next is None else id_next
    keys = sorted(table)
    return dict(d=d, table_uuids=np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 16).copy() if keys else np.zeros((0, 16), np.uint8),
                table_ids=np.array([table[k] for k in keys], np.uint32), free=np.array(free, np.uint32), id_next=id_next,
                id_limit=id_next + len(rows) if id_limit is None else id_limit,
                capacity=len(table) + len(rows) if capacity is None else capacity,
                joined_capacity=len(rows) if joined_capacity == "n" else joined_capacity)


def random_rows(n, seed, n_known=40, n_new=12, p_sub=0.3):
    """n frames of every kind from known senders (uuids 1000 ..) and new ones (uuids spread over both key
    halves), in random order: the joins' frame order is not their key order."""
    rng = np.random.default_rng(seed)
    new = [int(v) for v in rng.integers(1, 1 << 62, n_new)] if n_new else []
    new = [v * HI + int(rng.integers(0, 3)) if j % 2 else v for j, v in enumerate(new)]
    rows = []
    for _ in range(n):
        k = new[int(rng.integers(len(new)))] if new and rng.random() < 0.35 else 1000 + int(rng.integers(n_known))
        ins = SUB if rng.random() < p_sub else int(rng.choice([HB, UNSUB, GLOBAL, LOCAL, 9, 2]))
        kind = rng.choice(["ok", "noworld", "atglobal", "nopos", "bad"], p=[0.8, 0.06, 0.05, 0.05, 0.04])
        rows.append((ins, k, str(kind)))
    return rows


KNOWN = {1000 + k: 3 * k + 1 for k in range(40)}    # ids that are not the index


@functools.lru_cache(maxsize=None)
def cases():
    """name -> the arguments of join_peers_np (a dict: d, table_uuids, table_ids, free, id_next, id_limit,
    capacity, joined_capacity)."""
    c = {}
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025, 2100):
        c[f"mix_{n}"] = case(random_rows(n, seed=n), KNOWN, free=(200, 7, 150))
    c["no_candidate"] = case([(LOCAL, 1000 + i % 40, "ok") for i in range(130)] + [(UNSUB, 5, "ok"), (HB, 5, "ok")], KNOWN)
    c["one_uuid_every_frame"] = case([(SUB, 77, "ok")] * 2100, KNOWN)
    rng = np.random.default_rng(1)
    distinct = [int(v) for v in rng.permutation(2100)]
    c["distinct_every_frame"] = case([(SUB, 5000 + v * (HI if v % 3 == 0 else 1), "ok") for v in distinct], KNOWN, free=(500, 501))
    c["low_half_only"] = case([(SUB, 9 * HI + int(v), "ok") for v in rng.permutation(70)], {9 * HI + 35: 0, 9 * HI + 200: 1})
    c["high_half_only"] = case([(SUB, int(v) * HI + 9, "ok") for v in rng.permutation(70)], {35 * HI + 9: 0, 200 * HI + 9: 1})
    # the all-ones key is the padding's: real candidates must come out before the pads, and the pads join nobody
    c["zero_and_ones_join"] = case([(LOCAL, 1001, "ok"), (SUB, ONES, "ok"), (HB, 0, "ok"), (SUB, 0, "ok"), (LOCAL, ONES, "ok"),
                                    (SUB, ONES, "ok"), (LOCAL, 0, "ok")] + [(HB, 1002, "ok")] * 70, KNOWN)
    c["zero_and_ones_in_table"] = case([(SUB, 1, "ok"), (LOCAL, 0, "ok"), (SUB, ONES - 1, "ok"), (SUB, ONES, "ok"), (SUB, 0, "ok")],
                                       {0: 4, ONES: 5, 50: 6})
    # the joiner's frames around its first subscribe: before it they keep the no-peer id
    around = [(LOCAL, 8, "ok"), (UNSUB, 8, "ok"), (HB, 8, "ok"), (SUB, 8, "ok"), (LOCAL, 8, "ok"), (UNSUB, 8, "ok"), (HB, 8, "ok"),
              (SUB, 8, "ok"), (GLOBAL, 8, "ok")]
    c["around_first_subscribe"] = case(around, KNOWN)
    c["around_first_subscribe_across_granules"] = case(around[:3] + [(LOCAL, 1003, "ok")] * 61 + around[3:] +
                                                       [(HB, 8, "ok")] * 1000 + [(SUB, 9, "ok"), (LOCAL, 8, "ok")], KNOWN)
    # frames that must not join: an unresolved world, "@global", no position, and a frame that did not decode
    c["must_not_join"] = case([(SUB, 20, "noworld"), (SUB, 21, "atglobal"), (SUB, 22, "nopos"), (SUB, 23, "bad"), (LOCAL, 20, "ok"),
                               (SUB, 24, "ok"), (SUB, 24, "bad"), (LOCAL, 24, "bad"), (SUB, 24, "noworld"), (SUB, 20, "noworld"),
                               (UNSUB, 24, "nopos")], KNOWN)
    joiners = [(SUB, 300 + k, "ok") for k in (5, 3, 9, 1, 7)] + [(LOCAL, 303, "ok"), (SUB, 305, "ok")]
    c["n_free_0"] = case(joiners, KNOWN)
    c["n_free_larger"] = case(joiners, KNOWN, free=(90, 2, 77, 3, 91, 92, 93))
    c["free_then_next"] = case(joiners, KNOWN, free=(90, 2))
    c["id_limit_reached"] = case(joiners, KNOWN, free=(90, 2), id_next=400, id_limit=403)
    c["one_join_too_many"] = case(joiners, KNOWN, free=(90, 2), id_next=400, id_limit=402)
    c["no_ids_at_all"] = case(joiners, KNOWN, id_next=400, id_limit=400)
    c["table_empty"] = case(joiners + [(LOCAL, 1000, "ok")], {})
    mid = {100 * HI + k: k for k in range(50)}
    c["new_keys_below"] = case([(SUB, 7 + k, "ok") for k in (4, 2, 3)], mid)
    c["new_keys_above"] = case([(SUB, 200 * HI + k, "ok") for k in (4, 2, 3)], mid)
    c["new_keys_interleaved"] = case([(SUB, 100 * HI + 2 * k + 1 if k % 2 else 100 * HI - k, "ok") for k in range(40)],
                                     {100 * HI + 2 * k: k for k in range(50)})
    c["table_at_capacity"] = case(joiners, KNOWN, capacity=45)
    c["table_one_over"] = case(joiners, KNOWN, capacity=44)
    big = {3 * k + 1: k for k in range(4090)}
    c["table_4096"] = case([(SUB, 3 * int(v), "ok") for v in rng.permutation(4096)[:6]] + [(LOCAL, 4, "ok")], big, capacity=4096)
    c["joined_capacity_exact"] = case(joiners, KNOWN, joined_capacity=5)
    c["joined_capacity_short"] = case(joiners, KNOWN, joined_capacity=4)
    c["every_overflow"] = case(joiners, KNOWN, id_next=400, id_limit=401, capacity=41, joined_capacity=0)
    c["no_j_arrays"] = case(joiners, KNOWN, joined_capacity=None)
    c["no_reserve"] = dict(case(joiners, KNOWN), capacity=None)
    # flags and values drawn independently: most frames disagree; nothing may fault and the definition decides
    hostile = case(random_rows(700, seed=5), KNOWN)
    hostile["d"]["flags"] = rng.integers(0, 256, 700).astype(np.uint8)
    hostile["d"]["world"] = rng.choice(np.array([0, 1, 4, W_GLOBAL, W_INVALID, 0xFFFFFFFD], np.uint32), size=700)
    hostile["d"]["sender"] = rng.choice(np.array([0, 1, 49, NO_PEER, 0xFFFFFFFE], np.uint32), size=700)
    c["hostile_700"] = hostile
    return c


OVERFLOWS = {"one_join_too_many": 1, "no_ids_at_all": 1, "table_one_over": 2, "joined_capacity_short": 4, "every_overflow": 7}


def drop_cases():
    """name -> (table {uuid int: id}, capacity, the ids to drop)."""
    t100 = {7 * k + 1: (k * 37) % 100 for k in range(100)}
    return {
        "empty_list": (t100, 128, []),
        "every_id": (t100, 128, list(range(100))),
        "absent_ids": (t100, 128, [100, 101, 5000, 3]),
        "duplicates": (t100, 100, [5, 5, 9, 5, 9, 64, 64]),
        "above_id_limit": (t100, 128, [0xFFFFFFFF, 0xFFFFFFFE, 1 << 31, 99]),
        "empty_table": ({}, 16, [1, 2, 3]),
        "capacity_0": ({}, 0, [1]),
        "granule_edges": ({k + 1: k for k in range(130)}, 130, [0, 63, 64, 65, 127, 128, 129]),
        "table_4096": ({3 * k + 1: k for k in range(4096)}, 4096, list(range(0, 4096, 3)) + [4095]),
    }


def drop_args(name):
    table, cap, ids = drop_cases()[name]
    keys = sorted(U(k) for k in table)
    by = {U(k): v for k, v in table.items()}
    tu = np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 16).copy() if keys else np.zeros((0, 16), np.uint8)
    return tu, np.array([by[k] for k in keys], np.uint32), cap, np.array(ids, np.uint32)


@functools.lru_cache(maxsize=None)
def definition(name):
    a = cases()[name]
    return ingest.join_peers_np(a["d"], a["table_uuids"], a["table_ids"], a["free"], a["id_next"], a["id_limit"], a["capacity"],
                                a["joined_capacity"])


def same(got, want, what="", fields=FIELDS, counters=True, table=True):
    for k in fields:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            at = int(np.flatnonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(axis=1))[0])
            raise AssertionError((what, k, "row", at, g[at], w[at]))
    if counters:
        assert got["counters"] == want["counters"], (what, got["counters"], want["counters"])
    if table:
        assert got["table"][0].tobytes() == want["table"][0].tobytes(), (what, "table uuids")
        assert got["table"][1].tolist() == want["table"][1].tolist(), (what, "table ids")


# ---- the restatement ---------------------------------------------------------------------------------------

def sequential(a):
    """The frames one at a time: a subscribe that passes area_subscribe.rs's checks (not "@global", a world
    the table holds, a position) asks for the sender's id; everything else only looks it up."""
    d = a["d"]
    ids = {u.tobytes(): int(i) for u, i in zip(a["table_uuids"], a["table_ids"])}
    free, nxt = [int(v) for v in a["free"]], int(a["id_next"])   # the allocator: the free list first, then upwards
    sender, flags = d["sender"].copy(), d["flags"].copy()
    joins = []
    for i in range(len(sender)):
        f = int(d["flags"][i])
        if not f & OK:
            continue
        u = d["sender_uuid"][i].tobytes()
        if d["instruction"][i] == SUB and f & POS and not f & ATG and f & WK and u not in ids:
            if free:
                ids[u] = free.pop(0)
            else:
                ids[u], nxt = nxt, nxt + 1
            joins.append((u, ids[u], i))
        if u in ids:
            sender[i], flags[i] = ids[u], f | SK
    return sender, flags, joins, ids


CONSISTENT = [k for k in cases() if k not in OVERFLOWS and k not in ("hostile_700", "no_reserve")]


@pytest.mark.parametrize("name", CONSISTENT)
def test_case_equals_the_sequential_restatement(name):
    a, got = cases()[name], definition(name)
    sender, flags, joins, ids = sequential(a)
    assert got["sender"].tolist() == sender.tolist() and got["flags"].tolist() == flags.tolist()
    assert [bytes(u) for u in got["j_uuid"]] == [j[0] for j in joins]
    assert got["j_id"].tolist() == [j[1] for j in joins] and got["j_frame"].tolist() == [j[2] for j in joins]
    tu, ti = got["table"]
    assert {u.tobytes(): int(i) for u, i in zip(tu, ti)} == ids
    assert [u.tobytes() for u in tu] == sorted(ids)
    c = got["counters"]
    assert c["overflow"] == 0 and c["error"] == 0 and c["n_joined"] == len(joins) and c["n_table"] == len(ids)
    assert c["n_free_used"] == min(len(joins), len(a["free"]))
    assert c["id_next"] == a["id_next"] + len(joins) - c["n_free_used"]
    assert c["first_join"] == (joins[0][2] if joins else len(sender))
    assert c["n_patched"] == int((got["flags"] != a["d"]["flags"]).sum())
    # what the join leaves, the dispatch defers only for its world
    disp = ingest.dispatch_np(dict(a["d"], sender=got["sender"], flags=got["flags"]))
    left = disp["side_src"][disp["counters"]["side_begin"][4]:]
    assert all(not a["d"]["flags"][i] & WK for i in left)


def test_what_the_named_cases_hold():
    d = definition
    assert d("no_candidate")["counters"]["n_candidates"] == 0 and d("no_candidate")["counters"]["n_patched"] == 0
    assert d("one_uuid_every_frame")["counters"] == dict(n_frames=2100, n_candidates=2100, n_joined=1, n_patched=2100,
                                                          n_free_used=0, id_next=120, n_table=41, first_join=0, overflow=0, error=0)
    assert d("distinct_every_frame")["counters"]["n_joined"] == 2100
    assert d("zero_and_ones_join")["j_frame"].tolist() == [1, 3] and d("zero_and_ones_join")["counters"]["n_patched"] == 5
    assert d("zero_and_ones_in_table")["counters"]["n_joined"] == 2
    a = d("around_first_subscribe")
    assert a["sender"].tolist() == [NO_PEER] * 3 + [119] * 6 and a["counters"]["n_candidates"] == 2
    m = d("must_not_join")
    assert m["j_frame"].tolist() == [5] and m["counters"]["n_patched"] == 3   # frames 5, 8 and 10: decoded, after the join
    assert m["sender"][[0, 4, 6, 7, 9]].tolist() == [NO_PEER] * 5
    assert d("n_free_larger")["j_id"].tolist() == [90, 2, 77, 3, 91]
    assert d("free_then_next")["j_id"].tolist() == [90, 2, 119, 120, 121] and d("free_then_next")["counters"]["id_next"] == 122
    assert d("id_limit_reached")["j_id"].tolist() == [90, 2, 400, 401, 402]
    assert d("table_at_capacity")["counters"]["n_table"] == 45
    assert d("hostile_700")["counters"]["error"] == abi.JOIN_ERROR_DISAGREE
    n = d("no_reserve")
    assert n["counters"] == dict(n_frames=7, n_candidates=0, n_joined=0, n_patched=0, n_free_used=0, id_next=119, n_table=0,
                                 first_join=7, overflow=0, error=abi.JOIN_ERROR_NO_TABLE)


@pytest.mark.parametrize("name", sorted(OVERFLOWS))
def test_an_overflow_changes_nothing(name):
    a, got = cases()[name], definition(name)
    c = got["counters"]
    assert c["overflow"] == OVERFLOWS[name] and c["n_joined"] == 5 and c["n_candidates"] == 6
    assert (c["n_patched"], c["n_free_used"], c["id_next"], c["n_table"], c["first_join"]) == (0, 0, a["id_next"], 40, 7)
    assert got["sender"].tobytes() == a["d"]["sender"].tobytes() and got["flags"].tobytes() == a["d"]["flags"].tobytes()
    assert len(got["j_id"]) == len(got["j_frame"]) == len(got["j_uuid"]) == 0
    assert got["table"][0].tobytes() == a["table_uuids"].tobytes() and got["table"][1].tolist() == a["table_ids"].tolist()


# ---- the property: a real PeerIds, frame by frame ------------------------------------------------------------------

def test_random_ticks_through_peer_ids():
    """300 random small ticks on one growing population. A sequential PeerIds takes every frame in arrival
    order as _apply_run / _sender_id do; the host's PeerIds only adopts what the join assigned. Between
    ticks some peers leave (release on both, drop_peers_np on the table)."""
    rng = np.random.default_rng(12)
    seq, host = PeerIds(), PeerIds()
    table: dict = {}
    total_joined = total_free_used = 0
    for t in range(300):
        n = int(rng.integers(0, 60))
        pool = [int(v) for v in rng.integers(1, 400, 12)]
        rows = [(SUB if rng.random() < 0.3 else int(rng.choice([HB, UNSUB, GLOBAL, LOCAL])), pool[int(rng.integers(12))],
                 str(rng.choice(["ok", "atglobal", "nopos", "bad"], p=[0.85, 0.05, 0.05, 0.05]))) for _ in range(n)]
        d = frames(rows, table)
        tu, ti = ingest._table_arrays(table)
        free = host.free_in_pop_order()
        got = ingest.join_peers_np(d, tu, ti, free, host.high_water, host.high_water + n, len(table) + n, n)
        want_sender = []
        for ins, k, kind in rows:                      # the sequential loop
            if kind == "bad":
                want_sender.append(NO_PEER)
                continue
            if ins == SUB and kind == "ok":
                seq.id(U(k))
            pid = seq.lookup(U(k))
            want_sender.append(NO_PEER if pid is None else pid)
        assert got["sender"].tolist() == want_sender, t
        c = got["counters"]
        assert c["overflow"] == 0 and c["error"] == 0
        host.adopt([bytes(u) for u in got["j_uuid"]], got["j_id"])
        assert host._ids == seq._ids and host._peers == seq._peers and host._free == seq._free, t
        assert c["id_next"] == host.high_water and c["n_free_used"] == len(free) - len(host._free)
        disp = ingest.dispatch_np(dict(d, sender=got["sender"], flags=got["flags"]))
        assert disp["counters"]["n_deferred"] == 0, t       # every world resolves: nothing is left for the host
        table = {u.tobytes(): int(i) for u, i in zip(*got["table"])}
        assert table == seq._ids
        total_joined += c["n_joined"]
        total_free_used += c["n_free_used"]
        if table and rng.random() < 0.5:                    # some peers leave between the ticks
            leave = [u for u in sorted(table) if rng.random() < 0.2]
            gone = [table[u] for u in leave]
            left = ingest.drop_peers_np(*ingest._table_arrays(table), gone + gone[:1] + [100000])
            assert left["counters"]["n_patched"] == len(leave) and left["counters"]["n_table"] == len(table) - len(leave)
            for u in leave:
                assert seq.release(u) == host.release(u) == table[u]
            table = {u.tobytes(): int(i) for u, i in zip(*left["table"])}
    assert total_joined > 300 and total_free_used > 100


# ---- the leave side, and adopt ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(drop_cases()))
def test_drop_cases(name):
    table, cap, ids = drop_cases()[name]
    tu, ti, _, drop = drop_args(name)
    got = ingest.drop_peers_np(tu, ti, drop)
    kept = {U(k): v for k, v in table.items() if v not in set(ids)}
    assert [u.tobytes() for u in got["table"][0]] == sorted(kept) and got["table"][1].tolist() == [kept[u] for u in sorted(kept)]
    assert got["counters"] == dict(n_frames=len(ids), n_candidates=0, n_joined=0, n_patched=len(table) - len(kept), n_free_used=0,
                                   id_next=0, n_table=len(kept), first_join=len(ids), overflow=0, error=0)
    none = ingest.drop_peers_np(tu, ti, drop, reserved=False)
    assert none["counters"]["error"] == abi.JOIN_ERROR_NO_TABLE and none["table"][1].tolist() == ti.tolist()


def test_adopt_refuses_what_id_would_not_hand_out():
    p = PeerIds()
    for k in range(5):
        p.id(f"p{k}")
    p.release("p1"), p.release("p3")
    assert p.free_in_pop_order() == [3, 1]
    before = (dict(p._ids), list(p._peers), list(p._free))
    for peers, ids in ((["a", "b"], [1, 3]), (["a"], [5]), (["a", "b", "c"], [3, 1, 6]), (["a", "a"], [3, 1]), (["p0"], [3]),
                       (["a"], [3, 1])):
        with pytest.raises(ValueError):
            p.adopt(peers, ids)
        assert (p._ids, p._peers, p._free) == before
    p.adopt(["a", "b", "c"], np.array([3, 1, 5], np.uint32))
    q = PeerIds()
    for k in range(5):
        q.id(f"p{k}")
    q.release("p1"), q.release("p3")
    for name in "abc":
        q.id(name)
    assert (p._ids, p._peers, p._free) == (q._ids, q._peers, q._free) and p.high_water == 6
    p.adopt([], [])
