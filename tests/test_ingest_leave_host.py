"""CPU: the ingest leaves' definition (worldql_server_amd/ingest.py leave_peers_np) and the shared case list of
the mirror (tests/test_ingest_leave_cpp_mirror.py) and GPU (tests/test_gpu_ingest_leave.py) tests.

  - every named case against a straight restatement: a dict-backed PeerMap and a real PeerIds, one peer at a
    time: is_stale as transport/peer.rs:59-69 states it, the stale set collected and then removed as
    transport/zeromq/outgoing.rs:132-150 does, every removal broadcasting its uuid's text and releasing its id;
  - the overflow cases change nothing and say what was needed; a handle without a reserve;
  - l_param is str(uuid.UUID(bytes=...)) for every leaver;
  - 200 random sweeps of a joining, heart-beating and leaving population through a real PeerIds: after each,
    PeerIds.release_ids leaves the free list equal to free_out, and a recycled id never carries its previous
    owner's stamp;
  - the lifecycle the GPU test runs, on the CPU: its seed and probabilities make enough peers leave stale and
    listed, enough ids come back and enough peers join for that test to mean something;
  - PeerIds.release_ids' refusals."""
import functools
import uuid

import numpy as np
import pytest

from worldql_server_amd import abi, ingest
from worldql_server_amd.subscriptions import PeerIds

NEVER = abi.SEEN_NEVER
NOW, MAX_AGE = 1000, 10
FIELDS = ("l_uuid", "l_id", "l_reason", "l_param", "l_param_offsets", "gone_bits", "free_out", "last_seen")
ROW_FIELDS = ("l_uuid", "l_id", "l_reason", "l_param", "l_param_offsets")
BLOCK = 256                       # the flag pass's block


def case(n_live, n_all=None, n_ids=None, stale=(), listed=(), pinned=(), never=(), future=(), stamps=None, extra_listed=(),
         capacity=None, leave_capacity="n", free_capacity="fit", max_age=MAX_AGE, now=NOW, seed=0, reserved=True):
    """A table of n_live entries (random uuids; ids a random draw from range(n_all), every other id of that
    range on the free list, shuffled) and one stamp per id < n_ids (default n_all). stale / listed / pinned /
    never / future: table positions (uuid order) whose stamp is too old / whose id is listed / pinned / whose
    stamp is NEVER / ahead of `now`; stamps: {position: stamp}. Everybody else was seen within max_age.
    extra_listed: ids appended to the listed ones as they are. capacity: the reserved room (default n_live +
    3); leave_capacity "n": room for everybody, None: no l_* arrays; free_capacity "fit": exactly sufficient
    for everybody, None: no free_out."""
    rng = np.random.default_rng(1000 + seed + n_live)
    n_all = n_live + 5 if n_all is None else n_all
    n_ids = n_all if n_ids is None else n_ids
    keys = sorted(uuid.UUID(int=int(h) << 64 | int(l)).bytes
                  for h, l in zip(rng.integers(0, 1 << 63, n_live), rng.integers(0, 1 << 63, n_live)))
    draw = rng.permutation(n_all)
    ids, free = draw[:n_live].astype(np.uint32), draw[n_live:].astype(np.uint32)
    seen = np.full(n_ids, NEVER, np.uint32)           # ids nobody holds were never seen
    for e, i in enumerate(ids):
        if i < n_ids:
            seen[i] = now - min(e % (max_age + 1), now)
    put = {e: max(now - max_age - 1 - e % 3, 0) for e in stale}
    put.update({e: NEVER for e in never})
    put.update({e: now + 1 + e % 7 for e in future})
    put.update(stamps or {})
    for e, s in put.items():
        if ids[e] < n_ids:
            seen[ids[e]] = s
    leave_ids = [int(ids[e]) for e in listed] + [int(v) for v in extra_listed]
    return dict(table_uuids=np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 16).copy() if keys else np.zeros((0, 16), np.uint8),
                table_ids=ids, last_seen=seen, now=now, max_age=max_age,
                pinned=ingest.id_bits([ids[e] for e in pinned if ids[e] < n_ids], n_ids) if pinned else None,
                leave_ids=np.array(leave_ids, np.uint32), free=free,
                leave_capacity=n_live if leave_capacity == "n" else leave_capacity,
                free_capacity=len(free) + n_live if free_capacity == "fit" else free_capacity,
                capacity=n_live + 3 if capacity is None else capacity, reserved=reserved)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> the arguments of leave_peers_np (a dict) plus `capacity`, the table's reserved room."""
    c = {}
    for n in (0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 1024, 1025):
        rng = np.random.default_rng(n)
        pick = lambda p: [e for e in range(n) if rng.random() < p]
        c[f"mix_{n}"] = case(n, stale=pick(0.2), listed=pick(0.15), pinned=pick(0.2), never=pick(0.1), future=pick(0.05),
                             extra_listed=(n + 4, n + 100, 0xFFFFFFFE))
    c["table_full_to_its_reserve"] = case(130, stale=range(0, 130, 7), listed=(1, 128), capacity=130)
    c["nobody_leaves"] = case(200)
    c["everybody_stale"] = case(200, stale=range(200))
    c["everybody_listed"] = case(200, listed=range(200))
    c["only_the_first"] = case(200, stale=(0,))
    c["only_the_last"] = case(200, listed=(199,))
    c["positions_63_and_64"] = case(200, stale=(63,), listed=(64,))
    c["n_ids_not_a_multiple_of_32"] = case(70, n_all=77, stale=(3, 69), listed=(5,), pinned=(3, 9))
    c["n_ids_one_word_and_one_bit"] = case(20, n_all=33, stale=(3,), listed=(5,))
    # the per-id arrays end below some of the table's ids: those entries are not judged (error bit 2)
    c["table_id_above_n_ids"] = case(90, n_all=100, n_ids=61, stale=range(0, 90, 4), listed=range(1, 90, 5), never=range(2, 90, 9))
    c["listed_duplicated"] = case(100, listed=(4, 4, 9, 4, 9, 70, 70))
    unknown = case(100, n_all=120, listed=(7,), extra_listed=(5000,))                       # an id nobody has, and free ids
    c["listed_unknown"] = dict(unknown, leave_ids=np.concatenate([unknown["leave_ids"], unknown["free"][:3]]))
    c["listed_above_n_ids"] = case(100, listed=(7,), extra_listed=(105, 106, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF))
    c["stamp_never"] = case(100, never=(0, 5, 63, 64, 99), stale=(6,))
    c["stamp_never_and_listed"] = case(100, never=(5, 6), listed=(5,))
    c["stamp_in_the_future"] = case(100, future=range(0, 100, 3), stamps={1: NEVER - 1, 2: NOW + 1})
    c["age_equals_max_age_stays"] = case(100, stamps={e: NOW - MAX_AGE for e in (0, 50, 99)})
    c["age_one_above_max_age_leaves"] = case(100, stamps={e: NOW - MAX_AGE - 1 for e in (0, 50, 99)})
    c["max_age_0"] = case(100, max_age=0, stamps={3: NOW - 1, 4: NOW, 5: NOW + 1, 6: 0})
    c["now_0"] = case(50, now=0, max_age=0, never=(3,))
    c["stamp_0_and_a_late_now"] = case(50, now=0xFFFFFFFE, max_age=5, stamps={3: 0, 4: 0xFFFFFFFE - 5, 5: 0xFFFFFFFE - 6})
    c["pinned_stale_stays"] = case(100, stale=(3, 40, 41), pinned=(3, 41, 50))
    c["pinned_listed_leaves"] = case(100, stale=(3,), listed=(3, 8), pinned=(3, 8))
    c["listed_and_stale"] = case(100, stale=(3, 70), listed=(3, 70, 71))
    c["leave_capacity_exact"] = case(100, stale=range(10), leave_capacity=10)
    c["leave_capacity_short"] = case(100, stale=range(10), never=(50,), leave_capacity=9)
    c["free_capacity_exact"] = case(100, stale=range(10), free_capacity=15)
    c["free_capacity_short"] = case(100, stale=range(10), never=(50,), free_capacity=14)
    c["both_overflows"] = case(100, stale=range(10), listed=(20,), leave_capacity=0, free_capacity=5)
    c["no_l_arrays"] = case(100, stale=range(10), leave_capacity=None)
    c["no_free_out"] = case(100, stale=range(10), free_capacity=None)
    c["no_reserve"] = case(100, stale=range(10), listed=(20,), never=(50,), reserved=False)
    return c


OVERFLOWS = {"leave_capacity_short": 1, "free_capacity_short": 2, "both_overflows": 3}
ARGS = ("table_uuids", "table_ids", "last_seen", "now", "max_age", "pinned", "leave_ids", "free", "leave_capacity", "free_capacity")


def define(a):
    return ingest.leave_peers_np(*[a[k] for k in ARGS], reserved=a["reserved"])


@functools.lru_cache(maxsize=None)
def definition(name):
    return define(cases()[name])


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

class Peer:
    """transport/peer.rs: a ZeroMQ peer carries its last heartbeat, a WebSocket peer (pinned here) none."""

    def __init__(self, uid, pid, last_heartbeat, zmq):
        self.uuid, self.id, self.last_heartbeat, self.zmq = uid, pid, last_heartbeat, zmq

    def is_stale(self, now, max_duration):
        if not self.zmq or self.last_heartbeat is None:       # not seen yet: the clock starts at the sweep
            return False
        return now > self.last_heartbeat and now - self.last_heartbeat > max_duration


def host_ids(a):
    """A real PeerIds in the case's state: the table's peers hold their ids, every other id is free."""
    ids, free = [int(i) for i in a["table_ids"]], [int(i) for i in a["free"]]
    peers = [None] * (max(ids + free + [-1]) + 1)
    for u, i in zip(a["table_uuids"], ids):
        peers[i] = u.tobytes()
    return PeerIds.restore(dict(peers=peers, free=free[::-1]))


def sequential(a):
    """One peer at a time over a dict-backed PeerMap: collect who leaves (the transport's disconnects, then the
    stale sweep), then remove each in uuid order: broadcast its text, release its id, forget its stamp."""
    n_ids = len(a["last_seen"])
    pin = a["pinned"]
    pinned = set() if pin is None else {i for i in range(n_ids) if (int(pin[i >> 5]) >> (i & 31)) & 1}
    stamps = {i: int(s) for i, s in enumerate(a["last_seen"])}
    peer_map = {}
    for u, i in zip(a["table_uuids"], a["table_ids"]):
        i = int(i)
        known = i < n_ids
        peer_map[u.tobytes()] = Peer(u.tobytes(), i, stamps[i] if known and stamps[i] != NEVER else None, known and i not in pinned)
    ids = host_ids(a)
    disconnects = {int(i) for i in a["leave_ids"] if int(i) < n_ids}
    reasons = {}
    for u, p in peer_map.items():
        if p.id >= n_ids:
            continue
        r = (abi.LEAVE_LISTED if p.id in disconnects else 0) | (abi.LEAVE_STALE if p.is_stale(a["now"], a["max_age"]) else 0)
        if r:
            reasons[u] = r
    broadcasts, released, started = [], [], 0
    for u in sorted(reasons):
        p = peer_map.pop(u)
        broadcasts.append(str(uuid.UUID(bytes=u)))            # peer_map.rs:121-141: parameter = uuid.to_string()
        released.append(ids.release(u))
        stamps[p.id] = NEVER
    for p in peer_map.values():
        if p.id < n_ids and p.last_heartbeat is None and stamps[p.id] == NEVER:
            stamps[p.id], started = a["now"], started + 1
    return dict(reasons=[reasons[u] for u in sorted(reasons)], uuids=sorted(reasons), text=broadcasts, released=released,
                free=ids.free_in_pop_order(), table={u: p.id for u, p in peer_map.items()},
                stamps=[stamps[i] for i in range(n_ids)], started=started)


CONSISTENT = [k for k in cases() if k not in OVERFLOWS and k != "no_reserve"]


@pytest.mark.parametrize("name", CONSISTENT)
def test_case_equals_the_sequential_restatement(name):
    a, got, s = cases()[name], definition(name), sequential(cases()[name])
    assert [bytes(u) for u in got["l_uuid"]] == s["uuids"] and got["l_id"].tolist() == s["released"]
    assert got["l_reason"].tolist() == s["reasons"]
    assert got["l_param"].tobytes().decode() == "".join(s["text"])
    assert got["l_param_offsets"].tolist() == [36 * k for k in range(len(s["uuids"]) + 1)]
    assert got["free_out"].tolist() == s["free"]
    assert got["last_seen"].tolist() == s["stamps"]
    tu, ti = got["table"]
    assert {u.tobytes(): int(i) for u, i in zip(tu, ti)} == s["table"] and [u.tobytes() for u in tu] == sorted(s["table"])
    assert got["gone_bits"].tolist() == ingest.id_bits(s["released"], len(a["last_seen"])).tolist()
    c = got["counters"]
    assert c["overflow"] == 0 and c["n_left"] == len(s["uuids"]) and c["n_stamped"] == s["started"]
    assert c["n_table_before"] == len(a["table_ids"]) and c["n_table"] == len(s["table"]) and c["n_free"] == len(s["free"])
    assert c["n_listed"] == len(a["leave_ids"])
    assert c["n_listed_found"] == sum(bool(r & 1) for r in s["reasons"]) and c["n_stale"] == sum(bool(r & 2) for r in s["reasons"])
    assert c["error"] == (abi.LEAVE_ERROR_ID_RANGE if any(int(i) >= len(a["last_seen"]) for i in a["table_ids"]) else 0)


def test_the_cases_cover_what_they_name():
    d = {k: definition(k) for k in cases()}
    assert d["nobody_leaves"]["counters"]["n_left"] == 0 and d["nobody_leaves"]["counters"]["n_stamped"] == 0
    assert d["everybody_stale"]["counters"]["n_table"] == 0 and d["everybody_listed"]["l_reason"].tolist() == [1] * 200
    assert d["table_id_above_n_ids"]["counters"]["error"] == abi.LEAVE_ERROR_ID_RANGE
    assert d["stamp_never"]["counters"]["n_stamped"] == 5 and d["stamp_never"]["counters"]["n_left"] == 1
    assert d["stamp_never_and_listed"]["counters"]["n_stamped"] == 1
    assert d["stamp_in_the_future"]["counters"]["n_left"] == 0
    assert d["age_equals_max_age_stays"]["counters"]["n_left"] == 0 and d["age_one_above_max_age_leaves"]["counters"]["n_left"] == 3
    assert d["max_age_0"]["counters"]["n_left"] == 2 and d["now_0"]["counters"]["n_left"] == 0
    assert d["stamp_0_and_a_late_now"]["counters"]["n_left"] == 2
    assert d["pinned_stale_stays"]["l_reason"].tolist() == [2] and d["pinned_listed_leaves"]["l_reason"].tolist() == [1, 1]
    assert d["listed_and_stale"]["l_reason"].tolist() == [3, 3, 1]
    assert d["listed_duplicated"]["counters"]["n_listed_found"] == 3 and d["listed_unknown"]["counters"]["n_left"] == 1
    assert d["listed_above_n_ids"]["counters"]["n_left"] == 1
    assert d["leave_capacity_exact"]["counters"]["overflow"] == 0 and d["free_capacity_exact"]["counters"]["overflow"] == 0
    assert d["no_l_arrays"]["counters"]["n_left"] == 10 and d["no_free_out"]["counters"]["n_left"] == 10
    assert d["positions_63_and_64"]["counters"]["n_left"] == 2
    for n in (65, BLOCK + 1, 1025):
        c = d[f"mix_{n}"]["counters"]
        assert c["n_left"] > 0 and c["n_stamped"] > 0 and c["n_listed_found"] > 0 and c["n_stale"] > 0 and c["error"] == 0


@pytest.mark.parametrize("name", sorted(OVERFLOWS))
def test_an_overflow_changes_nothing_and_says_what_was_needed(name):
    a, got = cases()[name], definition(name)
    c = got["counters"]
    assert c["overflow"] == OVERFLOWS[name] and c["n_left"] == (11 if name == "both_overflows" else 10) and c["n_stamped"] == 0
    assert c["n_table"] == c["n_table_before"] == 100 and c["n_free"] == len(a["free"])
    assert got["last_seen"].tolist() == a["last_seen"].tolist() and not got["gone_bits"].any()
    assert got["table"][0].tobytes() == a["table_uuids"].tobytes() and got["table"][1].tolist() == a["table_ids"].tolist()
    assert all(len(got[k]) == 0 for k in ROW_FIELDS + ("free_out",))
    # with the room it asked for the same sweep goes through
    roomy = define(dict(a, leave_capacity=c["n_left"], free_capacity=len(a["free"]) + c["n_left"]))
    assert roomy["counters"]["overflow"] == 0 and roomy["counters"]["n_left"] == c["n_left"]


def test_no_reserve_is_a_no_op():
    a, got = cases()["no_reserve"], definition("no_reserve")
    want = {k: 0 for k in abi.LEAVE_COUNTERS_DTYPE.names}
    want.update(n_listed=1, n_free=len(a["free"]), error=abi.LEAVE_ERROR_NO_TABLE)
    assert got["counters"] == want and got["last_seen"].tolist() == a["last_seen"].tolist() and not got["gone_bits"].any()
    assert all(len(got[k]) == 0 for k in ROW_FIELDS + ("free_out",))


def test_l_param_is_the_uuids_text():
    for name in ("mix_1025", "everybody_stale", "positions_63_and_64"):
        got = definition(name)
        text, off = got["l_param"].tobytes(), got["l_param_offsets"]
        assert len(got["l_uuid"]) > 0
        for k, u in enumerate(got["l_uuid"]):
            assert text[int(off[k]):int(off[k + 1])].decode() == str(uuid.UUID(bytes=u.tobytes()))


def test_now_must_not_be_the_never_stamp():
    a = cases()["mix_65"]
    with pytest.raises(ValueError):
        define(dict(a, now=NEVER))


# ---- a population through a real PeerIds ----------------------------------------------------------------------

def table_of(ids: PeerIds):
    """The sender table a PeerIds describes, its peers being uuid bytes."""
    keys = sorted(ids._ids)
    tu = np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 16).copy() if keys else np.zeros((0, 16), np.uint8)
    return tu, np.array([ids._ids[k] for k in keys], np.uint32)


def test_200_random_sweeps_through_a_real_peer_ids():
    rng = np.random.default_rng(11)
    ids, seen, n_ids = PeerIds(), np.full(256, NEVER, np.uint32), 256
    born = {}                                    # uuid -> the sweep before which it joined
    left = reused = stamped = 0
    for t in range(1, 201):
        joiners = [uuid.UUID(int=int(rng.integers(1, 1 << 62)) << 64 | t << 8 | k).bytes for k in range(int(rng.integers(0, 6)))]
        for u in joiners:
            reused += bool(ids._free)
            pid = ids.id(u)
            born[u] = t
            assert seen[pid] == NEVER, "a recycled id carries its previous owner's stamp"
        for u, pid in ids._ids.items():          # heartbeats, as the dispatch stamps them
            if born[u] < t and rng.random() < 0.6:
                seen[pid] = t
        members = sorted(ids._ids)
        listed = [ids._ids[u] for u in members if rng.random() < 0.02]
        free = ids.free_in_pop_order()
        got = ingest.leave_peers_np(*table_of(ids), seen, t, 3, None, listed + listed[:1], free, len(members), len(free) + len(members))
        c = got["counters"]
        assert c["overflow"] == 0 and c["error"] == 0 and c["n_table_before"] == len(members)
        gone = [u.tobytes() for u in got["l_uuid"]]
        assert not [u for u, r in zip(gone, got["l_reason"]) if born[u] == t and r & abi.LEAVE_STALE], "a fresh joiner was swept"
        ids.release_ids(gone, got["l_id"])
        assert ids.free_in_pop_order() == got["free_out"].tolist(), t
        tu, ti = table_of(ids)
        assert tu.tobytes() == got["table"][0].tobytes() and ti.tolist() == got["table"][1].tolist()
        seen = got["last_seen"]
        assert all(seen[i] == NEVER for i in ids._free) and all(seen[i] != NEVER for i in ids._ids.values())
        left, stamped = left + len(gone), stamped + c["n_stamped"]
    assert left > 200 and reused > 150 and stamped > 200 and len(ids) > 5


def test_release_ids_refuses_what_the_map_does_not_hold():
    ids = PeerIds()
    for p in "abcd":
        ids.id(p)
    before = (dict(ids._ids), list(ids._peers), list(ids._free))
    for peers, given in ((["a", "b"], [0]), (["a", "b"], [0, 2]), (["a", "x"], [0, 1]), (["a", "a"], [0, 0]), (["b"], [7])):
        with pytest.raises(ValueError):
            ids.release_ids(peers, given)
        assert (ids._ids, ids._peers, ids._free) == before
    ids.release_ids(["c", "a"], np.array([2, 0], np.uint32))
    assert ids._free == [2, 0] and ids.free_in_pop_order() == [0, 2] and ids._ids == {"b": 1, "d": 3}
    ids.release_ids([], [])
    assert ids.id("e") == 0 and ids.id("f") == 2


# ---- the GPU test's lifecycle, on the CPU -------------------------------------------------------------------

class Lifecycle:
    """The host's side of the GPU lifecycle test (tests/test_gpu_ingest_leave.py), shared with the CPU model
    below so that both draw the same population: 3,000 events in ticks of 97 and 400 frames, heartbeats from
    the members behind every tick's frames, a sweep after every tick. Peers that left keep sending for a
    while, as a client that was cut off does, and come back with their next subscribe."""
    SEED, N_EVENTS, SIZES = 5, 3000, (97, 400)
    P_HEARTBEAT, MAX_AGE, P_LISTED, N_FIRST = 0.55, 2, 0.03, 60

    def __init__(self):
        self.rng = np.random.default_rng(self.SEED)
        self.fresh, self.done, self.t, self.departed = 1000, 0, 0, []

    def tick(self, members):
        """The tick's events (population_events' Messages) and the members whose heartbeat follows them."""
        from test_gpu_ingest_join import population_events
        size = self.SIZES[self.t % 2]
        chunk, self.fresh = population_events(size, seed=300 + self.t, known=sorted(members) + sorted(self.departed),
                                              fresh_from=self.fresh)
        beats = [m for m in sorted(members) if self.rng.random() < self.P_HEARTBEAT]
        return chunk, beats

    def listed(self, members, joiners):
        """The disconnects the transport reports after the tick: members, none of them a joiner of this tick."""
        return [m for m in sorted(members) if m not in joiners and self.rng.random() < self.P_LISTED]

    def swept(self, leavers, size):
        self.departed = [m for m in self.departed if m not in leavers][-40:] + sorted(leavers)
        self.done += size
        self.t += 1

    @staticmethod
    def subscribers(chunk):
        """The senders the tick's subscribes give an id, in order: SubscriptionProcessor's rule."""
        from worldql_server_amd.processing import AREA_SUBSCRIBE
        return [ev.sender_uuid for ev in chunk if ev.instruction == AREA_SUBSCRIBE and ev.world_name != "@global"
                and ev.position is not None]


def test_the_gpu_lifecycles_population_is_not_vacuous():
    """The same population through leave_peers_np and a sequential PeerIds: the outcomes the GPU test asserts
    (more than 30 stale, 30 listed, 30 ids reused, 200 joined) hold for its seed and probabilities."""
    from test_ingest_dispatch_host import peer_uuid
    life, ids = Lifecycle(), PeerIds()
    for k in range(Lifecycle.N_FIRST):
        ids.id(f"peer-{k}")
    seen = np.full(1024, NEVER, np.uint32)
    stale = listed_n = reused = joined = 0
    while life.done < Lifecycle.N_EVENTS:
        members = set(ids._ids)
        chunk, beats = life.tick(members)
        joiners = set()
        for name in Lifecycle.subscribers(chunk):
            if ids.lookup(name) is None:
                reused += bool(ids._free)
                ids.id(name)
                joiners.add(name)
        joined += len(joiners)
        for m in beats:
            seen[ids._ids[m]] = life.t + 1
        listed = life.listed(set(ids._ids), joiners)
        keys = sorted(ids._ids, key=lambda m: peer_uuid(m).bytes)
        tu = np.frombuffer(b"".join(peer_uuid(m).bytes for m in keys), np.uint8).reshape(-1, 16)
        free = ids.free_in_pop_order()
        got = ingest.leave_peers_np(tu, [ids._ids[m] for m in keys], seen, life.t + 1, Lifecycle.MAX_AGE, None,
                                    [ids._ids[m] for m in listed], free, 1024, 1024)
        assert got["counters"]["overflow"] == 0 and got["counters"]["error"] == 0
        leavers = [f"peer-{uuid.UUID(bytes=u.tobytes()).int - 1}" for u in got["l_uuid"]]
        assert not joiners & set(leavers), "a fresh joiner was swept in the tick it joined"
        stale += int((got["l_reason"] & abi.LEAVE_STALE != 0).sum())
        listed_n += int((got["l_reason"] & abi.LEAVE_LISTED != 0).sum())
        ids.release_ids(leavers, got["l_id"])
        assert ids.free_in_pop_order() == got["free_out"].tolist()
        seen = got["last_seen"]
        life.swept(leavers, len(chunk))
    assert stale > 30 and listed_n > 30 and reused > 30 and joined > 200, (stale, listed_n, reused, joined)
    assert len(ids) > 20
