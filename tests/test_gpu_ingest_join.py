"""GPU parity for the ingest joins (include/wq_router.h wq_ingest_join_device, wq_ingest_drop_peers_device,
csrc/wq_join.hip): new senders get their peer ids on the device.

Bars, all bit-exact against worldql_server_amd/ingest.py join_peers_np / drop_peers_np (the shared case list
of tests/test_ingest_join_host.py):
  - sender, flags, j_*, the counters and the table (through read_peers) are the definition's; every device
    array is guarded with canaries before and behind it, the read-only inputs are as they were;
  - two calls are identical and reuse their scratch; nullable outputs; invalid arguments launch nothing; a
    handle without a reserve is untouched; the three overflows change nothing; a multi-GPU handle;
  - join, then a decode of the next tick resolves the joined uuids; drop, then they are unknown again; an id
    reused by a new uuid never resolves from the old one;
  - end to end on one handle: 6,000 events in ticks of 97 and 400 frames with a steady stream of fresh uuids
    subscribing and known ones disconnecting between the ticks, decode -> join -> dispatch -> process,
    equal the reference's sequential loop event by event with no frame deferred and the sender table set
    once."""
import ctypes
import uuid

import numpy as np
import pytest

from worldql_server_amd import abi, codec, ingest
from worldql_server_amd.processing import (AREA_SUBSCRIBE, AREA_UNSUBSCRIBE, DISCONNECT, GLOBAL_MESSAGE, LOCAL_MESSAGE,
                                           Message)
from worldql_server_amd.subscriptions import PeerIds, Vector3

from test_gpu_peer_pack import CANARY8, Bytes
from test_ingest_dispatch_host import all_worlds, check_events, peer_uuid, sanitized, ticks_of, wire
from test_ingest_join_host import (HB, KNOWN, LOCAL, NO_PEER, OVERFLOWS, SUB, U, UNSUB, case, cases, definition, drop_args,
                                   drop_cases, same)
from tests.seq_reference import WORLD_NAMES, SequentialReference

pytestmark = pytest.mark.gpu

CSIZE = abi.JOIN_COUNTERS_DTYPE.itemsize
J_WIDTH = dict(j_uuid=16, j_id=4, j_frame=4)
IN_WIDTH = dict(instruction=1, world=4, sender_uuid=16, flags=1, sender=4)
OWN_HANDLE = set(OVERFLOWS) | {"table_at_capacity", "table_4096", "no_reserve"}   # the reserved room is the case's


def u32_tensor(a, device="cuda:0"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to(device)


def set_table(r, a):
    """The case's sender table and reserved room on the handle."""
    r.set_ingest_peers(a["table_uuids"], a["table_ids"])
    if a["capacity"] is not None:
        r.reserve_peers(a["capacity"])


class Call:
    """One case on the device: guarded arrays, and the checks after a call."""

    def __init__(self, a, fields=tuple(J_WIDTH), with_counters=True, device="cuda:0"):
        self.a, d = a, a["d"]
        self.n = len(d["instruction"])
        self.want = ingest.join_peers_np(d, a["table_uuids"], a["table_ids"], a["free"], a["id_next"], a["id_limit"], a["capacity"],
                                         a["joined_capacity"] if fields else None)
        self.jc = (a["joined_capacity"] or 0) if fields else 0
        self.src = {k: Bytes(np.ascontiguousarray(d[k]).view(np.uint8).reshape(-1), device=device) for k in IN_WIDTH}
        self.free = Bytes(np.ascontiguousarray(a["free"], np.uint32).view(np.uint8), device=device)
        self.outs = {k: Bytes(n=self.jc * J_WIDTH[k], device=device) for k in fields}
        self.cnt = Bytes(n=CSIZE, device=device) if with_counters else None
        self.i = abi.JoinIn(**{k: b.ptr for k, b in self.src.items()}, free_ids=self.free.ptr if len(a["free"]) else None,
                            n_free=len(a["free"]), id_next=a["id_next"], id_limit=a["id_limit"])
        self.o = abi.JoinOut(**{k: b.ptr for k, b in self.outs.items()}, joined_capacity=self.jc)

    def launch(self, r):
        r.join_peers_device(self.i, self.n, self.o, self.cnt.ptr if self.cnt else None)

    def outputs(self, r):
        """A dict like join_peers_np's after the canary checks (synchronizes)."""
        import torch
        torch.cuda.synchronize()
        got = {}
        for k in ("sender", "flags"):
            raw = self.src[k].read()
            assert (raw[self.src[k].n:] == CANARY8).all() and self.src[k].front_intact(), "written beside " + k
            got[k] = raw[:self.src[k].n].copy().view(np.uint32 if k == "sender" else np.uint8)
        for k in ("instruction", "world", "sender_uuid"):
            assert self.src[k].unchanged(), "an input was written: " + k
        assert self.free.unchanged()
        rows = len(self.want["j_id"])
        for k, b in self.outs.items():
            raw = b.read()
            assert (raw[rows * J_WIDTH[k]:] == CANARY8).all() and b.front_intact(), "written beside the rows of " + k
            v = raw[:rows * J_WIDTH[k]].copy()
            got[k] = v.reshape(rows, 16) if k == "j_uuid" else v.view(np.uint32)
        if self.cnt:
            raw = self.cnt.read()
            assert (raw[CSIZE:] == CANARY8).all() and self.cnt.front_intact(), "written beside the counters"
            got["counters"] = ingest.join_counters(raw[:CSIZE].copy())
        got["table"] = r.read_peers()
        return got

    def check(self, r, what=""):
        same(self.outputs(r), self.want, what, fields=("sender", "flags") + tuple(self.outs), counters=self.cnt is not None)


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    yield r
    r.close()


# ---- the shared cases ---------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases()))
def test_case_equals_the_definition(router, name):
    from worldql_server_amd.router import Router
    a = cases()[name]
    r = Router(16, 0) if name in OWN_HANDLE else router
    set_table(r, a)
    c = Call(a, fields=tuple(J_WIDTH) if a["joined_capacity"] is not None else ())
    c.launch(r)
    c.check(r, name)
    same(c.want, definition(name), name)
    if r is not router:
        r.close()


def test_two_calls_are_identical_and_scratch_is_reused(router):
    """The same tick twice on the same table, the largest case after the smallest, and no allocation at
    steady state."""
    import torch
    big, small = cases()["distinct_every_frame"], cases()["mix_63"]
    first = None
    for _ in range(6):
        free = torch.cuda.mem_get_info()[0]
        for a in (small, big):
            set_table(router, a)
            c = Call(a)
            c.launch(router)
            got = c.outputs(router)
            same(got, c.want, "again")
        first = first or got
        same(got, first, "second call")
        del c
        after = torch.cuda.mem_get_info()[0]
        if after == free:
            return
    pytest.fail("the device's free memory kept changing: no quiet pair in six")


def test_nullable_outputs(router):
    a = cases()["mix_1025"]
    for fields in (("j_uuid",), ("j_id",), ("j_frame",), ("j_uuid", "j_frame"), ()):
        for with_counters in (True, False):
            set_table(router, a)
            c = Call(a, fields=fields, with_counters=with_counters)
            c.launch(router)
            c.check(router, str(fields))
    short = cases()["joined_capacity_short"]        # joined_capacity counts only when a j_* array is given
    set_table(router, short)
    c = Call(short, fields=())
    c.launch(router)
    c.check(router, "no arrays, no capacity")
    assert c.want["counters"]["overflow"] == 0 and c.want["counters"]["n_joined"] == 5


def test_invalid_arguments(router):
    import torch
    from worldql_server_amd.router import WQError, load_library
    a = cases()["mix_65"]
    set_table(router, a)
    before = router.read_peers()
    call = Call(a)

    def invalid(src=call.i, n=call.n, out=call.o):
        with pytest.raises(WQError) as e:
            router.join_peers_device(src, n, out, call.cnt.ptr)
        assert e.value.code == abi.WQ_E_INVALID

    def changed(struct, **kw):
        c = type(struct)()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(struct), ctypes.sizeof(struct))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    invalid(src=None)
    invalid(out=None)
    for k in IN_WIDTH:
        invalid(src=changed(call.i, **{k: None}))
    invalid(src=changed(call.i, free_ids=None))                        # n_free > 0 without the list
    invalid(src=changed(call.i, id_next=a["id_limit"] + 1))
    invalid(n=0xFFFFFFFF)
    lib = load_library()
    assert lib.wq_ingest_join_device(None, ctypes.byref(call.i), call.n, ctypes.byref(call.o), None) == abi.WQ_E_INVALID
    with pytest.raises(WQError):
        router.drop_peers_device(None, 3)
    with pytest.raises(WQError):
        router.drop_peers_device(call.free.ptr, 0xFFFFFFFF)
    with pytest.raises(WQError):
        router.reserve_peers(0xFFFFFFFF)
    torch.cuda.synchronize()
    for b in list(call.src.values()) + list(call.outs.values()) + [call.cnt]:
        assert b.unchanged()                                           # nothing was launched
    after = router.read_peers()
    assert after[0].tobytes() == before[0].tobytes() and after[1].tolist() == before[1].tolist()
    # n_frames == 0 needs no array
    empty = Call(cases()["mix_0"])
    empty.i = changed(empty.i, instruction=None, world=None, sender_uuid=None, flags=None, sender=None)
    set_table(router, cases()["mix_0"])
    empty.launch(router)
    empty.check(router, "empty, null inputs")
    set_table(router, a)
    call.launch(router)
    call.check(router, "after the refused calls")


def test_a_handle_without_a_reserve_is_untouched():
    """Join and drop are no-ops with error bit 1; set_ingest_peers, the decode and read_peers work as before."""
    import torch
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    a = dict(cases()["n_free_larger"], capacity=None)
    set_table(r, a)
    c = Call(a)
    c.launch(r)
    c.check(r, "no reserve")
    assert c.want["counters"]["error"] == abi.JOIN_ERROR_NO_TABLE and c.want["counters"]["n_joined"] == 0
    ids = u32_tensor(a["table_ids"][:5])
    cnt = Bytes(n=CSIZE)
    r.drop_peers_device(ids.data_ptr(), 5, cnt.ptr)
    torch.cuda.synchronize()
    got = ingest.join_counters(cnt.read()[:CSIZE].copy())
    assert got == ingest.drop_peers_np(a["table_uuids"], a["table_ids"], a["table_ids"][:5], reserved=False)["counters"]
    tu, ti = r.read_peers()
    assert tu.tobytes() == a["table_uuids"].tobytes() and ti.tolist() == a["table_ids"].tolist()
    r.close()


@pytest.mark.parametrize("name", sorted(OVERFLOWS))
def test_an_overflow_changes_nothing(name):
    from worldql_server_amd.router import Router
    a = cases()[name]
    r = Router(16, 0)
    set_table(r, a)
    before = r.read_peers()
    c = Call(a)
    c.launch(r)
    got = c.outputs(r)
    assert got["counters"]["overflow"] == OVERFLOWS[name] and got["counters"]["n_joined"] == 5
    assert got["sender"].tobytes() == a["d"]["sender"].tobytes() and got["flags"].tobytes() == a["d"]["flags"].tobytes()
    for b in c.outs.values():
        assert b.unchanged()
    assert got["table"][0].tobytes() == before[0].tobytes() and got["table"][1].tolist() == before[1].tolist()
    same(got, c.want, name)
    # with room, the same frames join
    roomy = dict(a, id_limit=a["id_next"] + 10, capacity=64, joined_capacity=7)
    r.reserve_peers(64)
    c = Call(roomy)
    c.launch(r)
    c.check(r, name + " with room")
    r.close()


@pytest.mark.parametrize("devices", [(0, 0), (0, 1)], ids=["one_device_twice", "two_devices"])
def test_multi_gpu_handle(devices):
    import torch
    from worldql_server_amd.router import Router
    if torch.cuda.device_count() <= max(devices):
        pytest.skip("needs two devices")
    r = Router.multi(16, devices, mode="replicate")
    for name in ("mix_1025", "around_first_subscribe_across_granules"):
        a = cases()[name]
        set_table(r, a)
        c = Call(a)
        c.launch(r)
        c.check(r, name)
    r.close()


@pytest.mark.parametrize("name", sorted(drop_cases()))
def test_drop_equals_the_definition(name):
    import torch
    from worldql_server_amd.router import Router
    tu, ti, cap, ids = drop_args(name)
    want = ingest.drop_peers_np(tu, ti, ids)
    r = Router(16, 0)
    r.set_ingest_peers(tu, ti)
    r.reserve_peers(cap)
    d_ids, cnt = Bytes(ids.view(np.uint8)), Bytes(n=CSIZE)
    for again in range(2):                       # the second call finds nothing left to remove
        r.drop_peers_device(d_ids.ptr if len(ids) else None, len(ids), cnt.ptr)
        torch.cuda.synchronize()
        raw = cnt.read()
        assert (raw[CSIZE:] == CANARY8).all() and cnt.front_intact() and d_ids.unchanged()
        gu, gi = r.read_peers()
        assert gu.tobytes() == want["table"][0].tobytes() and gi.tolist() == want["table"][1].tolist(), name
        c = ingest.join_counters(raw[:CSIZE].copy())
        assert c == (want["counters"] if not again else dict(want["counters"], n_patched=0)), (name, c)
    r.close()


# ---- join, decode, drop, reuse ------------------------------------------------------------------------

WORLDS = all_worlds()


def messages(rows):
    """(instruction code, peer number) rows as received frames: a subscribe or LocalMessage in WORLDS[0]."""
    return codec.serialize_messages([dict(instruction=ins, sender_uuid=uuid.UUID(int=k + 1), world_name=WORLDS[0],
                                          position=(1.0 + k, 2.0, 3.0), replication=0) for ins, k in rows])


def decode(tick, rows):
    import torch
    data, offsets = messages(rows)
    keep = (torch.from_numpy(data.copy()).to("cuda:0"), torch.from_numpy(offsets.view(np.int64).copy()).to("cuda:0"))
    tick.decode(*keep)
    torch.cuda.synchronize()
    return keep


def test_join_then_decode_then_drop_then_reuse():
    """Tick 1: peers 10, 12, 11 join in that order (ids 3, 4, 5). Tick 2's decode resolves them. Peer 11 leaves:
    dropped from the sender table, its id 5 on the free list. Tick 3: 11 is unknown again, peer 20 joins and
    gets 5; tick 4: 20 resolves to 5 and 11 to nothing. Then set_ingest_peers replaces the table as before."""
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    r.set_worlds(WORLDS)
    host = PeerIds()
    for k in range(3):
        host.id(k)
    r.set_ingest_peers([uuid.UUID(int=k + 1) for k in range(3)])
    r.reserve_peers(8)
    tick = ingest.IngestTick(r, capacity=16)

    def step(rows, free=None):
        keep = decode(tick, rows)
        tick.join(None if not free else u32_tensor(free), host.high_water, 64).dispatch()
        j = tick.read_join()
        cnt = tick.read_dispatch()["counters"]
        del keep
        host.adopt([uuid.UUID(bytes=bytes(u)).int - 1 for u in j["j_uuid"]], j["j_id"])
        return tick.read()["sender"].tolist(), j, cnt

    sender, j, cnt = step([(LOCAL, 10), (SUB, 10), (SUB, 12), (LOCAL, 1), (SUB, 11), (LOCAL, 10)])
    assert sender == [NO_PEER, 3, 4, 1, 5, 3] and j["j_id"].tolist() == [3, 4, 5] and cnt["n_deferred"] == 0
    assert j["counters"]["n_table"] == 6 and j["counters"]["id_next"] == 6
    keep = decode(tick, [(LOCAL, 11), (LOCAL, 12), (UNSUB, 10), (HB, 30)])
    assert tick.read()["sender"].tolist() == [5, 4, 3, NO_PEER] and tick.read()["counters"]["n_sender_unknown"] == 1
    gone = u32_tensor([host.release(11)])
    r.remove_peers([5])
    r.drop_peers_device(gone.data_ptr(), 1)
    assert host.free_in_pop_order() == [5] and len(r.read_peers()[1]) == 5
    sender, j, cnt = step([(LOCAL, 11), (SUB, 20), (LOCAL, 20), (UNSUB, 11)], free=host.free_in_pop_order())
    assert sender == [NO_PEER, 5, 5, NO_PEER] and j["j_id"].tolist() == [5] and j["counters"]["n_free_used"] == 1
    keep = decode(tick, [(LOCAL, 20), (LOCAL, 11), (LOCAL, 12)])
    assert tick.read()["sender"].tolist() == [5, NO_PEER, 4]                    # the reused id never resolves from 11
    tu, ti = r.read_peers()
    assert dict(zip([uuid.UUID(bytes=bytes(u)).int - 1 for u in tu], ti.tolist())) == {0: 0, 1: 1, 2: 2, 10: 3, 12: 4, 20: 5}
    # set_ingest_peers keeps working on a reserved handle and keeps the room
    r.set_ingest_peers([uuid.UUID(int=k + 1) for k in (7, 3)], [9, 8])
    keep = decode(tick, [(LOCAL, 3), (LOCAL, 20), (SUB, 40)])
    tick.join(None, 10, 64)
    j = tick.read_join()
    assert j["sender"].tolist() == [8, NO_PEER, 10] and j["counters"]["n_table"] == 3 and j["counters"]["overflow"] == 0
    del keep
    r.close()


# ---- from the wire to the routed runs, with a joining and leaving population ----------------------------------

OK_NAMES = [w for w in WORLD_NAMES if sanitized(w) is not None]      # every world resolves: the only joins are senders
ID_LIMIT = 1024


def population_events(n, seed, known, fresh_from):
    """n events: a steady stream of fresh uuids whose first frames are not always their subscribe, and the
    usual traffic of the peers that have one. known: the names that may send as members."""
    rng = np.random.default_rng(seed)
    known, strangers, fresh, out = list(known), [], fresh_from, []
    for _ in range(n):
        r = rng.random()
        if r < 0.04 or not known:
            name, ins, fresh = f"peer-{fresh}", AREA_SUBSCRIBE, fresh + 1
            known.append(name)
        elif r < 0.06:
            name, ins, fresh = f"peer-{fresh}", (LOCAL_MESSAGE, AREA_UNSUBSCRIBE, GLOBAL_MESSAGE)[int(rng.integers(3))], fresh + 1
            strangers.append(name)
        elif r < 0.09 and strangers:
            name, ins = strangers.pop(int(rng.integers(len(strangers)))), AREA_SUBSCRIBE
            known.append(name)
        else:
            name = known[int(rng.integers(len(known)))] if r < 0.97 or not strangers else strangers[int(rng.integers(len(strangers)))]
            ins = (AREA_SUBSCRIBE, AREA_UNSUBSCRIBE, LOCAL_MESSAGE, GLOBAL_MESSAGE)[int(rng.choice(4, p=[0.3, 0.12, 0.42, 0.16]))]
        world = "@global" if rng.random() < 0.04 else OK_NAMES[int(rng.choice(len(OK_NAMES)))]
        pos = None if rng.random() < 0.02 else Vector3(*map(float, rng.uniform(-40, 40, 3)))
        out.append(Message(ins, name, world, pos, int(rng.choice(4, p=[0.5, 0.2, 0.2, 0.1]))))
    return out, fresh


def test_joining_and_leaving_population_equals_the_sequential_reference():
    """6,000 events in ticks of 97 and 400 frames on one handle: decode, join, dispatch, process. Between the
    ticks known peers disconnect: wq_remove_peers, drop_peers_device, then the id goes on the free list.
    Event by event the recipients are the sequential reference's, as uuids; no tick defers a frame; the host's
    PeerIds after adopt is the sequential one; wq_ingest_set_peers is called once."""
    import torch
    from worldql_server_amd.router import Router
    rng = np.random.default_rng(8)
    host, seq = PeerIds(), PeerIds()
    first = [f"peer-{k}" for k in range(60)]
    for name in first:
        host.id(name), seq.id(name)
    r = Router(16, 0)
    r.set_worlds(WORLDS)
    r.set_ingest_peers([peer_uuid(p) for p in first])          # once, before the first tick
    r.reserve_peers(ID_LIMIT)
    dev = torch.device("cuda:0")
    offs = torch.zeros(400 + 4 * 400 + 8, dtype=torch.int32, device=dev)
    out_peers = torch.zeros(400 * 1024, dtype=torch.int32, device=dev)
    rc = torch.zeros(24 * 400, dtype=torch.uint8, device=dev)
    tick = ingest.IngestTick(r, capacity=16)
    ref = SequentialReference(16)
    nonempty = joined = reused = left = patched_later = 0
    fresh, done, t = 1000, 0, 0
    while done < 6000:
        size = (97, 400)[t % 2]
        chunk, fresh = population_events(size, seed=100 + t, known=sorted(host._ids), fresh_from=fresh)
        data, offsets = wire(chunk)
        d_frames = torch.from_numpy(data.copy()).to(dev)
        d_off = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        free = host.free_in_pop_order()
        d_free = u32_tensor(free) if free else None
        tick.decode(d_frames, d_off).join(d_free, host.high_water, ID_LIMIT).dispatch(now=t + 1)
        cnt, runs, reads = tick.process(offs, out_peers, rc)
        jc = tick.join_counters                                  # read with the dispatch's counters: one read-back
        assert cnt["error"] == 0 and cnt["n_frames"] == len(chunk) and cnt["n_bad"] == 0
        assert cnt["n_deferred"] == 0, t
        assert jc["overflow"] == 0 and jc["error"] == 0 and jc["n_frames"] == len(chunk)
        j = tick.read_join()
        assert j["counters"] == jc
        host.adopt([f"peer-{uuid.UUID(bytes=bytes(u)).int - 1}" for u in j["j_uuid"]], j["j_id"])
        for ev in chunk:                                         # the sequential allocator, as _apply_run asks it
            if ev.instruction == AREA_SUBSCRIBE and ev.world_name != "@global" and ev.position is not None:
                seq.id(ev.sender_uuid)
        assert host._ids == seq._ids and host._peers == seq._peers and host._free == seq._free, t
        assert jc["id_next"] == host.high_water and jc["n_table"] == len(host)
        joined += jc["n_joined"]
        reused += jc["n_free_used"]
        patched_later += jc["n_patched"] - jc["n_candidates"]
        got_d = tick.read_dispatch()
        o, p = offs.cpu().numpy().view(np.uint32), out_peers.cpu().numpy().view(np.uint32)
        route_cnt = rc.cpu().numpy().view(abi.COUNTERS_DTYPE)
        res = [None] * len(chunk)
        for read in reads:
            for key, src in (("local", got_d["l_src"]), ("global", got_d["g_src"])):
                reg = read[key]
                if reg is None:
                    continue
                c = route_cnt[reg["call"]]
                assert c["error"] == 0 and c["overflow"] == 0, (t, read, c)
                lo, hi = reg["rows"]
                ro = o[reg["offsets"]:reg["offsets"] + hi - lo + 1]
                for k in range(hi - lo):
                    res[int(src[lo + k])] = p[reg["peers"] + ro[k]:reg["peers"] + ro[k + 1]].tolist()
        dec = dict(repl=tick.buf["repl"][:len(chunk)].cpu().numpy())
        nonempty += check_events(chunk, dec, got_d, res, ref, lambda ids: [host.peer(int(q)) for q in ids])
        # between the ticks: some members disconnect
        members = sorted(host._ids)
        leaving = [m for m in members if rng.random() < 0.04]
        if leaving:
            gone = [host.lookup(m) for m in leaving]
            d_gone = u32_tensor(gone + gone[:1])
            r.remove_peers(gone)
            r.drop_peers_device(d_gone.data_ptr(), len(gone) + 1)
            torch.cuda.synchronize()
            for m in leaving:
                ref.event(Message(DISCONNECT, m))
                assert host.release(m) == seq.release(m)
            left += len(leaving)
        done += size
        t += 1
    tu, ti = r.read_peers()
    assert {f"peer-{uuid.UUID(bytes=bytes(u)).int - 1}": int(i) for u, i in zip(tu, ti)} == host._ids
    assert r.route_health() == (0, 0)
    assert nonempty > 500 and joined > 200 and reused > 50 and left > 50 and patched_later > 20
    r.close()
