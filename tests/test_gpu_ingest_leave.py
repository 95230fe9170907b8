"""GPU parity for the ingest leaves (include/wq_router.h wq_ingest_leave_device, wq_remove_peers_device,
csrc/wq_leave.hip): stale and disconnected senders leave on the device.

Bars, all bit-exact against worldql_server_amd/ingest.py leave_peers_np (the shared case list of
tests/test_ingest_leave_host.py):
  - the l_* rows, the uuid text, gone_bits, free_out, last_seen, the counters and the table (through
    read_peers) are the definition's; every device array is guarded with canaries before and behind it, the
    read-only inputs are as they were;
  - two calls are identical and reuse their scratch; nullable outputs; invalid arguments launch nothing; an
    overflow changes nothing; a handle without a reserve; a multi-GPU handle;
  - wq_remove_peers_device leaves exactly the table wq_remove_peers leaves on a twin handle; a zero count
    with bits set touches nothing; an empty table;
  - the sweep's l_param / l_param_offsets through the frame builder are the host serializer's PeerDisconnect
    frames;
  - end to end on one handle: 3,000 events in ticks of 97 and 400 frames of a joining, heart-beating and
    leaving population, a sweep after every tick, equal the reference's sequential loop event by event with
    no frame deferred, no host-side removal between the ticks and the sender table set once."""
import ctypes
import uuid

import numpy as np
import pytest

from worldql_server_amd import abi, codec, ingest
from worldql_server_amd.processing import DISCONNECT, Message
from worldql_server_amd.subscriptions import PeerIds

from test_gpu_peer_pack import CANARY8, Bytes
from test_gpu_ingest_join import ID_LIMIT, OK_NAMES, WORLDS, u32_tensor
from test_ingest_dispatch_host import INS_CODE, check_events, peer_uuid
from test_ingest_leave_host import OVERFLOWS, ROW_FIELDS, Lifecycle, cases, define, definition, same
from tests.seq_reference import SequentialReference

pytestmark = pytest.mark.gpu

CSIZE = abi.LEAVE_COUNTERS_DTYPE.itemsize
WIDTH = dict(l_uuid=16, l_id=4, l_reason=1, l_param=abi.LEAVE_TEXT)
ALL_OUT = ROW_FIELDS + ("gone_bits", "free_out")
DTYPES = dict(l_id=np.uint32, l_param_offsets=np.uint64, gone_bits=np.uint32, free_out=np.uint32)
OWN_HANDLE = {"table_full_to_its_reserve", "no_reserve"}          # the reserved room is the case's


def set_table(r, a):
    """The case's sender table and reserved room on the handle."""
    r.set_ingest_peers(a["table_uuids"], a["table_ids"])
    if a["reserved"]:
        r.reserve_peers(a["capacity"])


def fields_of(a):
    return tuple(k for k in ALL_OUT if (a["leave_capacity"] is not None or k not in ROW_FIELDS) and
                 (a["free_capacity"] is not None or k != "free_out"))


class Call:
    """One case on the device: guarded arrays, and the checks after a call."""

    def __init__(self, a, fields=None, with_counters=True, device="cuda:0"):
        fields = fields_of(a) if fields is None else fields
        rows = any(k in fields for k in ROW_FIELDS)
        self.a, self.fields = a, fields
        self.want = define(dict(a, leave_capacity=a["leave_capacity"] if rows else None,
                                free_capacity=a["free_capacity"] if "free_out" in fields else None))
        self.n_ids = len(a["last_seen"])
        lc = (a["leave_capacity"] or 0) if rows else 0
        fc = (a["free_capacity"] or 0) if "free_out" in fields else 0
        words = (self.n_ids + 31) // 32
        as_bytes = lambda v: Bytes(np.ascontiguousarray(v, np.uint32).view(np.uint8), device=device)
        self.seen, self.free, self.listed = as_bytes(a["last_seen"]), as_bytes(a["free"]), as_bytes(a["leave_ids"])
        self.pinned = as_bytes(a["pinned"]) if a["pinned"] is not None else None
        room = dict({k: lc * w for k, w in WIDTH.items()}, l_param_offsets=8 * (lc + 1), gone_bits=4 * words, free_out=4 * fc)
        self.outs = {k: Bytes(n=room[k], device=device) for k in fields}
        self.cnt = Bytes(n=CSIZE, device=device) if with_counters else None
        self.i = abi.LeaveIn(last_seen=self.seen.ptr, pinned_bits=self.pinned.ptr if self.pinned else None,
                             leave_ids=self.listed.ptr if len(a["leave_ids"]) else None,
                             free_ids=self.free.ptr if len(a["free"]) else None, n_ids=self.n_ids, now=a["now"],
                             max_age=a["max_age"], n_leave=len(a["leave_ids"]), n_free=len(a["free"]))
        self.o = abi.LeaveOut(**{k: b.ptr for k, b in self.outs.items()}, leave_capacity=lc, free_capacity=fc)

    def launch(self, r):
        r.leave_peers_device(self.i, self.o, self.cnt.ptr if self.cnt else None)

    def outputs(self, r):
        """A dict like leave_peers_np's after the canary checks (synchronizes)."""
        import torch
        torch.cuda.synchronize()
        raw = self.seen.read()
        assert (raw[self.seen.n:] == CANARY8).all() and self.seen.front_intact(), "written beside last_seen"
        got = dict(last_seen=raw[:self.seen.n].copy().view(np.uint32))
        assert self.free.unchanged() and self.listed.unchanged() and (self.pinned is None or self.pinned.unchanged())
        k = len(self.want["l_id"])
        wrote = dict({f: k * w for f, w in WIDTH.items()}, l_param_offsets=8 * len(self.want["l_param_offsets"]),
                     gone_bits=4 * ((self.n_ids + 31) // 32), free_out=4 * len(self.want["free_out"]))
        for f, b in self.outs.items():
            raw = b.read()
            assert (raw[wrote[f]:] == CANARY8).all() and b.front_intact(), "written beside the rows of " + f
            v = raw[:wrote[f]].copy()
            got[f] = v.reshape(k, 16) if f == "l_uuid" else v.view(DTYPES.get(f, np.uint8))
        if self.cnt:
            raw = self.cnt.read()
            assert (raw[CSIZE:] == CANARY8).all() and self.cnt.front_intact(), "written beside the counters"
            got["counters"] = ingest.leave_counters(raw[:CSIZE].copy())
        got["table"] = r.read_peers()
        return got

    def check(self, r, what=""):
        same(self.outputs(r), self.want, what, fields=self.fields + ("last_seen",), counters=self.cnt is not None)


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
    c = Call(a)
    c.launch(r)
    c.check(r, name)
    same(c.want, definition(name), name)
    if name in OVERFLOWS:
        assert c.want["counters"]["overflow"] == OVERFLOWS[name]
    if r is not router:
        r.close()


def test_two_calls_are_identical_and_scratch_is_reused(router):
    """The same sweep twice on the same table, the largest case after the smallest, and no allocation at
    steady state."""
    import torch
    big, small = cases()["mix_1025"], cases()["mix_63"]
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


def test_a_second_sweep_finds_nobody(router):
    """What the first sweep left, swept again with the same clock: nobody leaves, nobody is stamped."""
    a = cases()["mix_1025"]
    set_table(router, a)
    c = Call(a)
    c.launch(router)
    c.check(router, "first")
    w = c.want
    again = dict(a, table_uuids=w["table"][0], table_ids=w["table"][1], last_seen=w["last_seen"], free=w["free_out"],
                 free_capacity=len(w["free_out"]) + len(w["table"][1]), leave_capacity=len(w["table"][1]))
    c2 = Call(again)                      # the handle's table is already what the first sweep left
    c2.launch(router)
    c2.check(router, "second")
    assert c2.want["counters"]["n_left"] == 0 and c2.want["counters"]["n_stamped"] == 0 and not c2.want["gone_bits"].any()


def test_nullable_outputs(router):
    a = cases()["mix_1025"]
    for fields in (("l_uuid",), ("l_id",), ("l_reason",), ("l_param", "l_param_offsets"), ("l_param_offsets",), ("gone_bits",),
                   ("free_out",), ("l_id", "free_out"), ()):
        for with_counters in (True, False):
            set_table(router, a)
            c = Call(a, fields=fields, with_counters=with_counters)
            c.launch(router)
            c.check(router, str(fields))
    both = cases()["both_overflows"]          # a capacity counts only when its array is given
    for fields, overflow in ((("gone_bits",), 0), (("l_id",), 1), (("free_out",), 2)):
        set_table(router, both)
        c = Call(both, fields=fields)
        c.launch(router)
        c.check(router, "capacities and " + str(fields))
        assert c.want["counters"]["overflow"] == overflow and c.want["counters"]["n_left"] == 11


def test_invalid_arguments(router):
    import torch
    from worldql_server_amd.router import WQError, load_library
    a = cases()["mix_65"]
    set_table(router, a)
    before = router.read_peers()
    call = Call(a)

    def invalid(src=call.i, out=call.o):
        with pytest.raises(WQError) as e:
            router.leave_peers_device(src, out, call.cnt.ptr)
        assert e.value.code == abi.WQ_E_INVALID

    def changed(struct, **kw):
        c = type(struct)()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(struct), ctypes.sizeof(struct))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    invalid(src=None)
    invalid(out=None)
    invalid(src=changed(call.i, last_seen=None))
    invalid(src=changed(call.i, leave_ids=None))                       # n_leave > 0 without the list
    invalid(src=changed(call.i, free_ids=None))                        # n_free > 0 without the list
    for k in ("n_ids", "n_leave", "n_free", "now"):
        invalid(src=changed(call.i, **{k: 0xFFFFFFFF}))
    lib = load_library()
    assert lib.wq_ingest_leave_device(None, ctypes.byref(call.i), ctypes.byref(call.o), None) == abi.WQ_E_INVALID
    assert lib.wq_remove_peers_device(None, call.outs["gone_bits"].ptr, 8, None) == abi.WQ_E_INVALID
    with pytest.raises(WQError) as e:
        router.remove_peers_device(None, 8)
    assert e.value.code == abi.WQ_E_INVALID
    torch.cuda.synchronize()
    for b in [call.seen, call.free, call.listed, call.cnt] + list(call.outs.values()):
        assert b.unchanged()                                           # nothing was launched
    after = router.read_peers()
    assert after[0].tobytes() == before[0].tobytes() and after[1].tolist() == before[1].tolist()
    router.remove_peers_device(None, 0)                                # no ids need no bitmap
    call.launch(router)
    call.check(router, "after the refused calls")


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
    assert got["counters"]["overflow"] == OVERFLOWS[name] and got["counters"]["n_stamped"] == 0
    assert got["last_seen"].tobytes() == a["last_seen"].tobytes() and not got["gone_bits"].any()
    for k, b in c.outs.items():
        assert k == "gone_bits" or b.unchanged()
    assert got["table"][0].tobytes() == before[0].tobytes() and got["table"][1].tolist() == before[1].tolist()
    same(got, c.want, name)
    # with the room it asked for, the same sweep goes through
    n = got["counters"]["n_left"]
    c = Call(dict(a, leave_capacity=n, free_capacity=len(a["free"]) + n))
    c.launch(r)
    c.check(r, name + " with room")
    assert c.want["counters"]["overflow"] == 0 and c.want["counters"]["n_left"] == n
    r.close()


def test_a_handle_without_a_reserve_is_untouched():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    a = cases()["no_reserve"]
    set_table(r, a)
    c = Call(a)
    c.launch(r)
    got = c.outputs(r)
    same(got, c.want, "no reserve")
    assert got["counters"]["error"] == abi.LEAVE_ERROR_NO_TABLE and got["counters"]["n_left"] == 0
    for k, b in c.outs.items():
        assert k == "gone_bits" or b.unchanged()
    r.close()


@pytest.mark.parametrize("devices", [(0, 0), (0, 1)], ids=["one_device_twice", "two_devices"])
def test_multi_gpu_handle(devices):
    import torch
    from worldql_server_amd.router import Router, WQError
    if torch.cuda.device_count() <= max(devices):
        pytest.skip("needs two devices")
    r = Router.multi(16, devices, mode="replicate")
    for name in ("mix_1025", "positions_63_and_64"):
        a = cases()[name]
        set_table(r, a)
        c = Call(a)
        c.launch(r)
        c.check(r, name)
    with pytest.raises(WQError) as e:
        r.remove_peers_device(c.outs["gone_bits"].ptr, c.n_ids)
    assert e.value.code == abi.WQ_E_INVALID and "wq_remove_peers" in str(e.value)
    r.close()


# ---- wq_remove_peers_device against wq_remove_peers ---------------------------------------------------------

N_PEERS, N_IDS = 3000, 3007         # the bitmap's last word is partial


def removal_table():
    """Ops like test_gpu_delta.test_remove_peers_in_place_vs_oracle's, with the cube shapes k_remove_peers
    tells apart: record cubes with 10, 24 (the inline count), 25, 40 and 400 peers, one that loses every peer,
    slot cubes (off-grid raw keys) with 5, 25 and 60 peers, and random cubes around them."""
    rng = np.random.default_rng(21)
    sub = lambda world, peers, **kw: abi.ops_array(np.full(len(peers), world, np.uint32), np.asarray(peers, np.uint32),
                                                   np.zeros(len(peers), np.uint8), **kw)
    at = lambda x, n: dict(pos=np.tile([[x, 8.0, 8.0]], (n, 1)))
    parts = [abi.ops_array(rng.integers(0, 3, 4000).astype(np.uint32), rng.integers(0, N_PEERS, 4000).astype(np.uint32),
                           np.zeros(4000, np.uint8), pos=rng.uniform(-96, 96, (4000, 3)))]
    for k, n in enumerate((10, 24, 25, 40, 400)):
        parts.append(sub(0, np.arange(n), **at(1000.0 + 32 * k, n)))
    parts.append(sub(0, np.arange(1000, 1005), **at(2000.0, 5)))                       # loses every peer
    for k, n in enumerate((5, 25, 60)):
        parts.append(sub(1, np.arange(n), key=np.tile([[3 + 6 * k, 3, 3]], (n, 1))))    # off-grid: the slot table
    parts.append(sub(1, np.arange(1000, 1003), key=np.tile([[33, 3, 3]], (3, 1))))     # a slot cube that loses every peer
    gone = sorted(set(range(0, 400, 2)) | set(range(1000, 1005)) | set(rng.choice(N_PEERS, 150, replace=False).tolist()) |
                  set(range(2990, 3000)) | {3001, 3006})                               # and ids that hold nothing
    return abi.concat_ops(parts), np.array(gone, np.uint32)


def test_remove_peers_device_equals_remove_peers():
    import torch
    from worldql_server_amd.router import Router
    ops, gone = removal_table()
    a, b = Router(16, 0), Router(16, 0)
    for r in (a, b):
        r.apply_ops(ops)
    before = a.export_table().tobytes()
    assert before == b.export_table().tobytes()
    bits = u32_tensor(ingest.id_bits(gone, N_IDS))
    count = torch.tensor([len(gone)], dtype=torch.int64, device="cuda:0")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    keep = bits.clone()
    # a zero count with bits set: every block returns before it touches the table
    b.remove_peers_device(bits.data_ptr(), N_IDS, zero.data_ptr())
    torch.cuda.synchronize()
    assert b.export_table().tobytes() == before and b.stats() == a.stats()
    a.remove_peers(gone)
    b.remove_peers_device(bits.data_ptr(), N_IDS, count.data_ptr())
    got, want = b.export_table(), a.export_table()
    assert got.tobytes() == want.tobytes() and len(want) < len(ops) and want.tobytes() != before
    assert not np.isin(want["peer"], gone).any()
    assert a.stats() == b.stats() and a.route_health() == (0, 0) and b.route_health() == (0, 0)
    assert torch.equal(bits, keep)
    # without a count, and a second time: nothing is left to remove
    b.remove_peers_device(bits.data_ptr(), N_IDS)
    assert b.export_table().tobytes() == want.tobytes() and a.stats() == b.stats()
    # both keep taking batches
    more = abi.ops_array(np.zeros(50, np.uint32), np.arange(50, dtype=np.uint32), np.zeros(50, np.uint8),
                         pos=np.tile([[1000.0, 8.0, 8.0]], (50, 1)))
    for r in (a, b):
        r.apply_ops(more)
    assert a.export_table().tobytes() == b.export_table().tobytes() and a.stats() == b.stats()
    a.close()
    b.close()


def test_remove_peers_device_on_an_empty_table():
    import torch
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    bits = u32_tensor(ingest.id_bits([1, 2, 40], 64))
    r.remove_peers_device(bits.data_ptr(), 64)
    torch.cuda.synchronize()
    assert len(r.export_table()) == 0 and r.stats()["n_entries"] == 0 and r.route_health() == (0, 0)
    r.close()


# ---- the PeerDisconnect frames ---------------------------------------------------------------------------------

def test_peer_disconnect_frames_come_from_the_sweeps_text():
    """peer_map.rs:121-141: PeerDisconnect (instruction 3) with parameter = uuid.to_string() and every other
    field default. The sweep's l_param / l_param_offsets go through the frame builder as they are."""
    import torch
    from worldql_server_amd.router import Router
    a = cases()["mix_257"]
    r = Router(16, 0)
    r.set_worlds(WORLDS + [""])                           # the default world name is the empty one
    set_table(r, a)
    c = Call(a)
    c.launch(r)
    got = c.outputs(r)
    k = len(got["l_id"])
    assert k > 20
    want_data, want_off = codec.serialize_messages([dict(instruction=3, parameter=str(uuid.UUID(bytes=u.tobytes())))
                                                     for u in got["l_uuid"]])
    dev = "cuda:0"
    nil = torch.zeros(16 * k, dtype=torch.uint8, device=dev)
    world = u32_tensor(np.full(k, len(WORLDS), np.uint32))
    src = abi.FramesSrc(instruction=None, instruction_all=3, replication=None, replication_all=0, sender_uuid=nil.data_ptr(),
                        world=world.data_ptr(), pos=None, param=c.outs["l_param"].ptr, param_offsets=c.outs["l_param_offsets"].ptr,
                        n_param_bytes=abi.LEAVE_TEXT * k, flex=None, flex_offsets=None, n_flex_bytes=0, msg_flags=None)
    frames = torch.zeros(len(want_data) + 64, dtype=torch.uint8, device=dev)
    offsets = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    cnt = torch.zeros(abi.FRAMES_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    r.build_frames_device(src, k, frames.data_ptr(), frames.numel(), offsets.data_ptr(), None, cnt.data_ptr())
    torch.cuda.synchronize()
    fc = cnt.cpu().numpy().view(abi.FRAMES_COUNTERS_DTYPE)[0]
    assert fc["error"] == 0 and fc["overflow"] == 0 and fc["n_complete"] == k
    assert offsets.cpu().numpy().view(np.uint64).tolist() == want_off.tolist()
    assert frames.cpu().numpy()[:len(want_data)].tobytes() == want_data.tobytes()
    r.close()


# ---- from the wire to the routed runs, with a joining, heart-beating and leaving population -----------------------

def wire_with_heartbeats(chunk, beats):
    """The tick's events as received frames, then a heartbeat (instruction 0) from every name in `beats`."""
    msgs = [dict(instruction=INS_CODE[e.instruction], sender_uuid=peer_uuid(e.sender_uuid), world_name=e.world_name,
                 position=None if e.position is None else (e.position.x, e.position.y, e.position.z),
                 replication=e.replication) for e in chunk]
    msgs += [dict(instruction=0, sender_uuid=peer_uuid(m), world_name=OK_NAMES[0]) for m in beats]
    return codec.serialize_messages(msgs)


def name_of(u) -> str:
    return f"peer-{uuid.UUID(bytes=bytes(u)).int - 1}"


def test_joining_heartbeating_and_leaving_population_equals_the_sequential_reference():
    """Lifecycle's 3,000 events on one handle: decode, join, dispatch (the heartbeats stamp last_seen), process,
    then IngestTick.leave: the sweep and the table's removal, with nothing but the transport's disconnects
    handed over by the host. Event by event the recipients are the sequential reference's; no tick defers a
    frame; the host's PeerIds after adopt and release_ids is the sequential one; no joiner is swept in the tick
    it joined; wq_ingest_set_peers is called once."""
    import torch
    from worldql_server_amd.router import Router
    life = Lifecycle()
    host, seq = PeerIds(), PeerIds()
    first = [f"peer-{k}" for k in range(Lifecycle.N_FIRST)]
    for name in first:
        host.id(name), seq.id(name)
    r = Router(16, 0)
    r.set_worlds(WORLDS)
    r.set_ingest_peers([peer_uuid(p) for p in first])          # once, before the first tick
    r.reserve_peers(ID_LIMIT)
    dev = torch.device("cuda:0")
    room = 400 + ID_LIMIT
    offs = torch.zeros(room + 4 * room + 8, dtype=torch.int32, device=dev)
    out_peers = torch.zeros(400 * 1024, dtype=torch.int32, device=dev)
    rc = torch.zeros(24 * room, dtype=torch.uint8, device=dev)
    last_seen = torch.full((ID_LIMIT,), -1, dtype=torch.int32, device=dev)      # all ones: nobody was seen yet
    tick = ingest.IngestTick(r, capacity=16)
    ref = SequentialReference(16)
    nonempty = joined = reused = stale = listed_n = stamped = 0
    while life.done < Lifecycle.N_EVENTS:
        t = life.t
        chunk, beats = life.tick(set(host._ids))
        data, offsets = wire_with_heartbeats(chunk, beats)
        n = len(chunk) + len(beats)
        d_frames = torch.from_numpy(data.copy()).to(dev)
        d_off = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        free = host.free_in_pop_order()
        d_free = u32_tensor(free) if free else None
        tick.decode(d_frames, d_off).join(d_free, host.high_water, ID_LIMIT).dispatch(last_seen=last_seen, now=t + 1)
        cnt, runs, reads = tick.process(offs, out_peers, rc)
        jc = tick.join_counters
        assert cnt["error"] == 0 and cnt["n_frames"] == n and cnt["n_bad"] == 0
        assert cnt["n_deferred"] == 0, t
        assert jc["overflow"] == 0 and jc["error"] == 0
        j = tick.read_join()
        joiners = [name_of(u) for u in j["j_uuid"]]
        host.adopt(joiners, j["j_id"])
        for name in Lifecycle.subscribers(chunk):
            seq.id(name)
        assert host._ids == seq._ids and host._peers == seq._peers and host._free == seq._free, t
        joined += jc["n_joined"]
        reused += jc["n_free_used"]
        got_d = tick.read_dispatch()
        o, p = offs.cpu().numpy().view(np.uint32), out_peers.cpu().numpy().view(np.uint32)
        route_cnt = rc.cpu().numpy().view(abi.COUNTERS_DTYPE)
        res = [None] * n
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
        # the sweep: the transport's disconnects are all the host hands over
        listed = life.listed(set(host._ids), set(joiners))
        d_listed = u32_tensor([host.lookup(m) for m in listed]) if listed else None
        free = host.free_in_pop_order()
        d_free = u32_tensor(free) if free else None
        members_before = len(host)
        tick.leave(last_seen, now=t + 1, max_age=Lifecycle.MAX_AGE, leave_ids=d_listed, free_ids=d_free)
        lv = tick.read_leave()
        lc = lv["counters"]
        assert lc["overflow"] == 0 and lc["error"] == 0 and lc["n_table_before"] == members_before
        assert lc["n_listed"] == len(listed) == lc["n_listed_found"]
        leavers = [name_of(u) for u in lv["l_uuid"]]
        assert not set(joiners) & set(leavers), "a fresh joiner was swept in the tick it joined"
        assert lv["l_param"].tobytes().decode() == "".join(str(peer_uuid(m)) for m in leavers)
        host.release_ids(leavers, lv["l_id"])
        for m in leavers:
            ref.event(Message(DISCONNECT, m))
            seq.release(m)
        assert host._ids == seq._ids and host._peers == seq._peers and host._free == seq._free, t
        assert host.free_in_pop_order() == lv["free_out"].tolist() and lc["n_table"] == len(host)
        assert lv["gone_bits"].tolist() == ingest.id_bits(lv["l_id"], ID_LIMIT).tolist()
        seen = lv["last_seen"]
        assert all(seen[i] == abi.SEEN_NEVER for i in host._free) and all(seen[i] != abi.SEEN_NEVER for i in host._ids.values())
        stale += int((lv["l_reason"] & abi.LEAVE_STALE != 0).sum())
        listed_n += int((lv["l_reason"] & abi.LEAVE_LISTED != 0).sum())
        stamped += lc["n_stamped"]
        life.swept(leavers, len(chunk))
    tu, ti = r.read_peers()
    assert {name_of(u): int(i) for u, i in zip(tu, ti)} == host._ids
    assert r.route_health() == (0, 0)
    assert stale > 30 and listed_n > 30 and reused > 30 and joined > 200, (stale, listed_n, reused, joined)
    assert nonempty > 200 and stamped >= joined          # every joiner's clock was started by a sweep
    r.close()
