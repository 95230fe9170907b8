"""GPU parity for the record dispatch (include/wq_router.h wq_records_dispatch_device,
csrc/wq_recdispatch.hip): a tick's record frames to store ops and queries on the device.

Bars, all bit-exact against worldql_server_amd/ingest.py records_dispatch_np (the shared cases of
tests/test_records_dispatch_host.py and the shapes of tests/test_records_dispatch_cpp_mirror.py):
  - every output array, the run table and the counters are the definition's;
  - every device array is guarded: every output is sized exactly to the rows the definition writes, with
    canaries before and behind it, every input is as it was, and the frame bytes sit at an odd address;
  - capacity cuts, the allocator's three cases, every nullable output left out in turn;
  - two calls give identical bytes and a steady-state call allocates nothing;
  - end to end on one handle: frames -> decode -> dispatch -> records dispatch -> DeviceRecordProcessor on a
    GpuRecordStore, over 3,000 random events in ticks of 97 and 400 frames, gives RecordProcessor.process's
    replies on a RecordStoreRef, tick by tick, the same totals and the same live rows; with two worlds
    missing from the table every read before first_deferred is answered alike and the deferred list is the
    definition's."""
import ctypes

import numpy as np
import pytest

from worldql_server_amd import abi, ingest, records
from worldql_server_amd.world_names import WorldIds

import test_gpu_frames_decode as decode_gpu
import test_gpu_ingest_dispatch as dispatch_gpu
import test_gpu_peer_pack as pack_gpu
from test_frames_decode_host import batches
from test_gpu_peer_pack import CANARY8, Bytes
from test_ingest_dispatch_host import cases as dispatch_cases
from test_records_dispatch_cpp_mirror import CSIZE, WIDTH, capacities, rows_written, shape, shapes
from test_records_dispatch_host import (ARRAYS, NOW, PEERS, SIZES, TABLE_SIZE, WORLDS, Case, hostile, named, processor_events,
                                        random_events, same)

pytestmark = pytest.mark.gpu


class Call:
    """One case on the device: guarded inputs and outputs, and the checks after a call."""

    def __init__(self, case, fields=ARRAYS, with_counters=True, shift=1, device="cuda:0", **over):
        probe = case.definition(**{k: v for k, v in over.items() if k in ("max_records", "free_handles", "handle_next")})
        self.caps = capacities(probe, fields, over)
        self.want = case.definition(**dict(over, **self.caps))
        kw = dict(case.kw, **over)
        free = np.array(kw["free_handles"] if kw["free_handles"] is not None else [], np.uint32)
        arrays = dict(frames=(case.data, shift), frame_offsets=(np.array(case.offsets, np.uint64), 0),
                      msg=(case.decoded["msg"], 0), world=(np.array(case.decoded["world"], np.uint32), 4 * shift),
                      flags=(case.decoded["flags"], shift), free_handles=(free, 4 * shift))
        if case.db_src is not None:
            arrays["db_src"] = (np.array(case.db_src, np.uint32), 4 * shift)
        self.src = {k: Bytes(np.ascontiguousarray(a).view(np.uint8).reshape(-1), shift=s, device=device) for k, (a, s) in arrays.items()}
        ptr = lambda k: self.src[k].ptr if k in self.src and self.src[k].n else None  # noqa: E731
        total = probe["counters"]["n_records_total"]
        self.a = abi.RecDispatchIn(frames=ptr("frames"), frame_offsets=self.src["frame_offsets"].ptr, n_frames=len(case.offsets) - 1,
                                   n_frame_bytes=len(case.data), msg=ptr("msg"), world=ptr("world"), flags=ptr("flags"),
                                   db_src=ptr("db_src"), n_db=case.n_db, now_us=kw["now_us"], free_handles=ptr("free_handles"),
                                   n_free=len(free), handle_next=kw["handle_next"],
                                   max_records=total if kw.get("max_records") is None else kw["max_records"])
        self.rows = {k: rows_written(k, self.want) for k in fields}
        self.outs = {k: Bytes(n=self.rows[k] * WIDTH[k], device=device) for k in fields}
        self.cnt = Bytes(n=CSIZE, device=device) if with_counters else None
        cap_of = dict(ops="ops_capacity", op_ref="ops_capacity", defer="defer_capacity", runs="runs_capacity")
        given = {k: b.ptr for k, b in self.outs.items() if k not in cap_of or self.caps[cap_of[k]]}   # no array with capacity 0
        self.out = abi.RecDispatchOut(**given, **self.caps)

    def launch(self, r):
        """Enqueues the call; nothing is waited for."""
        r.records_dispatch_device(self.a, self.out, self.cnt.ptr if self.cnt else None)

    def outputs(self):
        """A dict like records_dispatch_np's (outputs left out: None) after the canary checks."""
        import torch
        torch.cuda.synchronize()
        got = dict.fromkeys(ARRAYS)
        for k, b in self.outs.items():
            raw = b.read()
            assert (raw[self.rows[k] * WIDTH[k]:] == CANARY8).all(), "written behind " + k
            assert b.front_intact(), "written before " + k
            got[k] = shape(k, raw, self.rows[k])
        if self.cnt:
            raw = self.cnt.read()
            assert (raw[CSIZE:] == CANARY8).all() and self.cnt.front_intact(), "written beside the counters"
            got["counters"] = ingest.records_dispatch_counters(raw[:CSIZE].copy())
        for k, b in self.src.items():
            assert b.unchanged(), "an input was written: " + k
        return got

    def run(self, r):
        import torch
        torch.cuda.synchronize()
        self.launch(r)
        return self.outputs()

    def check(self, what=""):
        same(self.outputs(), self.want, what, fields=tuple(self.outs), counters=self.cnt is not None)


def open_router(worlds=WORLDS, store=True):
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    r.set_worlds(worlds)
    r.set_ingest_peers(PEERS)
    return r, (records.GpuRecordStore(r, *SIZES, TABLE_SIZE) if store else None)


@pytest.fixture(scope="module")
def router():
    r, _ = open_router()
    yield r
    r.close()


# ---- the shared cases ---------------------------------------------------------------------

def all_cases():
    out = {"named/" + k: v for k, v in named().items() if k != "no_table"}
    out.update({"hostile/" + k: v for k, v in hostile().items()})
    out.update({"shape/" + k: v for k, v in shapes().items()})
    return out


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_case_equals_the_definition(router, name):
    c = Call(all_cases()[name])
    c.launch(router)
    c.check(name)


def test_a_handle_without_a_world_table():
    r, _ = open_router(worlds=[])
    c = Call(named()["no_table"])
    c.launch(r)
    c.check("no_table")
    r.close()


def test_capacity_cuts(router):
    case = shapes()["one_frame_65"]
    n_ops = case.definition()["counters"]["n_creates"]
    big = shapes()["n_db_1025"]
    c = big.definition()["counters"]
    calls = [Call(case, ops_capacity=cap) for cap in (0, 1, n_ops // 2, n_ops - 1)]      # cuts inside the frame
    calls += [Call(big, defer_capacity=cap) for cap in (0, 1)]
    calls += [Call(big, runs_capacity=cap) for cap in (0, 1, c["n_runs"], c["n_runs"] + 1)]
    calls += [Call(big, max_records=limit) for limit in (0, 1, 64, c["n_records_total"] // 2, c["n_records_total"] - 1)]
    for k in calls:
        k.launch(router)
    for k in calls:
        k.check(str(k.caps))
    assert calls[0].want["counters"]["overflow"] == abi.RECDISP_OVERFLOW_OPS
    assert calls[-1].want["counters"]["overflow"] == abi.RECDISP_OVERFLOW_RECORDS


def test_the_allocator(router):
    case = shapes()["n_db_65"]
    creates = case.definition()["counters"]["n_creates"]
    for free in ([], [5, 3, 8], list(range(1000, 1000 + creates + 4))):     # none, below and above the creates
        c = Call(case, free_handles=free, handle_next=0xFFFFFFFE)
        c.launch(router)
        c.check(f"{len(free)} free")


def test_nullable_outputs(router):
    case = shapes()["n_db_65"]
    combos = [()] + [tuple(k for k in ARRAYS if k != left_out) for left_out in ARRAYS] + [("runs",), ("ops",), ("op_ref", "cls")]
    calls = [Call(case, fields=f, with_counters=wc) for f in combos for wc in ((True, False) if len(f) < 3 else (True,))]
    for c in calls:
        c.launch(router)
    for c in calls:
        c.check(str(tuple(c.outs)))


def test_two_calls_are_identical_and_scratch_is_reused(router):
    """The same call twice, the largest case after the smallest, and no allocation at steady state."""
    import torch
    big, small = Call(shapes()["one_big_frame_among_empty_ones"]), Call(shapes()["n_db_63"])
    first = big.run(router)
    for _ in range(5):
        free = torch.cuda.mem_get_info()[0]
        small.run(router)
        again = big.run(router)
        same(again, first, "second call")
        after = torch.cuda.mem_get_info()[0]
        assert after >= free, ("a steady-state call allocated", free - after)
        if after == free:
            return
    pytest.fail("the device's free memory kept rising: no quiet pair in five")


def test_invalid_arguments(router):
    import torch
    from worldql_server_amd.router import Router, WQError, load_library
    call = Call(shapes()["n_db_65"], free_handles=[1, 2])

    def invalid(r=router, src=call.a, out=call.out):
        with pytest.raises(WQError) as e:
            r.records_dispatch_device(src, out, call.cnt.ptr)
        assert e.value.code == abi.WQ_E_INVALID

    def changed(struct, **fields):
        c = type(struct)()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(struct), ctypes.sizeof(struct))
        for k, v in fields.items():
            setattr(c, k, v)
        return c

    invalid(src=None)
    invalid(out=None)
    for k in ("frames", "frame_offsets", "msg", "world", "flags", "free_handles"):
        invalid(src=changed(call.a, **{k: None}))
    invalid(src=changed(call.a, n_db=0xFFFFFFFF))
    invalid(src=changed(call.a, n_frames=0xFFFFFFFF))
    invalid(src=changed(call.a, max_records=abi.RECDISP_MAX_RECORDS))
    for k, cap in (("ops", "ops_capacity"), ("defer", "defer_capacity"), ("runs", "runs_capacity")):
        invalid(out=changed(call.out, **{cap: 0}))                     # an array with capacity 0
        invalid(out=changed(call.out, **{k: None, "op_ref": None} if k == "ops" else {k: None}))   # a capacity without its array
    lib = load_library()
    assert lib.wq_records_dispatch_device(None, ctypes.byref(call.a), ctypes.byref(call.out), None) == abi.WQ_E_INVALID
    closed, _ = open_router(store=False)                               # no record store is open
    invalid(r=closed)
    closed.close()
    torch.cuda.synchronize()
    for b in list(call.outs.values()) + [call.cnt]:
        assert b.unchanged()                                           # nothing was launched
    call.launch(router)
    call.check("after the refused calls")


@pytest.mark.parametrize("devices", [(0, 0)], ids=["one_device_twice"])
def test_a_multi_gpu_handle_has_no_store(devices):
    from worldql_server_amd.router import Router, WQError
    r = Router.multi(16, devices, mode="replicate")
    call = Call(shapes()["n_db_1"])
    with pytest.raises(WQError) as e:
        r.records_dispatch_device(call.a, call.out, call.cnt.ptr)
    assert e.value.code == abi.WQ_E_INVALID
    r.close()


def test_between_decode_dispatch_route_and_pack():
    """Records dispatch, decode, dispatch, a route tick, pack, records dispatch on one handle and stream, nothing
    waited for, both orders."""
    import torch
    r, _ = open_router()
    d1, o1, _ = batches()["corpus_3"]
    a, b = Call(shapes()["n_db_65"]), Call(hostile()["record_offsets_past_the_frame"], shift=0)
    dec = decode_gpu.Call(d1, o1)
    dsp = dispatch_gpu.Call(*dispatch_cases()["mix_65"][:1], **dispatch_cases()["mix_65"][1])
    p = pack_gpu.Call("tiny_runs", True)
    dev = torch.device("cuda:0")
    pos = torch.zeros(3 * 64, dtype=torch.float64, device=dev)
    world = torch.zeros(64, dtype=torch.int32, device=dev)
    sender = torch.zeros(64, dtype=torch.int32, device=dev)
    repl = torch.zeros(64, dtype=torch.uint8, device=dev)
    offs = torch.zeros(65, dtype=torch.int32, device=dev)
    peers = torch.zeros(64 * 8, dtype=torch.int32, device=dev)

    class Route:
        def launch(self, r):
            r.route_device(pos.data_ptr(), world.data_ptr(), sender.data_ptr(), repl.data_ptr(), 64, offs.data_ptr(),
                           peers.data_ptr(), None, 64 * 8, None)

    torch.cuda.synchronize()
    for order in ((a, dec, dsp, Route(), p, b), (p, b, Route(), dsp, a, dec)):
        for x in order:
            x.launch(r)
        a.check("n_db_65")
        dsp.check("mix_65")
        pack_gpu.check("tiny_runs", True, *p.outputs())
        b.check("record_offsets_past_the_frame")
        dec.outputs()
    assert r.route_health() == (0, 0)
    r.close()


# ---- from the wire to the store -----------------------------------------------------------

def ticks_of(events, sizes):
    k, i = 0, 0
    while i < len(events):
        yield events[i:i + sizes[k % len(sizes)]]
        i += sizes[k % len(sizes)]
        k += 1


def plain(replies):
    """Replies as comparable values: sender, world, and the records as a sorted list of (uuid, position, data, flex)."""
    return [(s, w, sorted((tuple(r["uuid"]), tuple(r["position"]), r["data"], r["flex"]) for r in recs)) for s, w, recs in replies]


def reference_processor(worlds=WORLDS):
    ids = WorldIds()
    for w in worlds:
        ids.intern(w)
    return records.RecordProcessor(records.RecordStoreRef(*SIZES, TABLE_SIZE), ids)


def test_frames_to_the_store_equal_the_record_processor():
    """3,000 random events, about 40% of them record instructions with 0 - 6 records a frame, 8 worlds all in
    the table, ticks of 97 and 400 frames on one handle: decode, dispatch, records dispatch and
    DeviceRecordProcessor on a GpuRecordStore against RecordProcessor.process on a RecordStoreRef."""
    from test_records_dispatch_host import wire
    events = random_events(3000, seed=21, p_record=0.4, max_records=6)
    r, store = open_router()
    dev = records.DeviceRecordProcessor(store, ingest.IngestTick(r, capacity=16), WORLDS)
    ref = reference_processor()
    n_replies = n_runs = 0
    for t, chunk in enumerate(ticks_of(events, (97, 400))):
        data, offsets = wire(chunk)
        got = dev.process(data, offsets, NOW + 1000 * t)
        want = ref.process(processor_events(chunk), NOW + 1000 * t)
        c = dev.last_counters
        assert c["n_deferred_records"] == c["n_read_deferred"] == 0 and c["first_deferred"] == len(chunk)
        assert plain(got) == plain(want), t
        n_replies += len(want)
        n_runs += c["n_runs"]
    assert n_replies > 100 and n_runs > 200 and dev.deferred == 0
    assert dev.totals() == ref.store.totals() and dev.totals()["deduped_rows"] > 0 and dev.totals()["deleted_rows"] > 0
    assert dev.totals()["rejected_queries"] > 0 and dev.totals()["rejected_ops"] == 0
    assert store.stats()[0] == ref.store.stats()[0] > 100
    assert sum(x is not None for x in dev.slab) == sum(x is not None for x in ref.slab)
    store.close()
    r.close()


def test_two_worlds_missing_from_the_table():
    """The table lacks two of the eight worlds: every read before first_deferred gets the reference's reply, the
    deferred list holds exactly the definition's pairs, the host's fallback interns the names and the next tick
    resolves them on the device."""
    from test_records_dispatch_host import wire
    table = WORLDS[:6]
    from test_records_dispatch_host import RAW_NAMES
    first = random_events(300, seed=5, p_record=0.5, max_records=4, raw_names=RAW_NAMES[:6]) + random_events(100, seed=6, p_record=0.5)
    second = random_events(300, seed=7, p_record=0.5, max_records=4)
    r, store = open_router(worlds=table)
    tick = ingest.IngestTick(r, capacity=16)
    dev = records.DeviceRecordProcessor(store, tick, table)
    data, offsets = wire(first)
    got = dev.process(data, offsets, NOW)
    out = tick.read_records_dispatch()
    want = Case(first, worlds=table, free_handles=[], handle_next=0).definition()
    same(out, want, "tick 1", fields=("cls", "ops", "op_ref", "q_src", "q_world", "q_pos", "q_after", "defer", "runs"))
    fd = want["counters"]["first_deferred"]
    assert 300 <= fd < len(first) and len(want["defer"]) > 10 and dev.deferred == len(want["defer"])
    ref = reference_processor(table)
    before = ref.process(processor_events(first[:fd]), NOW)
    assert len(before) > 5 and plain(got[:len(before)]) == plain(before)
    assert dev.names[:6] == table and sorted(dev.names[6:]) == sorted(WORLDS[6:])
    data, offsets = wire(second)
    dev.process(data, offsets, NOW + 1000)
    assert dev.last_counters["n_deferred_records"] == dev.last_counters["n_read_deferred"] == 0
    store.close()
    r.close()
