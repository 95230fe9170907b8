"""GPU parity for the record payload slab (include/wq_router.h wq_slab_store_device, csrc/wq_slab.hip) and
records.DeviceRecordSlab.

Bars, all bit-exact against worldql_server_amd/records.py slab_store_np (the shared cases of
tests/test_slab_store_host.py):
  - entries, arena, cursor and counters are the definition's from several cursors, and the same bytes on a
    second call;
  - every device array is guarded: the slab is sized exactly with canaries before and behind it, the inputs
    are as they were, and the frame bytes sit at an odd address;
  - all or nothing on both overflows; DeviceRecordSlab's overflow-then-grow leaves the slab one large-enough
    call leaves;
  - a 1 MiB flex stored and returned;
  - from the wire: a tick's frames through decode, dispatch and records dispatch into the slab hold, handle by
    handle, the records DeviceRecordProcessor.process keeps on the host;
  - free, the dead-byte count and put_host."""
import numpy as np
import pytest

from worldql_server_amd import abi, ingest, records

from test_gpu_peer_pack import CANARY8, Bytes
from test_slab_store_host import CASES, IDS, E

pytestmark = pytest.mark.gpu

CSIZE = abi.SLAB_COUNTERS_DTYPE.itemsize


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    yield r
    r.close()


class Call:
    """One case on the device with a slab of exactly n_entries / n_bytes, canaries all around."""

    def __init__(self, case, n_entries, n_bytes, cursor, with_counters=True, shift=1):
        self.case, self.n_entries, self.n_bytes, self.cursor0 = case, n_entries, n_bytes, cursor
        ops, refs, frames, fo = case.arrays()
        u8 = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1)   # noqa: E731
        self.src = dict(ops=Bytes(u8(ops)), refs=Bytes(u8(refs)), frames=Bytes(u8(frames), shift=shift), fo=Bytes(u8(fo)))
        self.n_ops, self.n_frames = len(ops), len(fo) - 1
        self.ent, self.pay = Bytes(n=64 * n_entries), Bytes(n=n_bytes)
        self.cur = Bytes(np.array([cursor], np.uint64).view(np.uint8))
        self.cnt = Bytes(n=CSIZE) if with_counters else None
        self.view = abi.SlabView(entries=self.ent.ptr if n_entries else None, n_entries=n_entries,
                                 payload=self.pay.ptr if n_bytes else None, n_payload_bytes=n_bytes)
        ent = np.full(64 * n_entries, CANARY8, np.uint8).view(E)
        self.want = records.slab_store_np(ops, refs, frames, fo, ent, np.full(n_bytes, CANARY8, np.uint8), cursor)

    def launch(self, r):
        s = self.src
        p = lambda b: b.ptr if b.n else None   # noqa: E731
        r.slab_store_device(p(s["ops"]), p(s["refs"]), self.n_ops, p(s["frames"]), s["fo"].ptr, self.n_frames, self.view,
                            self.cur.ptr, self.cnt.ptr if self.cnt else None)

    def outputs(self):
        import torch
        torch.cuda.synchronize()
        got = []
        for b, n in ((self.ent, 64 * self.n_entries), (self.pay, self.n_bytes), (self.cur, 8)) + (((self.cnt, CSIZE),) if self.cnt else ()):
            raw = b.read()
            assert (raw[n:] == CANARY8).all() and b.front_intact(), "written outside an output"
            got.append(raw[:n].copy())
        for k, b in self.src.items():
            assert b.unchanged(), "an input was written: " + k
        return got

    def check(self, r):
        self.launch(r)
        got = self.outputs()
        w_ent, w_pay, w_cur, w_cnt = self.want
        assert got[0].tobytes() == w_ent.tobytes(), (self.case.name, "entries")
        assert np.array_equal(got[1], w_pay), (self.case.name, "payload")
        assert int(got[2].view(np.uint64)[0]) == w_cur
        if self.cnt:
            assert records.slab_counters(got[3]) == w_cnt
        return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_equals_the_definition(router, case):
    ne, nb = case.need()
    for cursor, extra in ((0, 0), (5, 0), (1019, 1500), (1024, 3)):
        c = Call(case, ne + (extra > 0), cursor + nb + extra, cursor)
        first = c.check(router)
        again = Call(case, ne + (extra > 0), cursor + nb + extra, cursor, shift=0)
        second = again.check(router)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    Call(case, ne, 7 + nb, 7, with_counters=False).check(router)


@pytest.mark.parametrize("name", ["one of each", "0..40", "1 MiB flex", "hostile references"])
def test_all_or_nothing(router, name):
    case = next(c for c in CASES if c.name == name)
    ne, nb = case.need()
    for n_entries, n_bytes in ((ne, 3 + nb - 1), (ne - 1, 3 + nb), (0, 3), (ne, 2), (ne - 1, 3 + nb - 1)):
        c = Call(case, n_entries, n_bytes, 3)
        assert c.want[3]["overflow"]
        c.check(router)


def test_validation(router):
    from worldql_server_amd.router import WQError
    case = CASES[2]
    ne, nb = case.need()
    c = Call(case, ne, nb + 16, 0)
    c.view.payload += 8
    with pytest.raises(WQError):
        c.launch(router)
    c.view.payload -= 8
    c.check(router)


def slab_after(router, chunks, **kw):
    import torch
    slab = records.DeviceRecordSlab(router, torch.device("cuda:0"), **kw)
    keep = []
    for ops, refs, frames, fo in chunks:
        t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in (ops, refs, frames, fo)]
        keep.append(t)
        torch.cuda.synchronize()
        slab.store(t[0].data_ptr(), t[1].data_ptr(), len(ops), t[2].data_ptr() if len(frames) else 0, t[3].data_ptr(), len(fo) - 1)
    return slab


def test_overflow_then_grow_equals_one_large_call(router):
    chunks = []
    base = 0
    for name in ("0..40", "one of each", "around a tile", "1 MiB flex"):
        ops, refs, frames, fo = next(c for c in CASES if c.name == name).arrays()
        ops = ops.copy()
        ops["handle"] += base
        base += len(ops)
        chunks.append((ops, refs, frames, fo))
    small = slab_after(router, chunks, n_entries=4, n_payload_bytes=64)
    large = slab_after(router, chunks, n_entries=4096, n_payload_bytes=4 << 20)
    assert small.grows >= 3 and large.grows == 0 and small.cursor == large.cursor > 1 << 20
    (e1, p1), (e2, p2) = small.read(), large.read()
    assert e1[:base].tobytes() == e2[:base].tobytes() and np.array_equal(p1, p2)
    assert not e1[base:].view(np.uint8).any()
    # and it is the definition's slab
    ent, pay, cur = np.zeros(base, E), np.zeros(large.cursor, np.uint8), 0
    for ch in chunks:
        ent, pay, cur, _ = records.slab_store_np(*ch, ent, pay, cur)
    assert e2[:base].tobytes() == ent.tobytes() and np.array_equal(p2, pay)


def test_a_1_mib_flex_stored_and_returned(router):
    case = next(c for c in CASES if c.name == "1 MiB flex")
    ops, refs, frames, fo = case.arrays()
    slab = slab_after(router, [case.arrays()], n_entries=1, n_payload_bytes=16)
    got = slab.get(1, raw_data=True)   # the case's bytes are random, not text
    a = int(fo[0])
    assert got["data"] == frames[a + 3:a + 20].tobytes()
    assert got["flex"] == frames[a + 37:a + 37 + (1 << 20)].tobytes() and len(got["flex"]) == 1 << 20
    assert got["uuid"] == (int(ops[1]["uuid_hi"]), int(ops[1]["uuid_lo"])) and got["position"] == tuple(ops[1]["pos"])


def test_free_dead_bytes_and_put_host(router):
    case = next(c for c in CASES if c.name == "one of each")
    slab = slab_after(router, [case.arrays()])
    ent, _ = slab.read()
    assert slab.dead_bytes == 0 and all(ent[h]["bits"] & abi.SLAB_LIVE for h in range(4))
    slab.free([0, 2, 2, 900000])
    slab.free([2])   # not live any more: counts nothing
    assert slab.dead_bytes == 40 + 1 and slab.get(0) is None and slab.get(2) is None and slab.get(1, raw_data=True) is not None
    rec = {"uuid": (7, 9), "position": (1.5, -2.0, 3.25), "data": "héllo", "flex": b"\x00\x01\x02"}
    at = slab.cursor
    slab.put_host(5000, rec, world=3)
    assert slab.get(5000) == dict(rec, world=3) and slab.cursor == at + 6 + 3 and slab.n_entries > 5000
    slab.put_host(0, {"uuid": (1, 2), "position": (0.0, 0.0, 0.0), "data": None, "flex": None}, world=0)
    assert slab.get(0) == {"uuid": (1, 2), "position": (0.0, 0.0, 0.0), "data": None, "flex": None, "world": 0}
    # a device store behind a host put starts at the host's cursor
    before = slab.cursor
    ops, refs, frames, fo = case.arrays()
    ops = ops.copy()
    ops["handle"] += 10
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in (ops, refs, frames, fo)]
    torch.cuda.synchronize()
    cnt = slab.store(t[0].data_ptr(), t[1].data_ptr(), len(ops), t[2].data_ptr(), t[3].data_ptr(), len(fo) - 1)
    assert cnt["bytes_need"] - cnt["bytes_stored"] == before and slab.get(5000) == dict(rec, world=3)
    assert slab.get(10, raw_data=True)["flex"] == frames[20:50].tobytes()


def test_from_the_wire_the_slab_holds_the_processors_records():
    """A tick of record frames: decode, dispatch, records dispatch, then the slab store on the device arrays; every
    created handle's entry equals the dict DeviceRecordProcessor.process slices out of the frames on the host."""
    import torch
    from test_gpu_records_dispatch import open_router
    from test_records_dispatch_host import NOW, WORLDS, random_events, wire
    events = random_events(400, seed=33, p_record=0.6, max_records=6)
    data, offsets = wire(events)
    r, store = open_router()
    host = records.DeviceRecordProcessor(store, ingest.IngestTick(r, capacity=16), WORLDS)
    host.process(data, offsets, NOW)
    r2, store2 = open_router()
    tick = ingest.IngestTick(r2, capacity=16)
    d_frames = torch.from_numpy(data.copy()).to("cuda:0")
    d_offsets = torch.from_numpy(np.asarray(offsets, np.uint64).view(np.int64).copy()).to("cuda:0")
    tick.decode(d_frames, d_offsets).dispatch()
    tick.records_dispatch(d_frames, d_offsets, NOW)
    cnt, _ = tick.read_records_ctrl()
    slab = records.DeviceRecordSlab(r2, torch.device("cuda:0"), n_entries=8, n_payload_bytes=64)
    got = tick.slab_store(d_frames, d_offsets, slab, cnt["n_creates"] + cnt["n_deletes"])
    assert got["n_creates"] == cnt["n_creates"] > 200 and got["error"] == 0 and slab.grows == 1
    ops = tick.read_records_rows("ops", 0, cnt["n_creates"] + cnt["n_deletes"])
    handles = [int(o["handle"]) for o in ops if o["kind"] == records.CREATE]
    assert sorted(handles) == list(range(len(handles)))
    # the host processor freed what its deletes and dedupes killed; a created record it still holds must be equal
    checked = 0
    for hd in handles:
        want = host.slab[hd]
        if want is None:
            continue
        g = slab.get(hd)
        assert (g["uuid"], g["position"], g["data"], g["flex"]) == (want["uuid"], want["position"], want["data"], want["flex"])
        assert WORLDS[g["world"]] == want["world_name"]
        checked += 1
    assert checked > 100
    for x in (store, store2):
        x.close()
    r.close()
    r2.close()
