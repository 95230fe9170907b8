"""GPU parity for the slab's compaction (include/wq_router.h wq_slab_compact_device, csrc/wq_slab_compact.hip)
and records.DeviceRecordSlab's compact / export / load.

Bars, all bit-exact against worldql_server_amd/records.py slab_compact_np (the shared cases of
tests/test_slab_compact_host.py):
  - entries, arena, cursor and counters are the definition's, and the same bytes on a second call;
  - every device array is guarded: the destination is sized exactly with canaries before and behind it, the
    inputs are as they were, and the source arena sits at an odd address;
  - all or nothing on both overflows; WQ_E_INVALID for overlapping and for misaligned views;
  - a 1 MiB flex compacted and returned;
  - DeviceRecordSlab.compact() after store / free / put_host, the compact_at policy, export() then load()."""
import numpy as np
import pytest

from worldql_server_amd import abi, records

from test_gpu_peer_pack import CANARY8, Bytes
from test_slab_compact_host import CASES, IDS, E, by_name
from test_slab_store_host import CASES as STORE_CASES

pytestmark = pytest.mark.gpu

CSIZE = abi.SLAB_COMPACT_COUNTERS_DTYPE.itemsize
CURSOR0 = 0x4321


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    yield r
    r.close()


class Call:
    """One case on the device into a destination of exactly n_entries / n_bytes, canaries all around."""

    def __init__(self, case, n_entries, n_bytes, with_counters=True, shift=1):
        self.case, self.n_entries, self.n_bytes = case, n_entries, n_bytes
        self.src = dict(entries=Bytes(case.entries.view(np.uint8).reshape(-1)), payload=Bytes(case.payload, shift=shift))
        self.ent, self.pay = Bytes(n=64 * n_entries), Bytes(n=n_bytes)
        self.cur = Bytes(np.array([CURSOR0], np.uint64).view(np.uint8))
        self.cnt = Bytes(n=CSIZE) if with_counters else None
        p = lambda b: b.ptr if b.n else None   # noqa: E731
        self.sview = abi.SlabView(entries=p(self.src["entries"]), n_entries=len(case.entries), payload=p(self.src["payload"]),
                                  n_payload_bytes=len(case.payload))
        self.dview = abi.SlabView(entries=p(self.ent), n_entries=n_entries, payload=p(self.pay), n_payload_bytes=n_bytes)
        ent = np.full(64 * n_entries, CANARY8, np.uint8).view(E)
        self.want = records.slab_compact_np(case.entries, case.payload, n_entries, n_bytes,
                                            dst=(ent, np.full(n_bytes, CANARY8, np.uint8), CURSOR0))

    def launch(self, r):
        r.slab_compact_device(self.sview, self.dview, self.cur.ptr, self.cnt.ptr if self.cnt else None)

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
            assert records.slab_compact_counters(got[3]) == w_cnt
        return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_equals_the_definition(router, case):
    ne, nb = case.need()
    for n_entries, n_bytes in ((ne, nb), (len(case.entries) + 3, nb + 1500)):
        first = Call(case, n_entries, n_bytes).check(router)
        second = Call(case, n_entries, n_bytes, shift=0).check(router)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    Call(case, ne, nb, with_counters=False).check(router)


@pytest.mark.parametrize("name", ["65 entries", "0..40", "two 1 MiB payloads", "hostile ranges", "runs of 65 dead"])
def test_all_or_nothing(router, name):
    case = by_name(name)
    ne, nb = case.need()
    for n_entries, n_bytes in ((ne, nb - 1), (ne - 1, nb), (0, 0), (ne, 0), (ne - 1, nb - 1), (ne + 5, nb // 2)):
        c = Call(case, n_entries, n_bytes)
        assert c.want[3]["overflow"] and c.want[2] == CURSOR0
        c.check(router)


def test_validation(router):
    from worldql_server_amd.router import WQError
    case = by_name("65 entries")
    ne, nb = case.need()

    def refused(edit):
        c = Call(case, ne, nb + 32)
        edit(c)
        with pytest.raises(WQError):
            c.launch(router)
        assert c.outputs()[0].tobytes() == bytes([CANARY8]) * (64 * ne)   # nothing launched

    def set_(view, **kw):
        for k, v in kw.items():
            setattr(view, k, v)

    # misaligned: the destination's arena, either entry array (the source arena may sit anywhere)
    refused(lambda c: set_(c.dview, payload=c.dview.payload + 8))
    refused(lambda c: set_(c.dview, entries=c.dview.entries + 8))
    refused(lambda c: set_(c.sview, entries=c.sview.entries + 4))
    # overlapping: entries on entries, arena on arena, by one element
    refused(lambda c: set_(c.dview, entries=c.sview.entries + 64 * (len(case.entries) - 1), n_entries=1))
    refused(lambda c: set_(c.dview, entries=c.sview.entries, n_entries=len(case.entries)))
    refused(lambda c: set_(c.sview, payload=c.dview.payload + 16, n_payload_bytes=16))
    # null with a size, too many entries
    refused(lambda c: set_(c.dview, payload=None))
    refused(lambda c: set_(c.sview, n_entries=0xFFFFFFFF))
    with pytest.raises(WQError):
        c = Call(case, ne, nb)
        router.slab_compact_device(c.sview, c.dview, None, None)
    Call(case, ne, nb + 32).check(router)


def slab_after(router, chunks, **kw):
    import torch
    slab = records.DeviceRecordSlab(router, torch.device("cuda:0"), **kw)
    for ops, refs, frames, fo in chunks:
        t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in (ops, refs, frames, fo)]
        torch.cuda.synchronize()
        slab.store(t[0].data_ptr(), t[1].data_ptr(), len(ops), t[2].data_ptr() if len(frames) else 0, t[3].data_ptr(), len(fo) - 1)
    return slab


def store_chunks(names):
    chunks, base = [], 0
    for name in names:
        ops, refs, frames, fo = next(c for c in STORE_CASES if c.name == name).arrays()
        ops = ops.copy()
        ops["handle"] += base
        base += len(ops)
        chunks.append((ops, refs, frames, fo))
    return chunks, base


def test_a_1_mib_flex_compacted_and_returned(router):
    chunks, _ = store_chunks(["0..40", "1 MiB flex"])
    slab = slab_after(router, chunks)
    before = slab.get(42, raw_data=True)
    assert len(before["flex"]) == 1 << 20
    slab.free(list(range(0, 41)))
    got = slab.compact()
    assert got["reclaimed"] == sum(range(41)) and got["n_live"] == 3 and slab.cursor == 80 + 17 + (1 << 20) + 5
    assert slab.get(42, raw_data=True) == before and slab.get(7) is None


def test_compact_after_store_free_and_put_host(router):
    chunks, base = store_chunks(["0..40", "one of each", "around a tile"])
    slab = slab_after(router, chunks, n_entries=8, n_payload_bytes=64)
    rec = {"uuid": (7, 9), "position": (1.5, -2.0, 3.25), "data": "héllo", "flex": b"\x00\x01\x02"}
    slab.put_host(base + 2, rec, world=3)
    slab.free([1, 2, 5, 40, 41, base - 1, 900000])
    dead = slab.dead_bytes
    assert dead > 1000
    ent, pay = slab.read()
    cursor = slab.cursor
    got = slab.compact()
    want = records.slab_compact_np(ent, pay, slab.n_entries, slab.n_payload_bytes)
    e2, p2 = slab.read()
    assert e2.tobytes() == want[0].tobytes() and np.array_equal(p2, want[1][:want[2]])
    assert {k: got[k] for k in want[3]} == want[3] and got["reclaimed"] == dead == cursor - slab.cursor
    assert slab.dead_bytes == 0 and slab.cursor == want[2] and slab.compactions == 1
    assert slab.get(base + 2) == dict(rec, world=3) and slab.get(2) is None
    # a store behind the compaction lands at the new cursor
    ops, refs, frames, fo = next(c for c in STORE_CASES if c.name == "one of each").arrays()
    ops = ops.copy()
    ops["handle"] += base + 10
    at = slab.cursor
    cnt = slab_store(slab, (ops, refs, frames, fo))
    assert cnt["bytes_need"] - cnt["bytes_stored"] == at and slab.read()[0][base + 10]["off"] == at
    assert slab.get(base + 10, raw_data=True)["flex"] == frames[20:50].tobytes()


def slab_store(slab, chunk):
    import torch
    ops, refs, frames, fo = chunk
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in (ops, refs, frames, fo)]
    torch.cuda.synchronize()
    return slab.store(t[0].data_ptr(), t[1].data_ptr(), len(ops), t[2].data_ptr(), t[3].data_ptr(), len(fo) - 1)


def test_compact_at_triggers_where_it_should_and_nowhere_else(router):
    chunks, base = store_chunks(["0..40"])          # handle k holds k bytes: 820 in all
    never = slab_after(router, chunks)
    never.free(list(range(41)))
    assert never.compactions == 0 and never.dead_bytes == 820 == never.cursor
    slab = slab_after(router, chunks, compact_at=0.5)
    slab.free([40, 39, 38, 37, 36, 35, 34, 33, 32, 31])   # 355 of 820: below a half
    assert slab.compactions == 0 and slab.dead_bytes == 355 and slab.cursor == 820
    slab.free([30, 29])                                   # 414 >= 410
    assert slab.compactions == 1 and slab.dead_bytes == 0 and slab.cursor == 820 - 414
    slab.free([30])                                       # dead already: nothing
    assert slab.compactions == 1
    # a store that overflows grows by compacting: the dead bytes are not carried along
    small = slab_after(router, chunks, n_entries=64, n_payload_bytes=1024, compact_at=0.9)
    small.free(list(range(21, 41)))                       # 610 of 820 dead: below 0.9
    assert small.compactions == 0 and small.grows == 0
    ops, refs, frames, fo = next(c for c in STORE_CASES if c.name == "0..40").arrays()
    ops = ops.copy()
    ops["handle"] += 41
    cnt = slab_store(small, (ops, refs, frames, fo))      # 820 + 820 > 1024
    assert small.compactions == 1 and small.grows == 1 and cnt["overflow"] == 0
    assert small.cursor == 210 + 820 and small.dead_bytes == 0 and small.read()[0][41 + 5]["off"] == 210 + 10
    plain = slab_after(router, chunks, n_entries=64, n_payload_bytes=1024)
    plain.free(list(range(21, 41)))
    slab_store(plain, (ops, refs, frames, fo))
    assert plain.cursor == 820 + 820 and plain.compactions == 0 and plain.grows == 1
    assert plain.export()[0].tobytes() == small.export()[0].tobytes() and np.array_equal(plain.export()[1], small.export()[1])


def test_export_then_load_gives_equal_reads(router):
    import torch
    chunks, base = store_chunks(["0..40", "one of each", "around a tile"])
    slab = slab_after(router, chunks)
    slab.free([0, 3, 4, 44, base - 1])
    before = slab.read()
    ent, pay = slab.export()
    after = slab.read()
    assert before[0].tobytes() == after[0].tobytes() and np.array_equal(before[1], after[1])   # export leaves the slab alone
    want = records.slab_compact_np(before[0], before[1], 0, 0)[3]
    assert len(ent) == want["entries_need"] == base - 1 and len(pay) == want["bytes_live"]
    full = records.slab_compact_np(before[0], before[1], len(ent), len(pay))
    assert ent.tobytes() == full[0].tobytes() and np.array_equal(pay, full[1])
    other = records.DeviceRecordSlab(router, torch.device("cuda:0"), n_entries=4, n_payload_bytes=16)
    cnt = other.load(ent, pay)
    assert cnt["error"] == 0 and cnt["n_live"] == want["n_live"] and other.cursor == len(pay)
    slab.compact()
    (e1, p1), (e2, p2) = slab.read(), other.read()
    n = len(ent)
    assert e1[:n].tobytes() == e2[:n].tobytes() and np.array_equal(p1, p2) and not e1[n:].view(np.uint8).any() and not e2[n:].view(np.uint8).any()
    for h in (1, 2, 41, 43, base - 2):
        assert other.get(h, raw_data=True) == slab.get(h, raw_data=True) is not None
    # a load validates: a range that leaves the file comes out live and empty, and is reported
    bad = ent.copy()
    bad["off"][2] = len(pay) - 1
    cnt = records.DeviceRecordSlab(router, torch.device("cuda:0")).load(bad, pay)
    assert cnt["error"] == abi.SLAB_COMPACT_ERROR_RANGE and cnt["bytes_live"] == len(pay) - 2
    empty = records.DeviceRecordSlab(router, torch.device("cuda:0"))
    assert [len(a) for a in empty.export()] == [0, 0] and empty.load(*empty.export())["n_live"] == 0
