"""wq_records_vacuum / _export / _import on the GPU (csrc/wq_records.hip).

Bars: every shared script of test_records_host.py cases() with a vacuum after step k (every k on the
small scripts, every 5th step of random_stream) returns byte for byte what the reference does without
one, after every call: offsets, handles, times, counters, the drained dead list, at the end the
totals, and rows_stored == rows_live after each vacuum; the same with an export, a second store on
another handle, an import and the rest of the script there. The hand-written cases of
test_records_vacuum_host.py run against a twin RecordStoreRef that never vacuums. Output arrays are
exactly sized with canary words behind them.
"""
import ctypes

import numpy as np
import pytest

from worldql_server_amd import abi, records as R

from test_records_host import CFG, cases
from test_records_vacuum_host import CASES, creates, deletes, agree, points_of, replay, same

pytestmark = pytest.mark.gpu

CANARY = 64
P = (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def routers():
    from worldql_server_amd.router import Router
    rs = [Router(16, 0), Router(16, 0)]
    yield rs
    for r in rs:
        r.close()


class GpuStore:
    """GpuRecordStore behind the interface of test_records_vacuum_host.RefStore."""

    def __init__(self, router, cfg):
        from worldql_server_amd.router import WQError
        self.refused = WQError
        self.cfg, self.raw = tuple(cfg), R.GpuRecordStore(router, *cfg)

    def step(self, step, want_res):
        if step[0] == "apply":
            return self.raw.apply(step[1])
        _, world, pos, after, dedupe, cap = step
        cap = int(want_res["returned"]) if cap is None else cap
        got = self.raw.read(world, pos, after, dedupe=dedupe, capacity=cap, canary=CANARY)
        assert got["canaries_ok"]
        return got

    def read(self, qs, dedupe=False):
        world, pos = [q[0] for q in qs], [q[1] for q in qs]
        need = self.raw.read(world, pos, dedupe=False, capacity=0)["returned"]
        got = self.raw.read(world, pos, dedupe=dedupe, capacity=need, canary=CANARY)
        assert got["canaries_ok"] and got["returned"] == need
        return got

    def close(self):
        self.raw.close()

    def __getattr__(self, name):
        return getattr(self.raw, name)


@pytest.fixture
def open_gpu(routers):
    return lambda cfg, which=0: GpuStore(routers[which], cfg)


@pytest.mark.parametrize("form", ["vacuum", "snapshot"])
@pytest.mark.parametrize("name", sorted(cases()))
def test_invisible_in_every_shared_script(open_gpu, name, form):
    dropped = sum(replay(open_gpu, name, form, pts) for pts in points_of(name))
    if name in ("random_stream", "deletes", "duplicates", "capacity", "one_region_many_queries"):
        assert dropped > 0


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_hand_written(open_gpu, case):
    case(open_gpu)


@pytest.mark.parametrize("n,live_rows", [(1025, "every other"), (4099, "one")])
def test_block_and_word_boundaries(open_gpu, n, live_rows):
    """1,025 rows with every other one dead and 4,099 rows with one alive: the scan and the remap
    across blocks of 256 and live words of 4, the last row in a word and a block of its own."""
    dead = list(range(0, n, 2)) if live_rows == "every other" else [i for i in range(n) if i != n - 2]
    store, twin = open_gpu(CFG, 0), R.RecordStoreRef(*CFG)
    try:
        pos = [(16.0 * (i % 7) + 1.0, 1.0, 1.0) for i in range(n)]
        ops = R.make_ops(R.CREATE, 0, pos, np.arange(n) % 3, np.arange(n), 10 + np.arange(n) % 5, np.arange(n))
        kill = R.make_ops(R.DELETE, 0, [pos[i] for i in dead], np.asarray(dead) % 3, np.asarray(dead, dtype=np.uint64))
        for st in (store, twin):
            st.apply(ops)
            st.apply(kill)
        v = store.vacuum()
        assert (v["rows_before"], v["rows_after"]) == (n, n - len(dead)) and v["bytes_after"] < v["bytes_before"]
        assert store.stats() == (n - len(dead), n - len(dead), n + len(dead))
        qs = [(0, (16.0 * k + 2.0, 1.0, 1.0)) for k in range(8)]
        agree(store, twin, qs, (n, "after the vacuum"))
        for st in (store, twin):
            st.apply(ops[:300])
        agree(store, twin, qs, (n, "after an apply"), dedupe=True)
    finally:
        store.close()


def test_export_capacity_one_short_writes_nothing(routers):
    store = R.GpuRecordStore(routers[0], *CFG)
    try:
        store.apply(creates(10))
        store.apply(deletes([2, 3]))
        lib, h = routers[0].lib, routers[0].h
        n, ops = ctypes.c_size_t(), ctypes.c_uint64()
        buf = np.full(7 * 8 + CANARY, 0xA5A5A5A5A5A5A5A5, np.uint64)  # room for 7 rows of 64 bytes, then canaries
        rc = lib.wq_records_export(h, buf.ctypes.data_as(ctypes.c_void_p), 7, ctypes.byref(n), ctypes.byref(ops))
        assert rc == abi.WQ_E_CAPACITY and n.value == 8 and (buf == 0xA5A5A5A5A5A5A5A5).all()
        rc = lib.wq_records_export(h, None, 0, ctypes.byref(n), ctypes.byref(ops))
        assert rc == abi.WQ_E_CAPACITY and n.value == 8 and ops.value == 12
        buf = np.full(8 * 8 + CANARY, 0xA5A5A5A5A5A5A5A5, np.uint64)
        rc = lib.wq_records_export(h, buf.ctypes.data_as(ctypes.c_void_p), 8, ctypes.byref(n), ctypes.byref(ops))
        assert rc == 0 and n.value == 8 and (buf[64:] == 0xA5A5A5A5A5A5A5A5).all()
        rows = buf[:64].view(R.REC_ROW_DTYPE)
        assert list(rows["handle"]) == [0, 1, 4, 5, 6, 7, 8, 9] and list(rows["seq"]) == [0, 1, 4, 5, 6, 7, 8, 9]
        assert store.stats() == (8, 10, 12)  # an export does not vacuum
        same(store.drain_dead(), np.array([2, 3], np.uint32), "nor drain")
    finally:
        store.close()


def test_device_snapshot_without_a_host_copy(routers):
    """export_device into a torch buffer, import_device from it into a store on another handle; the
    device form with a capacity one short leaves the buffer alone."""
    import torch
    from worldql_server_amd.router import WQError
    s = cases()["duplicates"]
    a, twin = R.GpuRecordStore(routers[0], *s.cfg), R.RecordStoreRef(*s.cfg)
    b = None
    try:
        for st in (a, twin):
            st.apply(s.steps[0][1])
        _, world, pos, after, _, _ = s.steps[3]  # `after` one below the winners: the dedupe kills
        twin.read([(int(world[j]), pos[j], int(after[j])) for j in range(len(world))], dedupe=True)
        a.read(world, pos, after, dedupe=True, capacity=0)
        same(a.drain_dead(), twin.drain_dead(), "dead")
        live, stored, ops = a.stats()
        assert 0 < live < stored and a.export_device(0, 0) == (live, ops)
        buf = torch.full((live * 8 + CANARY,), -1, dtype=torch.int64, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        with pytest.raises(WQError) as e:
            a.export_device(buf.data_ptr(), live - 1)
        assert e.value.code == abi.WQ_E_CAPACITY and bool((buf == -1).all())
        assert a.export_device(buf.data_ptr(), live) == (live, ops)
        assert bool((buf[live * 8:] == -1).all())
        b = R.GpuRecordStore(routers[1], *s.cfg)
        assert b.import_device(buf.data_ptr(), live, ops) == {"imported": live, "rejected": 0}
        assert b.stats() == (live, live, ops)
        rows = buf[: live * 8].cpu().numpy().view(R.REC_ROW_DTYPE)
        same(rows, twin.export_rows()[0], "the snapshot")
        same(b.export_rows()[0], rows, "round trip")
        same(a.export_rows()[0], rows, "two exports, the same bytes")
        want = twin.read([(int(world[j]), pos[j], None) for j in range(len(world))], dedupe=True)
        got = b.read(world, pos, dedupe=True, capacity=want["returned"], canary=CANARY)
        for k in ("offsets", "handles", "ts_us"):
            same(got[k], want[k], k)
        assert got["canaries_ok"] and got["deduped_rows"] == want["deduped_rows"]
    finally:
        a.close()
        if b is not None:
            b.close()


def test_vacuum_gives_the_memory_back(routers):
    """At least half the rows dead: fewer bytes afterwards, rows_after == rows_live, and the same
    bytes from two exports either side of it."""
    store = R.GpuRecordStore(routers[0], *CFG)
    try:
        n = 6000
        store.apply(creates(n))
        store.apply(deletes(range(0, n, 2)))
        store.apply(deletes(range(1, n, 8)))
        live = store.stats()[0]
        assert live < n // 2
        before = store.export_rows()[0]
        same(store.export_rows()[0], before, "two exports")
        v = store.vacuum()
        assert v["rows_before"] == n and v["rows_after"] == live and v["bytes_after"] < v["bytes_before"]
        same(store.export_rows()[0], before, "the vacuum moves rows, a snapshot does not see it")
        assert len(store.drain_dead()) == n - live  # the undrained handles came along
        v = store.vacuum()
        assert v["rows_before"] == v["rows_after"] == live and v["bytes_after"] == v["bytes_before"]
    finally:
        store.close()


def test_multi_gpu_handle_refuses_all_five():
    from worldql_server_amd.router import Router
    r = Router.multi(16, (0, 0))
    try:
        n, ops = ctypes.c_size_t(), ctypes.c_uint64()
        row = np.zeros(1, R.REC_ROW_DTYPE)
        p = row.ctypes.data_as(ctypes.c_void_p)
        vres, ires = R.RecVacuumResult(), R.RecImportResult()
        assert r.lib.wq_records_vacuum(r.h, ctypes.byref(vres)) == abi.WQ_E_INVALID
        assert r.lib.wq_records_export(r.h, p, 1, ctypes.byref(n), ctypes.byref(ops)) == abi.WQ_E_INVALID
        assert r.lib.wq_records_export_device(r.h, None, 0, ctypes.byref(n), ctypes.byref(ops)) == abi.WQ_E_INVALID
        assert r.lib.wq_records_import(r.h, p, 1, 5, ctypes.byref(ires)) == abi.WQ_E_INVALID
        assert r.lib.wq_records_import_device(r.h, None, 0, 5, ctypes.byref(ires)) == abi.WQ_E_INVALID
    finally:
        r.close()
