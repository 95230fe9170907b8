"""The record store on the GPU (wq_records_*, csrc/wq_records.hip).

Bars: after every call of every shared script (test_records_host.py cases()) the offsets, handles,
times, result counters, the drained dead list and wq_records_stats are byte-identical to
RecordStoreRef; output arrays are exactly sized and the canary words behind them stay intact; the
scripts' rejected counts are the expected ones (0 everywhere but the rejection scripts, so a store
that rejects everything cannot pass).
"""
import ctypes

import numpy as np
import pytest

from worldql_server_amd import abi, records as R, synth

from test_records_host import CFG, cases, edge_coords, region_kats, too_large_read, wants

pytestmark = pytest.mark.gpu

CANARY = 64


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    yield r
    r.close()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


def check_step(store, step, want, what):
    """Runs one script step on the GPU store and compares everything with the reference's result."""
    w_res, w_dead, w_stats = want
    if step[0] == "apply":
        got = store.apply(step[1])
        assert got == {k: int(v) for k, v in w_res.items()}, what
    else:
        _, world, pos, after, dedupe, cap = step
        cap = int(w_res["returned"]) if cap is None else cap
        got = store.read(world, pos, after, dedupe=dedupe, capacity=cap, canary=CANARY)
        assert got["canaries_ok"], what
        for k in ("returned", "deduped_rows", "rejected", "scanned", "overflow", "error"):
            assert got[k] == int(w_res[k]), (what, k, got[k], int(w_res[k]))
        _same(got["offsets"], w_res["offsets"], (what, "offsets"))
        _same(got["handles"], w_res["handles"], (what, "handles"))
        _same(got["ts_us"], w_res["ts_us"], (what, "ts_us"))
    _same(store.drain_dead(), w_dead, (what, "dead list"))
    assert store.stats() == tuple(int(v) for v in w_stats), (what, "stats")
    return got


@pytest.mark.parametrize("name", sorted(cases()))
def test_scripts_match_the_reference_after_every_call(router, name):
    s = cases()[name]
    res, ref = wants()[name]
    store = R.GpuRecordStore(router, *s.cfg)
    try:
        rejected = 0
        for i, (step, want) in enumerate(zip(s.steps, res)):
            rejected += check_step(store, step, want, (name, i, step[0]))["rejected"]
        assert rejected == s.rejected
        t = store.totals()
        assert t == ref.totals() and t["rejected_ops"] + t["rejected_queries"] == s.rejected
        if name == "random_stream":  # the case is not vacuous: the store computed these itself
            assert t["rejected_ops"] == 0 and t["deduped_rows"] >= 1000 and ref.deduped_cross >= 100
            assert t["created"] + t["deleted_rows"] > 18_000 and store.stats()[2] == 20_000
        if name == "one_region_many_queries":
            assert t["deduped_rows"] == 100
    finally:
        store.close()


def test_a_call_past_the_element_limit_is_refused_whole(router):
    ops, world, pos = too_large_read()
    store = R.GpuRecordStore(router, *CFG)
    try:
        store.apply(ops)
        with pytest.raises(R.ReadTooLarge):
            store.read(world, pos, dedupe=True, capacity=0)
        assert store.stats() == (20_000, 20_000, 20_000) and len(store.drain_dead()) == 0
        out = store.read(world[:2], pos[:2], capacity=40_000, canary=CANARY)
        assert out["returned"] == 40_000 and list(out["offsets"]) == [0, 20_000, 40_000] and out["canaries_ok"]
    finally:
        store.close()


def test_processor_on_the_gpu_store_equals_the_reference(router):
    """RecordProcessor over GpuRecordStore gives the replies it gives over RecordStoreRef: reads of
    one batch see one snapshot, a region asked several times included, and freed slots agree."""
    rec = lambda u, pos, data: {"uuid": (0, u), "world_name": "w", "position": pos, "data": data, "flex": None}
    ev = lambda ins, records=(), position=None, parameter=None: {
        "instruction": ins, "world_name": "w", "sender_uuid": b"s" * 16, "parameter": parameter, "position": position,
        "records": list(records)}
    A, B = (3.0, 0.0, 0.0), (19.0, 0.0, 0.0)
    ticks = [
        [ev("RecordCreate", [rec(u, A, f"a{u}") for u in range(40)] + [rec(1, B, "b1"), rec(2, (float("nan"), 0, 0), "x")])],
        [ev("RecordRead", position=A)] * 3 + [ev("RecordRead", position=B), ev("RecordRead", position=A, parameter="0")],
        [ev("RecordCreate", [rec(1, B, "b1 newer"), rec(3, A, "a3 newer")]), ev("RecordRead", position=B),
         ev("RecordRead", position=A), ev("RecordDelete", [rec(5, A, None)]), ev("RecordRead", position=A)],
    ]
    store = R.GpuRecordStore(router, *CFG)
    try:
        gpu, ref = R.RecordProcessor(store), R.RecordProcessor(R.RecordStoreRef(*CFG))
        for i, tick in enumerate(ticks):
            a = gpu.process(tick, now_us=1_000_000 * (i + 1))
            b = ref.process(tick, now_us=1_000_000 * (i + 1))
            assert [(s, w, [r["data"] for r in rs]) for s, w, rs in a] == \
                   [(s, w, [r["data"] for r in rs]) for s, w, rs in b], i
            assert (len(a) > 0) == (i > 0) and sorted(gpu.free) == sorted(ref.free) and gpu.dropped == ref.dropped
            assert store.stats() == ref.store.stats()
        # the snapshot: in the last tick's first batch A's stale copy of uuid 1 is still returned, and dies after
        assert any(r["data"] == "a1" for _, _, rs in [b[1]] for r in rs) and ref.store.totals()["deduped_rows"] >= 2
    finally:
        store.close()


def test_quantisers_host_entry_points(router):
    kat = region_kats()
    for c, size, want in kat["clamp_region_coord"]["cases"]:
        assert int(R.region_quantize(router.lib, [c], size)[0]) == want
    for c, t, want in kat["clamp_table_size"]["cases"]:
        assert int(R.table_quantize(router.lib, [c], t)[0]) == want
    for size in (16, 256, 1, 65535):
        coords = list(edge_coords(size))
        _same(R.region_quantize(router.lib, coords, size), R.region_coord_np(coords, size), size)
    with pytest.raises(ValueError):
        R.region_quantize(router.lib, [1.0, float("nan")], 16)
    reg = np.array([0, 1, -1, 1024, -1024, -1025, 1800, 5 * 1024 + 3, -5 * 1024 - 3, 1 << 40, -(1 << 40) + 5], np.int64)
    _same(R.table_quantize(router.lib, reg, 1024), R.table_coord_np(reg, 1024), "table")


def test_same_bytes_twice(router):
    """Placement comes from prefix sums alone: the same read twice gives the same bytes."""
    s = cases()["region_sizes"]
    store = R.GpuRecordStore(router, *s.cfg)
    try:
        store.apply(s.steps[0][1])
        _, world, pos, after, _, _ = s.steps[1]
        a = store.read(world, pos, after, capacity=6000)
        b = store.read(world, pos, after, capacity=6000)
        assert a["returned"] == b["returned"] == 1 + 63 + 64 + 65 + 2 * 257 + 5000 and a["rejected"] == 0
        for k in ("offsets", "handles", "ts_us"):
            _same(a[k], b[k], k)
    finally:
        store.close()


def test_device_entry_points(router):
    """wq_records_apply_device / wq_records_read_device on torch tensors: the same bytes as the
    host-array calls (compared through the reference, which those are compared with above)."""
    import torch
    s = cases()["duplicates"]
    ref = R.RecordStoreRef(*s.cfg)
    store = R.GpuRecordStore(router, *s.cfg)
    dev = torch.device("cuda", 0)
    to_dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)
    try:
        for i, step in enumerate(s.steps):
            if step[0] == "apply":
                want = ref.apply(step[1])
                ops = to_dev(step[1].view(np.uint8), np.uint8)
                torch.cuda.synchronize()
                store.apply_device(ops.data_ptr(), len(step[1]))
                assert store.stats() == ref.stats() and want["rejected"] == 0
                assert store.totals() == ref.totals()  # the asynchronous apply's counts are not lost
                continue
            _, world, pos, after, dedupe, _ = step
            n = len(world)
            want = ref.read([(int(world[j]), pos[j], None if after is None else int(after[j])) for j in range(n)],
                            dedupe=dedupe)
            cap = want["returned"]
            d_world, d_pos = to_dev(world, np.int32), to_dev(pos, np.float64)
            d_after = None if after is None else to_dev(after, np.int64)
            off = torch.full((n + 1 + CANARY,), -1, dtype=torch.int32, device=dev)
            hd = torch.full((cap + CANARY,), -1, dtype=torch.int32, device=dev)
            ts = torch.full((cap + CANARY,), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            got = store.read_device(n, d_world.data_ptr(), d_pos.data_ptr(), None if d_after is None else d_after.data_ptr(),
                                    dedupe, off.data_ptr(), hd.data_ptr(), ts.data_ptr(), cap)
            torch.cuda.synchronize()
            for k in ("returned", "deduped_rows", "rejected", "scanned", "overflow", "error"):
                assert got[k] == int(want[k]), (i, k)
            assert got["rejected"] == 0
            off_h, hd_h, ts_h = off.cpu().numpy(), hd.cpu().numpy(), ts.cpu().numpy()
            _same(off_h[: n + 1].view(np.uint32), want["offsets"], (i, "offsets"))
            _same(hd_h[:cap].view(np.uint32), want["handles"], (i, "handles"))
            _same(ts_h[:cap], want["ts_us"], (i, "ts_us"))
            assert (off_h[n + 1:] == -1).all() and (hd_h[cap:] == -1).all() and (ts_h[cap:] == -1).all(), (i, "canaries")
            _same(store.drain_dead(), ref.drain_dead(), (i, "dead"))
            assert store.stats() == ref.stats()
    finally:
        store.close()


def test_errors_and_limits(router):
    from worldql_server_amd.router import WQError
    for bad in ((0, 16, 16, 1024), (16, 16, 16, 0), (16, 48, 16, 1024)):
        with pytest.raises(WQError) as e:
            R.GpuRecordStore(router, *bad)
        assert e.value.code == abi.WQ_E_INVALID
    res = R.RecReadResult()
    off = np.zeros(1, np.uint32)
    rc = router.lib.wq_records_read(router.h, 0, None, None, None, 0, off.ctypes.data_as(ctypes.c_void_p), None, None, 0,
                                    ctypes.byref(res))
    assert rc == abi.WQ_E_INVALID  # no store open
    store = R.GpuRecordStore(router, *CFG)
    try:
        with pytest.raises(WQError):
            R.GpuRecordStore(router, *CFG)  # one store per handle
        assert store.stats() == (0, 0, 0) and len(store.drain_dead()) == 0
        out = store.read(np.zeros(2, np.uint32), np.zeros((2, 3)), capacity=0, canary=CANARY)
        assert list(out["offsets"]) == [0, 0, 0] and out["returned"] == 0 and out["canaries_ok"]
        # the dead list is not drained into an array that is too small
        store.apply(R.make_ops([R.CREATE, R.CREATE, R.DELETE], 0, [(1.0, 1.0, 1.0)] * 3, 0, 5, 1, [3, 4, 0]))
        n = ctypes.c_size_t()
        one = np.zeros(1, np.uint32)
        rc = router.lib.wq_records_drain_dead(router.h, one.ctypes.data_as(ctypes.c_void_p), 1, ctypes.byref(n))
        assert rc == abi.WQ_E_CAPACITY and n.value == 2
        assert list(store.drain_dead()) == [3, 4] and len(store.drain_dead()) == 0
    finally:
        store.close()


def test_multi_gpu_handle_has_no_store():
    from worldql_server_amd.router import Router, WQError
    r = Router.multi(16, (0, 0))  # the devices of a multi-GPU handle may repeat
    try:
        with pytest.raises(WQError) as e:
            R.GpuRecordStore(r, *CFG)
        assert e.value.code == abi.WQ_E_INVALID
    finally:
        r.close()


def test_router_is_unchanged_by_an_open_store():
    """A handle with a record store open routes a tick exactly like one without."""
    from worldql_server_amd.router import Router
    w = synth.config_c2(repl_mode="mixed", scale=0.005)
    plain, with_store = Router(w.cube_size, 0), Router(w.cube_size, 0)
    try:
        store = R.GpuRecordStore(with_store, *CFG)
        store.apply(cases()["deletes"].steps[0][1])
        for r in (plain, with_store):
            r.apply_ops(w.ops)
        a = plain.route(w.pos, w.world, w.sender, w.repl)
        b = with_store.route(w.pos, w.world, w.sender, w.repl)
        _same(a[0], b[0], "offsets")
        _same(a[1], b[1], "peers")
        assert len(a[1]) > 0 and plain.stats() == with_store.stats()
        out = store.read([0], [(5.0, 5.0, 5.0)], capacity=16)
        assert out["returned"] > 0 and out["rejected"] == 0
        store.close()
    finally:
        plain.close()
        with_store.close()
