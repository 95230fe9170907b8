"""csrc/record_ops.hpp on the CPU (tests/cpp/records_host_shim.hip: the header's functions in the
rows / flag / scan / emit shape of wq_records.hip) against RecordStoreRef, byte for byte, on the
shared scripts of test_records_host.py. Needs hipcc only, no GPU. Every output array is followed by
canary words that must survive the call.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import records as R

from test_records_host import CFG, cases, edge_coords, region_kats, too_large_read, wants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 16
MARK32, MARK64 = 0xA5A5A5A5, -0x5A5A5A5A5A5A5A5B

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("records_shim") / "librecordsshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-o", out, os.path.join(ROOT, "tests", "cpp", "records_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp, sz, u32, u16 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint16
    lib.wq_test_rec_open.restype, lib.wq_test_rec_open.argtypes = vp, [u16, u16, u16, u32]
    lib.wq_test_rec_close.restype, lib.wq_test_rec_close.argtypes = None, [vp]
    lib.wq_test_rec_apply.restype, lib.wq_test_rec_apply.argtypes = None, [vp, vp, sz, vp]
    lib.wq_test_rec_read.restype, lib.wq_test_rec_read.argtypes = ctypes.c_int, [vp, sz, vp, vp, vp, u32, vp, vp, vp, sz, vp]
    lib.wq_test_rec_drain.restype, lib.wq_test_rec_drain.argtypes = sz, [vp, vp, sz]
    lib.wq_test_rec_stats.restype, lib.wq_test_rec_stats.argtypes = None, [vp, vp]
    lib.wq_test_rec_quantize.restype, lib.wq_test_rec_quantize.argtypes = None, [vp, sz, u16, vp, u32, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


def shim_step(lib, st, step, want, what):
    w_res, w_dead, w_stats = want
    rejected = 0
    if step[0] == "apply":
        ops = np.ascontiguousarray(step[1])
        res = R.RecApplyResult()
        lib.wq_test_rec_apply(st, _p(ops), len(ops), ctypes.byref(res))
        got = {"created": res.created, "deleted_rows": res.deleted_rows, "rejected": res.rejected,
               "rows_live": res.rows_live}
        assert got == {k: int(v) for k, v in w_res.items()}, what
        rejected = res.rejected
    else:
        _, world, pos, after, dedupe, cap = step
        n = len(world)
        cap = int(w_res["returned"]) if cap is None else cap
        off = np.full(n + 1 + CANARY, MARK32, np.uint32)
        hd = np.full(cap + CANARY, MARK32, np.uint32)
        ts = np.full(cap + CANARY, MARK64, np.int64)
        res = R.RecReadResult()
        rc = lib.wq_test_rec_read(st, n, _p(world), _p(pos), None if after is None else _p(after), int(dedupe), _p(off),
                                  _p(hd), _p(ts), cap, ctypes.byref(res))
        assert rc == 0, what
        for k in ("returned", "deduped_rows", "rejected", "scanned", "overflow", "error"):
            assert getattr(res, k) == int(w_res[k]), (what, k)
        k = min(cap, int(res.returned))
        _same(off[: n + 1], w_res["offsets"], (what, "offsets"))
        _same(hd[:k], w_res["handles"], (what, "handles"))
        _same(ts[:k], w_res["ts_us"], (what, "ts_us"))
        assert (off[n + 1:] == MARK32).all() and (hd[k:] == MARK32).all() and (ts[k:] == MARK64).all(), (what, "canaries")
        rejected = res.rejected
    dead = np.full(len(w_dead) + CANARY, MARK32, np.uint32)
    assert lib.wq_test_rec_drain(st, _p(dead), len(w_dead)) == len(w_dead), (what, "dead count")
    _same(dead[: len(w_dead)], w_dead, (what, "dead list"))
    assert (dead[len(w_dead):] == MARK32).all()
    stats = np.zeros(3, np.uint64)
    lib.wq_test_rec_stats(st, _p(stats))
    assert tuple(int(v) for v in stats) == tuple(int(v) for v in w_stats), (what, "stats")
    return rejected


@pytest.mark.parametrize("name", sorted(cases()))
def test_kernel_arithmetic_matches_the_reference(shim, name):
    s = cases()[name]
    res, _ = wants()[name]
    st = shim.wq_test_rec_open(*s.cfg)
    try:
        rejected = sum(shim_step(shim, st, step, want, (name, i, step[0]))
                       for i, (step, want) in enumerate(zip(s.steps, res)))
        assert rejected == s.rejected
    finally:
        shim.wq_test_rec_close(st)


def test_a_call_past_the_element_limit_is_refused_whole(shim):
    ops, world, pos = too_large_read()
    st = shim.wq_test_rec_open(*CFG)
    try:
        res = R.RecApplyResult()
        shim.wq_test_rec_apply(st, _p(ops), len(ops), ctypes.byref(res))
        n = len(world)
        off, rr = np.zeros(n + 1, np.uint32), R.RecReadResult()
        rc = shim.wq_test_rec_read(st, n, _p(world), _p(pos), None, 1, _p(off), None, None, 0, ctypes.byref(rr))
        assert rc == -5  # WQ_E_CAPACITY
        stats = np.zeros(3, np.uint64)
        shim.wq_test_rec_stats(st, _p(stats))
        assert list(stats) == [20_000, 20_000, 20_000] and shim.wq_test_rec_drain(st, None, 0) == 0
        rc = shim.wq_test_rec_read(st, 2, _p(world), _p(pos), None, 0, _p(off), None, None, 0, ctypes.byref(rr))
        assert rc == 0 and rr.returned == 40_000 and rr.overflow == 1 and list(off[:3]) == [0, 20_000, 40_000]
    finally:
        shim.wq_test_rec_close(st)


def test_quantisers(shim):
    kat = region_kats()

    def both(coords, size, table):
        c = np.ascontiguousarray(coords, dtype=np.float64)
        reg, tab = np.zeros(len(c), np.int64), np.zeros(len(c), np.int64)
        shim.wq_test_rec_quantize(_p(c), len(c), size, _p(reg), table, _p(tab))
        return reg, tab
    for c, size, want in kat["clamp_region_coord"]["cases"]:
        assert int(both([c], size, 1024)[0][0]) == want
    for size in (16, 256, 1, 65535):
        coords = [c for c in edge_coords(size) if abs(c) < 2.0 ** 61]
        reg, tab = both(coords, size, 1024 * 15 * 17 * 257 if size == 65535 else 1024)
        _same(reg, R.region_coord_np(coords, size), size)
        _same(tab, R.table_coord_np(reg, 1024 * 15 * 17 * 257 if size == 65535 else 1024), size)
    sizes = kat["table_bounds"]["region_sizes"]
    for pos, bx, by, bz in kat["table_bounds"]["cases"]:
        got = [int(both([c], s, 1024)[1][0]) for c, s in zip(pos, sizes)]
        assert got == [bx[0], by[0], bz[0]], pos
