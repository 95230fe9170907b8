"""The ingest dispatch's arithmetic (csrc/dispatch_ops.hpp) on the CPU, through
tests/cpp/ingest_dispatch_host_shim.hip: the classification, the granules' sums from their class ballots,
the scan operator over the blocks' sums, the ranks and the emit, in the kernels' three passes and the
grid's order — byte for byte against worldql_server_amd/ingest.py (dispatch_np), canaries behind every
output. No GPU needed (the GPU instance: tests/test_gpu_ingest_dispatch.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi, ingest

from test_ingest_dispatch_host import (GLOBAL, LOCAL, SUB, UNSUB, cases, definition, random_decoded, same, small_names,
                                       stretches)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC5
TAIL = 64

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

WIDTH = dict(cls=1, l_src=4, l_pos=24, l_world=4, l_sender=4, l_repl=1, g_src=4, g_world=4, g_sender=4, g_repl=1, ops=40,
             op_src=4, side_src=4, runs=20)
DTYPE = dict(cls=np.uint8, l_src=np.uint32, l_pos=np.float64, l_world=np.uint32, l_sender=np.uint32, l_repl=np.uint8,
             g_src=np.uint32, g_world=np.uint32, g_sender=np.uint32, g_repl=np.uint8, ops=abi.OP_DTYPE, op_src=np.uint32,
             side_src=np.uint32, runs=abi.DISPATCH_RUN_DTYPE)
COUNT = dict(cls="n_frames", l_src="n_local", l_pos="n_local", l_world="n_local", l_sender="n_local", l_repl="n_local",
             g_src="n_global", g_world="n_global", g_sender="n_global", g_repl="n_global", ops="n_op", op_src="n_op")


def rows_written(k, want, cap):
    c = want["counters"]
    if k == "side_src":
        return c["side_begin"][5]
    if k == "runs":
        return min(c["n_runs"] + 1, cap)
    return c[COUNT[k]]


def shape(k, raw, rows):
    a = raw[:rows * WIDTH[k]].copy().view(DTYPE[k])
    return a.reshape(rows, 3) if k == "l_pos" else a


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dispatch_shim") / "libdispatchshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                           "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "ingest_dispatch_host_shim.hip")])
    lib = ctypes.CDLL(out)
    lib.wq_test_ingest_dispatch_host.restype = ctypes.c_int
    lib.wq_test_ingest_dispatch_host.argtypes = [ctypes.POINTER(abi.DispatchIn), ctypes.c_uint64,
                                                 ctypes.POINTER(abi.DispatchOut), ctypes.c_void_p]
    for f in ("granule", "block", "scan_block", "sizes"):
        getattr(lib, "wq_test_dispatch_" + f).restype = ctypes.c_uint32
    return lib


def shim_call(lib, d, runs_capacity=None, last_seen=None, now=0, fields=abi.DISPATCH_OUT_ARRAYS, with_counters=True):
    """The shim on exactly sized inputs with canaries behind every output, sized by the definition's counts:
    a dict like dispatch_np's, outputs left out as None."""
    want = ingest.dispatch_np(d, runs_capacity, last_seen, now)
    n = len(d["instruction"])
    cap = want["counters"]["n_runs"] + 1 if runs_capacity is None else runs_capacity
    src = {k: np.array(d[k], copy=True) for k in ("instruction", "flags", "world", "sender", "repl", "pos")}
    seen = None if last_seen is None else np.concatenate([np.asarray(last_seen, np.uint32), np.full(16, 0xC5C5C5C5, np.uint32)])
    a = abi.DispatchIn(**{k: v.ctypes.data for k, v in src.items()}, last_seen=None if seen is None else seen.ctypes.data,
                       n_last_seen=0 if last_seen is None else len(last_seen), now=now)
    outs = {k: np.full(rows_written(k, want, cap) * WIDTH[k] + TAIL, CANARY, np.uint8) for k in fields}
    o = abi.DispatchOut(**{k: v.ctypes.data for k, v in outs.items()}, runs_capacity=cap if "runs" in fields else 0)
    cnt = np.full(168 + TAIL, CANARY, np.uint8)
    assert lib.wq_test_ingest_dispatch_host(ctypes.byref(a), n, ctypes.byref(o), cnt.ctypes.data if with_counters else None) == 0
    for k, v in src.items():
        assert v.tobytes() == np.ascontiguousarray(d[k]).tobytes(), "an input was written: " + k
    got = dict.fromkeys(abi.DISPATCH_OUT_ARRAYS)
    for k, v in outs.items():
        rows = rows_written(k, want, cap)
        assert (v[rows * WIDTH[k]:] == CANARY).all(), "written behind " + k
        got[k] = shape(k, v, rows)
    if with_counters:
        assert (cnt[168:] == CANARY).all()
        got["counters"] = ingest.dispatch_counters(cnt)
    else:
        assert (cnt == CANARY).all()
    if seen is not None:
        assert (seen[len(last_seen):] == 0xC5C5C5C5).all(), "written behind last_seen"
        got["last_seen"] = seen[:len(last_seen)]
    return got, want


def test_constants_and_layouts(shim):
    assert (shim.wq_test_dispatch_granule(), shim.wq_test_dispatch_block(), shim.wq_test_dispatch_scan_block()) == (64, 1024, 256)
    assert [shim.wq_test_dispatch_sizes(k) for k in range(4)] == [ctypes.sizeof(abi.DispatchIn), ctypes.sizeof(abi.DispatchOut),
                                                                 abi.DISPATCH_RUN_DTYPE.itemsize,
                                                                 abi.DISPATCH_COUNTERS_DTYPE.itemsize]


@pytest.mark.parametrize("name", small_names())
def test_kernel_arithmetic_matches_the_definition(shim, name):
    d, kw = cases()[name]
    got, want = shim_call(shim, d, **kw)
    same(got, want, name)
    same(want, definition(name), name)


def test_the_multi_share_scan(shim):
    """65,537 frames: 65 blocks; and 300,001 frames: 293 blocks, two blocks in most of the scan's shares."""
    d, kw = cases()["big_3_changes"]
    got, want = shim_call(shim, d, **kw)
    same(got, want, "big_3_changes")
    assert want["counters"]["n_runs"] == 4
    d = random_decoded(300_001, seed=4, p_effective=0.002)
    got, want = shim_call(shim, d)
    same(got, want, "sparse 300,001")
    assert want["counters"]["n_runs"] > 50


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sizes_with_hostile_values(shim, n):
    d = random_decoded(n, seed=100 + n, hostile=True)
    got, want = shim_call(shim, d, last_seen=np.zeros(51, np.uint32), now=0xFFFFFFFF)
    same(got, want, f"hostile {n}")


@pytest.mark.parametrize("first", [0, 1, 62, 63, 64, 65, 127, 128, 1023, 1024, 1025])
def test_a_run_that_starts_at_every_lane_of_interest(shim, first):
    """A table run, `first` frames in; then quiet frames up to the next granule and block, and the same kind
    again: one run, not two. Then a read run on the last lane before a boundary and the first behind it."""
    spec = [(LOCAL, first), (SUB, 1), ("quiet", 64 - (first + 1) % 64), ("quiet", 64), (UNSUB, 1), ("quiet", 1100), (SUB, 2),
            (GLOBAL, 1)]
    spec += [("quiet", 63 - (sum(c for _, c in spec) % 64)), (SUB, 1), (LOCAL, 1)]
    d = stretches([s for s in spec if s[1]])
    got, want = shim_call(shim, d)
    same(got, want, f"first {first}")
    kinds = want["runs"]["kind"].tolist()
    head = [abi.RUN_READ] if first else []
    assert kinds == head + [abi.RUN_TABLE, abi.RUN_READ, abi.RUN_TABLE, abi.RUN_READ, abi.RUN_END]
    assert want["runs"]["first_frame"][-3] % 64 == 63 and want["runs"]["first_frame"][-2] % 64 == 0


def test_nullable_outputs(shim):
    d, kw = cases()["mix_4097"]
    all_ = abi.DISPATCH_OUT_ARRAYS
    combos = [()] + [tuple(k for k in all_ if k != left_out) for left_out in all_] + [("runs",), ("ops", "l_pos"), ("cls",)]
    for fields in combos:
        for with_counters in (True, False):
            got, want = shim_call(shim, d, fields=fields, with_counters=with_counters, **kw)
            if "runs" not in fields:        # no run table asked for: the capacity is 0, the rows are the same
                assert not with_counters or got["counters"]["overflow"] == 1
                want = dict(want, counters=dict(want["counters"], overflow=1))
            same(got, want, str(fields), fields=fields, counters=with_counters)


def test_runs_capacity(shim):
    d, _ = cases()["capacity_n_runs"]
    for cap in (0, 1, 5, 6, 7, 100):
        got, want = shim_call(shim, d, runs_capacity=cap)
        same(got, want, f"capacity {cap}")
        assert len(got["runs"]) == min(7, cap)
