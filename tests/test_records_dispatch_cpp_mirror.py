"""The record dispatch's arithmetic (csrc/recdispatch_ops.hpp) on the CPU, through
tests/cpp/records_dispatch_host_shim.hip: the frame rules, the record walk, the granules' flag words, the
scans' terms and the emit, in the kernels' passes and the grid's order — byte for byte against
worldql_server_amd/ingest.py (records_dispatch_np), canaries behind every output. No GPU needed (the GPU
instance: tests/test_gpu_records_dispatch.py)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi, frames, ingest, records

from test_records_dispatch_host import (ARRAYS, NOW, P, READ_PARAMS, SIZES, TABLE_SIZE, Case, ev, hostile, named, random_events,
                                        rec, same)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC5
TAIL = 64
CSIZE = abi.RECDISP_COUNTERS_DTYPE.itemsize

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

WIDTH = dict(cls=1, ops=64, op_ref=32, q_src=4, q_world=4, q_pos=24, q_after=8, defer=8, runs=16)
DTYPE = dict(cls=np.uint8, ops=records.REC_OP_DTYPE, op_ref=abi.REC_OP_REF_DTYPE, q_src=np.uint32, q_world=np.uint32,
             q_pos=np.float64, q_after=np.int64, defer=abi.RECDISP_DEFER_DTYPE, runs=abi.RECDISP_RUN_DTYPE)


class ShimEnv(ctypes.Structure):  # struct wq_test_recdisp_env
    _fields_ = [("world_bytes", ctypes.c_void_p), ("world_off", ctypes.c_void_p), ("n_worlds", ctypes.c_uint32),
                ("size", ctypes.c_uint16 * 3), ("pad_", ctypes.c_uint16), ("table_size", ctypes.c_uint32),
                ("n_waves", ctypes.c_uint32), ("scan_block", ctypes.c_uint32)]


def rows_written(k, want):
    """Rows of output k the call writes: the definition's arrays are already cut at the capacities."""
    return len(want[k])


def shape(k, raw, rows):
    a = raw[:rows * WIDTH[k]].copy().view(DTYPE[k])
    return a.reshape(rows, 3) if k == "q_pos" else a


def capacities(want, fields, over):
    """(ops, defer, runs) capacities of a call: what the test asks for, else what holds everything."""
    c = want["counters"]
    full = dict(ops_capacity=c["n_creates"] + c["n_deletes"], defer_capacity=c["n_deferred_records"] + c["n_read_deferred"],
                runs_capacity=c["n_runs"] + 1)
    caps = {k: over.get(k) if over.get(k) is not None else v for k, v in full.items()}
    if "ops" not in fields and "op_ref" not in fields:
        caps["ops_capacity"] = 0
    if "defer" not in fields:
        caps["defer_capacity"] = 0
    if "runs" not in fields:
        caps["runs_capacity"] = 0
    return caps


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("recdisp_shim") / "librecdispshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                           "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "records_dispatch_host_shim.hip")])
    lib = ctypes.CDLL(out)
    lib.wq_test_records_dispatch_host.restype = ctypes.c_int
    lib.wq_test_records_dispatch_host.argtypes = [ctypes.POINTER(abi.RecDispatchIn), ctypes.POINTER(ShimEnv),
                                                  ctypes.POINTER(abi.RecDispatchOut), ctypes.c_void_p]
    lib.wq_test_parse_after.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64)]
    for f in ("granule", "sizes"):
        getattr(lib, "wq_test_recdisp_" + f).restype = ctypes.c_uint32
    return lib


def shim_call(lib, case, fields=ARRAYS, with_counters=True, n_waves=0, scan_block=0, **over):
    """The shim on exactly sized inputs with canaries behind every output, sized by the definition's counts: (a
    dict like records_dispatch_np's, outputs left out as None; the definition's)."""
    probe = case.definition(**{k: v for k, v in over.items() if k in ("max_records", "free_handles", "handle_next")})
    caps = capacities(probe, fields, over)
    want = case.definition(**dict(over, **caps))
    kw = dict(case.kw, **over)
    n = len(case.offsets) - 1
    src = dict(frames=np.array(case.data, copy=True), frame_offsets=np.array(case.offsets, np.uint64),
               msg=np.array(case.decoded["msg"], copy=True), world=np.array(case.decoded["world"], np.uint32),
               flags=np.array(case.decoded["flags"], np.uint8))
    if case.db_src is not None:
        src["db_src"] = np.array(case.db_src, np.uint32)
    free = np.array(kw["free_handles"] if kw["free_handles"] is not None else [], np.uint32)
    src["free_handles"] = free
    before = {k: v.tobytes() for k, v in src.items()}
    ptr = lambda a: a.ctypes.data if len(a) else None  # noqa: E731
    total = probe["counters"]["n_records_total"]
    max_records = kw.get("max_records")
    a = abi.RecDispatchIn(frames=ptr(src["frames"]), frame_offsets=src["frame_offsets"].ctypes.data, n_frames=n,
                          n_frame_bytes=len(src["frames"]), msg=ptr(src["msg"]), world=ptr(src["world"]), flags=ptr(src["flags"]),
                          db_src=src["db_src"].ctypes.data if "db_src" in src and len(src["db_src"]) else None, n_db=case.n_db,
                          now_us=kw["now_us"], free_handles=ptr(free), n_free=len(free), handle_next=kw["handle_next"],
                          max_records=total if max_records is None else max_records)
    if case.db_src is not None and not len(case.db_src):
        a.n_db = 0
    wb, wo = frames.world_table(case.worlds or [])
    wbuf = np.frombuffer(wb, np.uint8).copy() if wb else np.zeros(1, np.uint8)
    env = ShimEnv(world_bytes=wbuf.ctypes.data, world_off=wo.ctypes.data, n_worlds=len(case.worlds or []),
                  size=(ctypes.c_uint16 * 3)(*SIZES), table_size=TABLE_SIZE, n_waves=n_waves, scan_block=scan_block)
    outs = {k: np.full(rows_written(k, want) * WIDTH[k] + TAIL, CANARY, np.uint8) for k in fields}
    o = abi.RecDispatchOut(**{k: v.ctypes.data for k, v in outs.items()}, **caps)
    cnt = np.full(CSIZE + TAIL, CANARY, np.uint8)
    assert lib.wq_test_records_dispatch_host(ctypes.byref(a), ctypes.byref(env), ctypes.byref(o),
                                             cnt.ctypes.data if with_counters else None) == 0
    for k, v in src.items():
        assert v.tobytes() == before[k], "an input was written: " + k
    got = dict.fromkeys(ARRAYS)
    for k, v in outs.items():
        rows = rows_written(k, want)
        assert (v[rows * WIDTH[k]:] == CANARY).all(), "written behind " + k
        got[k] = shape(k, v, rows)
    if with_counters:
        assert (cnt[CSIZE:] == CANARY).all()
        got["counters"] = ingest.records_dispatch_counters(cnt)
    else:
        assert (cnt == CANARY).all()
    return got, want


def check(lib, case, what, fields=ARRAYS, with_counters=True, **kw):
    got, want = shim_call(lib, case, fields=fields, with_counters=with_counters, **kw)
    same(got, want, what, fields=fields, counters=with_counters)
    return want


def test_constants_and_layouts(shim):
    assert shim.wq_test_recdisp_granule() == 64
    assert [shim.wq_test_recdisp_sizes(k) for k in range(7)] == [
        ctypes.sizeof(abi.RecDispatchIn), ctypes.sizeof(abi.RecDispatchOut), abi.RECDISP_RUN_DTYPE.itemsize,
        abi.RECDISP_DEFER_DTYPE.itemsize, abi.REC_OP_REF_DTYPE.itemsize, CSIZE, records.REC_OP_DTYPE.itemsize]
    assert [ctypes.sizeof(abi.RecDispatchIn), ctypes.sizeof(abi.RecDispatchOut), CSIZE] == [104, 88, 152]


def test_parameter_parsing(shim):
    for text, want in READ_PARAMS.items():
        out = ctypes.c_int64(-1)
        ok = shim.wq_test_parse_after(text.encode(), len(text), ctypes.byref(out))
        assert (out.value if ok else None) == want, text


@pytest.mark.parametrize("name", sorted(named()))
def test_named_case_matches_the_definition(shim, name):
    check(shim, named()[name], name)


@pytest.mark.parametrize("name", sorted(hostile()))
def test_hostile_case_matches_the_definition(shim, name):
    check(shim, hostile()[name], name)


@functools.lru_cache(maxsize=None)
def shapes():
    """name -> Case: the sizes at which the passes take another path."""
    out = {}
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025):        # listed frames: granule and block boundaries of the frame pass
        out[f"n_db_{n}"] = Case(random_events(n, 100 + n, p_record=1.0, max_records=3, unknown=True),
                                free_handles=[9, 4, 77], handle_next=1000)
    for k in (0, 1, 63, 64, 65, 1025):                     # one frame's records: granule boundaries of the record pass
        out[f"one_frame_{k}"] = Case([ev("RecordRead", position=P), ev("RecordCreate", records=many(k, seed=k)),
                                      ev("RecordRead", "w00", position=P)])
    out["one_big_frame_among_empty_ones"] = Case([ev("RecordCreate", records=[]) for _ in range(120)] + [ev("RecordDelete", records=many(5000, seed=5))]
                                                 + [ev("RecordCreate", records=[]) for _ in range(80)])
    return out


def many(k, seed):
    """k records with every outcome among them."""
    r = np.random.default_rng(seed)
    worlds = ["world", "a b", "0bad", "elsewhere", "arena"]
    return [rec(int(r.integers(1, 1 << 40)), worlds[int(r.integers(0, 5))],
                None if r.random() < 0.1 else (float(r.integers(-50, 50)), 1e12 if r.random() < 0.1 else 0.5, 2.0),
                None if r.random() < 0.3 else "x" * int(r.integers(0, 5)), None if r.random() < 0.5 else b"\x02\x03")
            for _ in range(k)]


@pytest.mark.parametrize("name", sorted(shapes()))
def test_shape_matches_the_definition(shim, name):
    want = check(shim, shapes()[name], name)
    if name == "one_big_frame_among_empty_ones":
        c = want["counters"]
        assert c["n_records"] == 5000 and c["n_deletes"] > 2000 and c["n_deferred_records"] > 500 and c["n_runs"] == 1


def test_striding_waves_and_scan_brackets(shim):
    """Any number of striding waves and any bracketing of the frame scan give the same bytes."""
    case = shapes()["n_db_1025"]
    for n_waves, blk in ((1, 1), (2, 1024), (64, 3), (4096, 64)):
        check(shim, case, f"waves {n_waves} bracket {blk}", n_waves=n_waves, scan_block=blk)


def test_capacity_cuts(shim):
    case = shapes()["one_frame_65"]
    n_ops = case.definition()["counters"]["n_creates"]
    assert n_ops > 20
    for cap in (0, 1, n_ops // 2, n_ops - 1, n_ops):           # cuts inside the frame
        want = check(shim, case, f"ops_capacity {cap}", ops_capacity=cap)
        assert want["counters"]["overflow"] == (abi.RECDISP_OVERFLOW_OPS if cap < n_ops else 0)
    case = shapes()["n_db_1025"]
    c = case.definition()["counters"]
    assert c["n_deferred_records"] + c["n_read_deferred"] > 50
    for cap in (0, 1):
        want = check(shim, case, f"defer_capacity {cap}", defer_capacity=cap)
        assert want["counters"]["overflow"] == abi.RECDISP_OVERFLOW_DEFER
    for cap in (0, 1, c["n_runs"], c["n_runs"] + 1):
        want = check(shim, case, f"runs_capacity {cap}", runs_capacity=cap)
        assert want["counters"]["overflow"] == (abi.RECDISP_OVERFLOW_RUNS if cap <= c["n_runs"] else 0) and len(want["runs"]) == min(cap, c["n_runs"] + 1)
    total = c["n_records_total"]
    for limit in (0, 1, 63, 64, total // 2, total - 1):
        want = check(shim, case, f"max_records {limit}", max_records=limit)
        assert want["counters"]["overflow"] == abi.RECDISP_OVERFLOW_RECORDS and want["counters"]["n_records"] == limit


def test_the_allocator(shim):
    case = shapes()["n_db_65"]
    creates = case.definition()["counters"]["n_creates"]
    assert creates > 10
    for free in ([], [5, 3, 8], list(range(1000, 1000 + creates + 4))):     # none, below and above the creates
        want = check(shim, case, f"{len(free)} free", free_handles=free, handle_next=0xFFFFFFFE)
        h = want["ops"]["handle"][want["ops"]["kind"] == records.CREATE].tolist()
        assert h == (free + [(0xFFFFFFFE + k) & 0xFFFFFFFF for k in range(creates)])[:creates]


def test_nullable_outputs(shim):
    case = shapes()["n_db_65"]
    combos = [()] + [tuple(k for k in ARRAYS if k != left_out) for left_out in ARRAYS] + [("runs",), ("ops",), ("op_ref", "cls")]
    for fields in combos:
        for with_counters in (True, False):
            check(shim, case, str(fields), fields=fields, with_counters=with_counters)


def test_db_src_null_and_empty(shim):
    events = random_events(130, 77, p_record=0.5)
    check(shim, Case(events, db_src=None), "every frame listed")
    check(shim, Case(events, db_src=[]), "nothing listed")
    check(shim, Case(events, db_src=[5, 9, 64, 129]), "four frames listed")
