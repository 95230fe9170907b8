"""The ingest leaves' arithmetic (csrc/leave_ops.hpp) on the CPU, through tests/cpp/ingest_leave_host_shim.hip:
the listed bitmap, the flags and their ballot words over the reserved room, the scan, the decision, the apply
(rows, uuid text, bitmap, free list, stamps, the table's compaction) and the copy back, in the kernels' passes
and the grid's order — byte for byte against worldql_server_amd/ingest.py (leave_peers_np), canaries behind
every output, the table, last_seen, the bitmap and the free list. No GPU needed (the GPU instance:
tests/test_gpu_ingest_leave.py)."""
import ctypes
import os
import subprocess
import uuid

import numpy as np
import pytest

from worldql_server_amd import abi, ingest

from test_ingest_leave_host import OVERFLOWS, ROW_FIELDS, cases, define, definition, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC5
TAIL = 64
CSIZE = abi.LEAVE_COUNTERS_DTYPE.itemsize
WIDTH = dict(l_uuid=16, l_id=4, l_reason=1, l_param=abi.LEAVE_TEXT)
ALL_OUT = ROW_FIELDS + ("gone_bits", "free_out")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("leave_shim") / "libleaveshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "ingest_leave_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    lib.wq_test_ingest_leave_host.restype = ctypes.c_int
    lib.wq_test_ingest_leave_host.argtypes = [ctypes.POINTER(abi.LeaveIn), ctypes.POINTER(abi.LeaveOut), vp, vp, vp, vp,
                                              ctypes.c_uint32, ctypes.c_int]
    lib.wq_test_leave_sizes.restype = ctypes.c_uint32
    lib.wq_test_leave_text_char.restype = ctypes.c_uint8
    lib.wq_test_leave_text_char.argtypes = [vp, ctypes.c_uint32]
    return lib


def guarded(a, room=None):
    """The array's bytes (room: the bytes the callee may write, default all of them) with the canary behind."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    room = len(raw) if room is None else room
    out = np.full(room + TAIL, CANARY, np.uint8)
    out[:len(raw)] = raw
    return out


def shim_call(lib, a, fields=ALL_OUT, with_counters=True):
    """The shim on exactly sized arrays with canaries behind every one: a dict like leave_peers_np's, and the
    definition's for the arrays given."""
    rows = any(k in fields for k in ROW_FIELDS)
    want = define(dict(a, leave_capacity=a["leave_capacity"] if rows else None,
                       free_capacity=a["free_capacity"] if "free_out" in fields else None))
    n_ids, cap = len(a["last_seen"]), a["capacity"]
    lc = (a["leave_capacity"] or 0) if rows else 0
    fc = (a["free_capacity"] or 0) if "free_out" in fields else 0
    words = (n_ids + 31) // 32
    seen, free, listed = guarded(a["last_seen"]), guarded(a["free"]), guarded(a["leave_ids"])
    pinned = guarded(a["pinned"]) if a["pinned"] is not None else None
    room = dict({k: lc * w for k, w in WIDTH.items()}, l_param_offsets=8 * (lc + 1), gone_bits=4 * words, free_out=4 * fc)
    outs = {k: np.full(room[k] + TAIL, CANARY, np.uint8) for k in fields}
    cnt = np.full(CSIZE + TAIL, CANARY, np.uint8)
    tu, ti = guarded(a["table_uuids"], 16 * cap), guarded(a["table_ids"], 4 * cap)
    live = np.array([len(a["table_ids"])] + [0xC5C5C5C5] * 4, np.uint32)
    i_ = abi.LeaveIn(last_seen=seen.ctypes.data, pinned_bits=None if pinned is None else pinned.ctypes.data,
                     leave_ids=listed.ctypes.data if len(a["leave_ids"]) else None, free_ids=free.ctypes.data if len(a["free"]) else None,
                     n_ids=n_ids, now=a["now"], max_age=a["max_age"], n_leave=len(a["leave_ids"]), n_free=len(a["free"]))
    o_ = abi.LeaveOut(**{k: v.ctypes.data for k, v in outs.items()}, leave_capacity=lc, free_capacity=fc)
    rc = lib.wq_test_ingest_leave_host(ctypes.byref(i_), ctypes.byref(o_), cnt.ctypes.data if with_counters else None,
                                       tu.ctypes.data, ti.ctypes.data, live.ctypes.data, cap, a["reserved"])
    assert rc == 0, "a working array was written behind its end"
    assert free.tobytes() == guarded(a["free"]).tobytes() and listed.tobytes() == guarded(a["leave_ids"]).tobytes()
    assert pinned is None or pinned.tobytes() == guarded(a["pinned"]).tobytes()
    assert (seen[4 * n_ids:] == CANARY).all(), "written behind last_seen"
    assert (tu[16 * cap:] == CANARY).all() and (ti[4 * cap:] == CANARY).all(), "written behind the table"
    assert (live[1:] == 0xC5C5C5C5).all(), "written behind the live count"
    n = int(live[0])
    got = dict(last_seen=seen[:4 * n_ids].copy().view(np.uint32),
               table=(tu[:16 * n].reshape(n, 16).copy(), ti[:4 * n].copy().view(np.uint32)))
    k = len(want["l_id"])
    wrote = dict({f: k * w for f, w in WIDTH.items()}, l_param_offsets=8 * len(want["l_param_offsets"]), gone_bits=4 * words,
                 free_out=4 * len(want["free_out"]))
    dtypes = dict(l_id=np.uint32, l_param_offsets=np.uint64, gone_bits=np.uint32, free_out=np.uint32)
    for f, v in outs.items():
        assert (v[wrote[f]:] == CANARY).all(), "written behind the rows of " + f
        r = v[:wrote[f]].copy()
        got[f] = r.reshape(k, 16) if f == "l_uuid" else r.view(dtypes.get(f, np.uint8))
    if with_counters:
        assert (cnt[CSIZE:] == CANARY).all()
        got["counters"] = ingest.leave_counters(cnt)
    else:
        assert (cnt == CANARY).all()
    return got, want


def test_layouts(shim):
    assert [shim.wq_test_leave_sizes(k) for k in range(4)] == [ctypes.sizeof(abi.LeaveIn), ctypes.sizeof(abi.LeaveOut), CSIZE, 96]


def test_uuid_text(shim):
    rng = np.random.default_rng(3)
    for raw in [bytes(16), bytes([255] * 16), bytes(range(16)), bytes.fromhex("0123456789abcdeffedcba9876543210")] + \
               [rng.integers(0, 256, 16).astype(np.uint8).tobytes() for _ in range(50)]:
        buf = np.frombuffer(raw, np.uint8).copy()
        text = bytes(shim.wq_test_leave_text_char(buf.ctypes.data, k) for k in range(36)).decode()
        assert text == str(uuid.UUID(bytes=raw))


@pytest.mark.parametrize("name", sorted(cases()))
def test_kernel_arithmetic_matches_the_definition(shim, name):
    a = cases()[name]
    fields = tuple(k for k in ALL_OUT if (a["leave_capacity"] is not None or k not in ROW_FIELDS) and
                   (a["free_capacity"] is not None or k != "free_out"))
    got, want = shim_call(shim, a, fields=fields)
    same(got, want, name, fields=fields + ("last_seen",))
    same(want, definition(name), name)
    if name in OVERFLOWS:
        assert got["counters"]["overflow"] == OVERFLOWS[name]


def test_nullable_outputs(shim):
    a = cases()["mix_1025"]
    for fields in (("l_uuid",), ("l_id",), ("l_reason",), ("l_param", "l_param_offsets"), ("l_param_offsets",), ("gone_bits",),
                   ("free_out",), ("l_id", "free_out"), ()):
        for with_counters in (True, False):
            got, want = shim_call(shim, a, fields=fields, with_counters=with_counters)
            same(got, want, str(fields), fields=fields + ("last_seen",), counters=with_counters)
    # a capacity counts only when its array is given
    got, want = shim_call(shim, cases()["both_overflows"], fields=("gone_bits",))
    assert got["counters"]["overflow"] == 0 and got["counters"]["n_left"] == 11
    same(got, want, "no arrays, no capacities", fields=("gone_bits", "last_seen"))
    got, want = shim_call(shim, cases()["both_overflows"], fields=("l_id",))
    assert got["counters"]["overflow"] == 1
    got, want = shim_call(shim, cases()["both_overflows"], fields=("free_out",))
    assert got["counters"]["overflow"] == 2
    same(got, want, "only the free list", fields=("free_out", "last_seen"))
