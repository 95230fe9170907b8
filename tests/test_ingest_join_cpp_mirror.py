"""The ingest joins' arithmetic (csrc/join_ops.hpp) on the CPU, through tests/cpp/ingest_join_host_shim.hip:
the flags and their ballot words, the compaction and its padding, the two stable sort passes, the heads and
their two scans, the decision, the apply and the merge, in the kernels' passes and the grid's order — byte
for byte against worldql_server_amd/ingest.py (join_peers_np, drop_peers_np), canaries behind every output
and the table. No GPU needed (the GPU instance: tests/test_gpu_ingest_join.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi, ingest

from test_ingest_join_host import OVERFLOWS, cases, definition, drop_args, drop_cases, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC5
TAIL = 64
CSIZE = abi.JOIN_COUNTERS_DTYPE.itemsize

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("join_shim") / "libjoinshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "ingest_join_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    lib.wq_test_ingest_join_host.restype = ctypes.c_int
    lib.wq_test_ingest_join_host.argtypes = [ctypes.POINTER(abi.JoinIn), ctypes.c_uint64, ctypes.POINTER(abi.JoinOut), vp, vp, vp,
                                             vp, ctypes.c_uint32, ctypes.c_int]
    lib.wq_test_ingest_drop_host.restype = ctypes.c_int
    lib.wq_test_ingest_drop_host.argtypes = [vp, ctypes.c_uint64, vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_int]
    lib.wq_test_join_sizes.restype = ctypes.c_uint32
    return lib


def guarded(a, room=None):
    """The array's bytes (room: the bytes the callee may write, default all of them) with the canary behind."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    room = len(raw) if room is None else room
    out = np.full(room + TAIL, CANARY, np.uint8)
    out[:len(raw)] = raw
    return out


def host_table(tu, ti, cap):
    """The table as the shim takes it: cap slots of uuids and ids, the canaries behind, the live word."""
    room = len(ti) if cap is None else cap          # without a reserve the table is not the call's to touch
    return guarded(tu, 16 * room), guarded(ti, 4 * room), np.array([len(ti)] + [0xC5C5C5C5] * 4, np.uint32)


def read_table(u, i, live, cap):
    assert (u[16 * cap:] == CANARY).all() and (i[4 * cap:] == CANARY).all(), "written behind the table"
    assert (live[1:] == 0xC5C5C5C5).all(), "written behind the live count"
    n = int(live[0])
    return u[:16 * n].reshape(n, 16).copy(), i[:4 * n].copy().view(np.uint32)


def shim_call(lib, a, fields=("j_uuid", "j_id", "j_frame"), with_counters=True):
    """The shim on exactly sized arrays with canaries behind every output and the table: a dict like
    join_peers_np's, and the definition's."""
    want = ingest.join_peers_np(a["d"], a["table_uuids"], a["table_ids"], a["free"], a["id_next"], a["id_limit"], a["capacity"],
                                a["joined_capacity"] if fields else None)
    d = a["d"]
    n = len(d["instruction"])
    cap = a["capacity"]
    jc = (a["joined_capacity"] or 0) if fields else 0
    src = {k: guarded(d[k]) for k in ("instruction", "world", "sender_uuid", "flags", "sender")}
    free = guarded(a["free"])
    outs = {k: np.full(jc * w + TAIL, CANARY, np.uint8) for k, w in (("j_uuid", 16), ("j_id", 4), ("j_frame", 4)) if k in fields}
    cnt = np.full(CSIZE + TAIL, CANARY, np.uint8)
    tu, ti, live = host_table(a["table_uuids"], a["table_ids"], cap)
    i_ = abi.JoinIn(**{k: v.ctypes.data for k, v in src.items()}, free_ids=free.ctypes.data if len(a["free"]) else None,
                    n_free=len(a["free"]), id_next=a["id_next"], id_limit=a["id_limit"])
    o_ = abi.JoinOut(**{k: v.ctypes.data for k, v in outs.items()}, joined_capacity=jc)
    rc = lib.wq_test_ingest_join_host(ctypes.byref(i_), n, ctypes.byref(o_), cnt.ctypes.data if with_counters else None,
                                      tu.ctypes.data, ti.ctypes.data, live.ctypes.data, cap or 0, cap is not None)
    assert rc == 0, "a working array was written behind its end"
    for k in ("instruction", "world", "sender_uuid"):
        assert src[k].tobytes() == guarded(d[k]).tobytes(), "an input was written: " + k
    assert free.tobytes() == guarded(a["free"]).tobytes()
    for k, v in list(src.items()) + list(outs.items()):
        assert (v[len(v) - TAIL:] == CANARY).all(), "written behind " + k
    k_rows = len(want["j_id"])
    got = dict(sender=src["sender"][:4 * n].copy().view(np.uint32), flags=src["flags"][:n].copy(),
               table=read_table(tu, ti, live, cap or 0) if cap is not None else want["table"])
    for k, w in (("j_uuid", 16), ("j_id", 4), ("j_frame", 4)):
        if k in outs:
            assert (outs[k][k_rows * w:] == CANARY).all(), "written behind the rows of " + k
            r = outs[k][:k_rows * w].copy()
            got[k] = r.reshape(k_rows, 16) if k == "j_uuid" else r.view(np.uint32)
    if with_counters:
        got["counters"] = ingest.join_counters(cnt)
    else:
        assert (cnt == CANARY).all()
    return got, want


def test_layouts(shim):
    assert [shim.wq_test_join_sizes(k) for k in range(4)] == [ctypes.sizeof(abi.JoinIn), ctypes.sizeof(abi.JoinOut), CSIZE, 96]


@pytest.mark.parametrize("name", sorted(cases()))
def test_kernel_arithmetic_matches_the_definition(shim, name):
    a = cases()[name]
    fields = ("j_uuid", "j_id", "j_frame") if a["joined_capacity"] is not None else ()
    got, want = shim_call(shim, a, fields=fields)
    same(got, want, name, fields=("sender", "flags") + fields)
    same(want, definition(name), name)
    if name in OVERFLOWS:
        assert got["counters"]["overflow"] == OVERFLOWS[name]


def test_nullable_outputs(shim):
    a = cases()["mix_1025"]
    for fields in (("j_uuid",), ("j_id",), ("j_frame",), ("j_id", "j_frame"), ()):
        for with_counters in (True, False):
            got, want = shim_call(shim, a, fields=fields, with_counters=with_counters)
            same(got, want, str(fields), fields=("sender", "flags") + fields, counters=with_counters)
    # joined_capacity counts only when a j_* array is given
    short = dict(cases()["joined_capacity_short"])
    got, want = shim_call(shim, short, fields=())
    assert got["counters"]["overflow"] == 0 and got["counters"]["n_patched"] == 7
    same(got, want, "no arrays, no capacity", fields=("sender", "flags"))


@pytest.mark.parametrize("name", sorted(drop_cases()))
def test_drop_matches_the_definition(shim, name):
    tu, ti, cap, ids = drop_args(name)
    for reserved in (True, False):
        want = ingest.drop_peers_np(tu, ti, ids, reserved=reserved)
        u, i, live = host_table(tu, ti, cap)
        d_ids = guarded(ids)
        cnt = np.full(CSIZE + TAIL, CANARY, np.uint8)
        assert shim.wq_test_ingest_drop_host(d_ids.ctypes.data if len(ids) else None, len(ids), cnt.ctypes.data, u.ctypes.data,
                                             i.ctypes.data, live.ctypes.data, cap, reserved) == 0
        assert d_ids.tobytes() == guarded(ids).tobytes() and (cnt[CSIZE:] == CANARY).all()
        gu, gi = read_table(u, i, live, cap)
        assert gu.tobytes() == want["table"][0].tobytes() and gi.tolist() == want["table"][1].tolist(), name
        assert ingest.join_counters(cnt) == want["counters"], name
