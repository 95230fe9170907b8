"""The table export's arithmetic of csrc/export_ops.hpp on the CPU (tests/cpp/table_export_host_shim.hip:
the live-cube flag, the cube sort words, the cube of a row, the row's peer, the row and the bitmap
test, in the flag / compact / radix passes / scan / granule emit / filter compaction shape of
wq_table_export.hip) against snapshot.TableRef.export, byte for byte. The shim builds the record,
slot and list layout itself from TableRef's cubes. Needs hipcc only, no GPU. Every output array is
followed by canary words that must survive the call, at full and truncated capacities.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi
from worldql_server_amd.snapshot import TableRef

from test_snapshot_host import BIG_WORLD, R, S, ops_of, random_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 16
MARK = 0xA5A5A5A5A5A5A5A5

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("table_export_shim") / "libtableexportshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-o", out, os.path.join(ROOT, "tests", "cpp", "table_export_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.wq_test_table_export_host.restype = ctypes.c_int
    lib.wq_test_table_export_host.argtypes = [ctypes.c_uint16, sz, vp, vp, vp, vp, u32, ctypes.c_int, vp, u32, vp, sz,
                                              ctypes.POINTER(sz)]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def layout_of(t: TableRef, emptied=()):
    """TableRef's cubes (in its dict's order: the shim must not depend on it) plus cubes that keep
    their key with no peer, as the shim's arrays."""
    cubes = list(t.cubes.items()) + [(c, set()) for c in emptied]
    world = np.array([c[0] for c, _ in cubes], np.uint32)
    key = np.array([c[1:] for c, _ in cubes], np.int64).reshape(-1, 3)
    off = np.zeros(len(cubes) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for _, s in cubes])
    peers = np.array([p for _, s in cubes for p in sorted(s)], np.uint32)
    return world, key, off, peers


def shim_export(lib, t, layout, capacity, world=None, peers=None):
    w, k, off, ps = layout
    out = np.full((capacity * 5 + CANARY), MARK, np.uint64)
    n = ctypes.c_size_t()
    fp = None if peers is None else np.ascontiguousarray(peers, np.uint32)
    rc = lib.wq_test_table_export_host(t.cube_size, len(w), _p(w), _p(k), _p(off), _p(ps),
                                       abi.WORLD_INVALID if world is None else world, int(peers is not None),
                                       None if fp is None or len(fp) == 0 else _p(fp), 0 if fp is None else len(fp),
                                       _p(out), capacity, ctypes.byref(n))
    kept = min(n.value, capacity)
    assert (out[kept * 5:] == MARK).all(), "rows past the capacity (or the count) were written"
    return rc, n.value, out[: kept * 5].tobytes()


def check(lib, t, emptied=(), **kw):
    want = t.export(**kw).tobytes()
    n = len(want) // 40
    layout = layout_of(t, emptied)
    for cap in sorted({n, n + 5, max(n - 1, 0), n // 2, min(n, 64), min(n, 65), min(n, 1), 0}):
        rc, got_n, raw = shim_export(lib, t, layout, cap, **kw)
        assert got_n == n and rc == (abi.WQ_E_CAPACITY if n > cap else 0), (kw, cap)
        assert raw == want[: cap * 40], (kw, cap)
    return n


def edge_table(cs):
    rows, nxt = [], 0
    for i, n in enumerate([1, 24, 25, 63, 64, 65, 257, 1025]):
        rows += [(i % 2, p, S, (cs * (i - 4), -cs * i, cs * 3)) for p in range(nxt, nxt + n)]
        nxt += n // 2
    far = (1 << 23) - 1
    rows += [(0, 7, S, (far * cs, -far * cs, far * cs)), (0, 5, S, (-far * cs, far * cs, -far * cs)),
             (0, 9, S, (7, 1, 1)), (0, 2, S, (7, 1, 1)), (BIG_WORLD, 1, S, (0, cs, 0)),
             (1, 11, S, None, (float("nan"), 1.0, -1.0)), (0, 30, S, None, (0.5 * cs, -0.5 * cs, 2.5 * cs))]
    t = TableRef(cs)
    t.apply(ops_of(rows))
    return t


@pytest.mark.parametrize("cs", [16, 10])
def test_list_length_edges_and_filters(shim, cs):
    t = edge_table(cs)
    emptied = [(0, cs * 9, 0, 0), (BIG_WORLD, 3, 3, 3), (1, -cs, 0, 0)]
    assert check(shim, t, emptied) > 1400
    top = int(t.export()["peer"].max())
    for kw in (dict(world=1), dict(world=0), dict(peers=[3, 600, top + 1000]), dict(world=0, peers=[3, 600, top + 1000]),
               dict(peers=[]), dict(world=77), dict(world=BIG_WORLD), dict(peers=[0xFFFFFFFE]),
               dict(world=1, peers=np.arange(0, top + 1, 3)), dict(peers=[top, 0, 0])):
        check(shim, t, emptied, **kw)


def test_empty_tables(shim):
    t = TableRef(16)
    assert check(shim, t) == 0
    assert check(shim, t, emptied=[(0, 16, 16, 16), (BIG_WORLD, 1, 2, 3)]) == 0
    assert check(shim, t, emptied=[(0, 16, 16, 16)], world=0, peers=[1]) == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_ops(shim, seed):
    t = TableRef(16)
    t.apply(random_ops(3000, seed))
    before = set(t.cubes)
    t.apply(ops_of([(abi.WORLD_INVALID, p, R, (0, 0, 0)) for p in range(0, 40, 3)]))
    emptied = sorted(before - set(t.cubes))  # cubes these disconnects emptied keep their key
    assert check(shim, t, emptied) > 50 and len(emptied) > 10
    check(shim, t, emptied, world=seed % 3)
    check(shim, t, emptied, peers=[1, 2, 4, 8, 16, 32, 64])
    check(shim, t, emptied, world=0, peers=np.arange(1, 40, 2))
