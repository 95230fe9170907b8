"""The send buffers' arithmetic (csrc/pack_ops.hpp, rows from csrc/budget_ops.hpp) on the CPU, through
tests/cpp/peer_pack_host_shim.hip: frame validity and size, the scan of the record sizes, the element
that covers a byte, the window search, the chunk composer with its masked 16-byte loads and the narrow
stores, in the passes and tile sizes the kernels use, byte for byte against
worldql_server_amd/interest.py (peer_pack_np). No GPU needed (the GPU instance:
tests/test_gpu_peer_pack.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi

from test_peer_pack_host import BIG, CHUNK, RUN, TILE, WINDOW, cap_of, cases, names, want, well_formed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC5
CANARY64 = 0xC0FFEE11C0FFEE11
TAIL = 64   # canary bytes behind the output

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("peer_pack_shim") / "libpeerpackshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                           "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "peer_pack_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp, sz, u32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64
    lib.wq_test_peer_pack_host.restype = u64
    lib.wq_test_peer_pack_host.argtypes = [vp, vp, u32, sz, vp, vp, sz, sz, u32, vp, sz, vp, vp, vp]
    for f in ("tile", "chunk", "window", "run"):
        getattr(lib, "wq_test_pack_" + f).restype = u32
    return lib


def shim_call(lib, c, prefix, capacity, with_elem=True, with_counters=True):
    """The shim on exactly sized inputs with canaries behind every output: (out[:bytes_written], PB, E or
    None, counters or None, tiles on the whole-tile path). The output buffer is 16-byte aligned."""
    n_in = len(c.msgs)
    raw = np.full(capacity + TAIL + 16, CANARY, np.uint8)
    shift = (-raw.ctypes.data) % 16
    out = raw[shift:shift + capacity + TAIL]
    pb = np.full(c.n_peers + 1 + 8, CANARY64, np.uint64)
    eb = np.full(n_in + 8, CANARY64, np.uint64)
    cnt = np.full(6 + 2, CANARY64, np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
    fast = lib.wq_test_peer_pack_host(p(c.offsets), p(c.msgs), c.n_peers, n_in, p(c.frames), p(c.frame_offsets),
                                      len(c.frame_offsets) - 1, len(c.frames), abi.PACK_LEN_PREFIX if prefix else 0,
                                      out.ctypes.data_as(ctypes.c_void_p) if capacity else None, capacity,
                                      pb.ctypes.data_as(ctypes.c_void_p), p(eb) if with_elem else None,
                                      p(cnt) if with_counters else None)
    assert (pb[c.n_peers + 1:] == CANARY64).all(), "written behind PB[n_peers]"
    written = min(int(pb[c.n_peers]), capacity)
    assert (out[written:] == CANARY).all(), "written behind d_out[bytes_written)"
    assert (raw[:shift] == CANARY).all()
    counters = None
    if with_counters:
        assert (cnt[6:] == CANARY64).all()
        counters = dict(zip(abi.PACK_COUNTERS_DTYPE.names, (int(v) for v in cnt[:6])))
        assert counters["bytes_written"] == written
        walked = counters["n_in"]
    else:
        assert (cnt == CANARY64).all()
        walked = len(want_walked(c, prefix))
    assert (eb[walked if with_elem else 0:] == CANARY64).all(), "written behind d_out_elem_bytes[walked)"
    return out[:written].copy(), pb[:c.n_peers + 1], eb[:walked] if with_elem else None, counters, fast


def want_walked(c, prefix):
    name = next(n for n, x in cases().items() if x is c)
    return want(name, prefix)[2]


def same(name, prefix, got):
    out, pb, eb, cnt = got[:4]
    w_out, w_pb, w_eb, w_cnt = want(name, prefix)
    assert out.tobytes() == w_out.tobytes()
    assert pb.tobytes() == w_pb.tobytes()
    assert eb is None or eb.tobytes() == w_eb.tobytes()
    assert cnt is None or cnt == w_cnt
    well_formed(cases()[name], prefix, out, pb, w_eb, cnt)


def test_constants_are_the_ones_the_cases_straddle(shim):
    assert shim.wq_test_pack_tile() == TILE and shim.wq_test_pack_chunk() == CHUNK
    assert shim.wq_test_pack_window() == WINDOW and TILE == CHUNK * 64
    assert shim.wq_test_pack_run() == RUN
    assert abi.PACK_COUNTERS_DTYPE.itemsize == 40


@pytest.mark.parametrize("prefix", [False, True])
@pytest.mark.parametrize("name", names())
def test_kernel_arithmetic_matches_host_reference(shim, name, prefix):
    c = cases()[name]
    cap = cap_of(name, prefix)
    first = shim_call(shim, c, prefix, cap)
    same(name, prefix, first)
    for with_elem, with_counters in ((False, True), (True, False), (False, False)):
        got = shim_call(shim, c, prefix, cap, with_elem=with_elem, with_counters=with_counters)
        same(name, prefix, got)
        assert got[0].tobytes() == first[0].tobytes()
    sizing = shim_call(shim, c, prefix, 0)
    assert sizing[1].tobytes() == first[1].tobytes() and sizing[3]["bytes_need"] == first[3]["bytes_need"]
    assert sizing[3]["bytes_written"] == 0


def test_big_frame_takes_the_whole_tile_path(shim):
    for prefix in (False, True):
        fast = shim_call(shim, cases()["big_frame"], prefix, cap_of("big_frame", prefix))[4]
        assert BIG // TILE - 1 <= fast <= BIG // TILE + 1
    assert shim_call(shim, cases()["tiny_runs"], True, cap_of("tiny_runs", True))[4] == 0


@pytest.mark.parametrize("prefix", [False, True])
def test_every_capacity_of_a_small_case(shim, prefix):
    """Every capacity from 0 to bytes_need + 1 of the tiny runs' first 300 bytes and of the capacity
    case: the cut falls on every byte of prefixes, frames and chunk ends."""
    from worldql_server_amd import interest
    for name, top in (("tiny_runs", 300), ("cap_need", None)):
        c = cases()[name]
        whole = want(name, prefix)[0]
        for cap in range(0, (top or len(whole)) + 2):
            out, pb, eb, cnt, _ = shim_call(shim, c, prefix, cap)
            assert out.tobytes() == whole[:cap].tobytes()
            w = interest.peer_pack_np(c.offsets, c.msgs, c.frames, c.frame_offsets, len_prefix=prefix, capacity=cap)
            assert cnt == w[3]
