"""The frame builder's arithmetic (csrc/frame_ops.hpp, tiles and stores from csrc/pack_ops.hpp) on the
CPU, through tests/cpp/frames_build_host_shim.hip: a message's fields under the validity rules, the
builder's push sequence replayed on counters, the scan, the frame that covers a byte, the chunk sink
with its masked 16-byte loads and the narrow stores, in the passes and tile sizes the kernels use, byte
for byte against worldql_server_amd/frames.py (build_frames_np). No GPU needed (the GPU instance:
tests/test_gpu_frames_build.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import frames

from test_frames_build_host import (MIB, TILE, cases, malformed_cases, names, nullable_cases, too_large_case, want)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC5
CANARY32 = 0xC0FFEE11
CANARY64 = 0xC0FFEE11C0FFEE11
TAIL = 64   # canary bytes behind the output

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


class ShimIn(ctypes.Structure):  # struct wq_test_frames_in
    _fields_ = [(k, ctypes.c_void_p) for k in ("instruction", "replication", "sender_uuid", "world", "pos", "param",
                                               "param_offsets", "flex", "flex_offsets", "msg_flags", "world_bytes",
                                               "world_off")] + \
               [(k, ctypes.c_uint64) for k in ("n", "n_param_bytes", "n_flex_bytes", "n_world_bytes")] + \
               [("n_worlds", ctypes.c_uint32), ("instruction_all", ctypes.c_uint8), ("replication_all", ctypes.c_uint8)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("frames_shim") / "libframesshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                           "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "frames_build_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    lib.wq_test_frames_build_host.restype = u64
    lib.wq_test_frames_build_host.argtypes = [ctypes.POINTER(ShimIn), vp, sz, vp, vp, vp]
    lib.wq_test_frames_tile.restype = ctypes.c_uint32
    lib.wq_test_frames_max.restype = u64
    return lib


def exact(a, dtype):
    """A fresh, exactly sized, contiguous copy (None stays None; an empty array keeps a real address)."""
    if a is None:
        return None
    a = np.array(a, dtype=dtype, copy=True).reshape(-1)
    return a if a.size else np.zeros(1, dtype)[:0]


def shim_call(lib, c, capacity, with_size=True, with_counters=True):
    """The shim on exactly sized inputs with canaries behind every output: (frames[:bytes_written],
    offsets, sizes or None, counters or None, tiles on the whole-tile path). The output buffer is
    16-byte aligned."""
    n = c.n
    keep = dict(uuid=exact(c.sender_uuid, np.uint8), world=exact(c.world, np.uint32),
                ins=None if np.isscalar(c.instruction) else exact(c.instruction, np.uint8),
                rep=None if np.isscalar(c.replication) else exact(c.replication, np.uint8),
                pos=exact(c.pos, np.float64), param=exact(c.param, np.uint8), po=exact(c.param_offsets, np.uint64),
                flex=exact(c.flex, np.uint8), fo=exact(c.flex_offsets, np.uint64), flags=exact(c.msg_flags, np.uint8))
    wb, wo = frames.world_table(c.worlds or [])
    keep["wb"], keep["wo"] = np.frombuffer(wb, np.uint8).copy(), wo
    p = lambda a: None if a is None else (a.ctypes.data or None)
    # a payload with no bytes still counts as given: the offsets decide
    given = lambda data, off: None if off is None else (p(data) or 1)
    a = ShimIn(instruction=p(keep["ins"]), replication=p(keep["rep"]), sender_uuid=p(keep["uuid"]), world=p(keep["world"]),
               pos=p(keep["pos"]), param=given(keep["param"], keep["po"]), param_offsets=p(keep["po"]),
               flex=given(keep["flex"], keep["fo"]), flex_offsets=p(keep["fo"]), msg_flags=p(keep["flags"]),
               world_bytes=p(keep["wb"]), world_off=p(keep["wo"]) if c.worlds else None, n=n,
               n_param_bytes=(len(keep["param"]) if c.n_param_bytes is None else c.n_param_bytes) if c.param is not None else 0,
               n_flex_bytes=(len(keep["flex"]) if c.n_flex_bytes is None else c.n_flex_bytes) if c.flex is not None else 0,
               n_world_bytes=len(wb), n_worlds=len(c.worlds or []),
               instruction_all=int(c.instruction) if np.isscalar(c.instruction) else 0,
               replication_all=int(c.replication) if np.isscalar(c.replication) else 0)
    raw = np.full(capacity + TAIL + 16, CANARY, np.uint8)
    shift = (-raw.ctypes.data) % 16
    out = raw[shift:shift + capacity + TAIL]
    off = np.full(n + 1 + 8, CANARY64, np.uint64)
    size = np.full(n + 8, CANARY32, np.uint32)
    cnt = np.full(6 + 2, CANARY64, np.uint64)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    fast = lib.wq_test_frames_build_host(ctypes.byref(a), vp(out) if capacity else None, capacity, vp(off),
                                         vp(size) if with_size else None, vp(cnt) if with_counters else None)
    assert (off[n + 1:] == CANARY64).all(), "written behind d_frame_offsets[n]"
    assert (size[n if with_size else 0:] == CANARY32).all(), "written behind d_frame_size[n)"
    written = min(int(off[n]), capacity)
    assert (out[written:] == CANARY).all(), "written behind d_frames[bytes_written)"
    assert (raw[:shift] == CANARY).all()
    counters = None
    if with_counters:
        assert (cnt[6:] == CANARY64).all()
        counters = dict(zip(frames.FRAMES_COUNTERS_DTYPE.names, (int(v) for v in cnt[:6])))
        assert counters["bytes_written"] == written
    else:
        assert (cnt == CANARY64).all()
    return out[:written].copy(), off[:n + 1].copy(), size[:n].copy() if with_size else None, counters, fast


def same(got, wanted):
    data, off, sizes, cnt = got[:4]
    w_data, w_off, w_sizes, w_cnt = wanted
    assert off.tobytes() == w_off.tobytes()
    assert sizes is None or sizes.tobytes() == w_sizes.tobytes()
    assert cnt is None or cnt == w_cnt
    if data.tobytes() != w_data.tobytes():
        bad = int(np.flatnonzero(data != w_data)[0])
        i = int(np.searchsorted(w_off, bad, side="right")) - 1
        raise AssertionError(f"first differing byte {bad}: frame {i}, byte {bad - int(w_off[i])} of {int(w_sizes[i])}")


def test_constants(shim):
    assert shim.wq_test_frames_tile() == TILE and shim.wq_test_frames_max() == frames.FRAME_MAX


@pytest.mark.parametrize("name", names())
def test_kernel_arithmetic_matches_host_reference(shim, name):
    c = cases()[name]
    w = want(name)
    need = len(w[0])
    first = shim_call(shim, c, need)
    same(first, w)
    for with_size, with_counters in ((False, True), (True, False), (False, False)):
        same(shim_call(shim, c, need, with_size=with_size, with_counters=with_counters), w)
    sizing = shim_call(shim, c, 0)
    assert sizing[1].tobytes() == w[1].tobytes() and sizing[2].tobytes() == w[2].tobytes()
    assert sizing[3] == dict(w[3], bytes_written=0, overflow=int(need > 0),
                             n_complete=int(np.count_nonzero(w[1][1:] <= 0)))
    roomy = shim_call(shim, c, need + 33)
    same(roomy, w)


def test_big_payloads_take_the_whole_tile_path(shim):
    fast = shim_call(shim, cases()["with_big"], len(want("with_big")[0]))[4]
    assert 2 * (MIB // TILE - 1) <= fast <= 2 * (MIB // TILE + 1)
    assert shim_call(shim, cases()["grid"], len(want("grid")[0]))[4] == 0


def test_every_capacity_of_a_small_case(shim):
    """Every capacity from 0 to bytes_need + 1 of a case of about 300 bytes: the cut falls on every byte
    of values, strings, payloads, padding and chunk ends."""
    c = cases()["cap_300"]
    whole, off, sizes, _ = want("cap_300")
    for cap in range(0, len(whole) + 2):
        data, o, s, cnt, _ = shim_call(shim, c, cap)
        assert data.tobytes() == whole[:cap].tobytes() and o.tobytes() == off.tobytes() and s.tobytes() == sizes.tobytes()
        assert cnt == frames.build_frames_np(capacity=cap, **c.kw())[3]


@pytest.mark.parametrize("combo,c", nullable_cases(), ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else "")
def test_every_nullable_combination(shim, combo, c):
    w = frames.build_frames_np(**c.kw())
    same(shim_call(shim, c, len(w[0])), w)
    assert w[3]["error"] == frames.ERROR_WORLD   # world 200 is outside the table in every combination


@pytest.mark.parametrize("name", list(malformed_cases()))
def test_malformed_inputs(shim, name):
    c, bits = malformed_cases()[name]
    w = frames.build_frames_np(**c.kw())
    got = shim_call(shim, c, len(w[0]))
    same(got, w)
    assert got[3]["error"] == bits


def test_too_large_frames_through_the_sizing_call(shim):
    """The 2^30 rule: offsets that claim the lengths, no payload memory, capacity 0."""
    c, sizes_want = too_large_case()
    w = frames.build_frames_np(capacity=0, **c.kw())
    got = shim_call(shim, c, 0)
    same(got, w)
    assert list(got[2]) == sizes_want and got[3]["error"] == frames.ERROR_TOO_LARGE
