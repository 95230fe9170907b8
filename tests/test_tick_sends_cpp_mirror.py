"""The tick sends' arithmetic (csrc/sends_ops.hpp) on the CPU, through tests/cpp/tick_sends_host_shim.hip:
the host's check of the regions, their prefixes, the region and the row that hold an element, its frame,
its drops and its composite key, the row check, the key widths and the per-peer lower bound, in the
begin / rows / expand / stable sort / lower bound shape the kernels use, byte for byte against
worldql_server_amd/interest.py (tick_sends_np). No GPU needed (the GPU instance: tests/test_gpu_tick_sends.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi

from test_tick_sends_host import cases, exact_names, hostile_names, invalid_cases, want, well_formed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC0FFEE11

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tick_sends_shim") / "libticksendsshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "tick_sends_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    lib.wq_test_tick_sends_host.restype = ctypes.c_int
    lib.wq_test_tick_sends_host.argtypes = [ctypes.POINTER(abi.TickSendsIn), vp, vp, ctypes.c_size_t, vp, ctypes.POINTER(ctypes.c_int)]
    return lib


def host_call(c):
    """The wq_tick_sends_in of a case with every array on the host; the arrays are kept alive beside it."""
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and len(a) else None
    n = lambda a: 0 if a is None else len(a)
    keep = (np.ascontiguousarray(c.regions), c.offsets, c.peers, c.srcs, c.connected)
    src = abi.TickSendsIn(regions=p(keep[0]), d_offsets=p(c.offsets), n_offsets=len(c.offsets), d_peers=p(c.peers),
                          n_pairs=c.n_pairs, d_src=(ctypes.c_void_p * 2)(p(c.srcs[0]), p(c.srcs[1])),
                          n_src=(ctypes.c_size_t * 2)(n(c.srcs[0]), n(c.srcs[1])),
                          d_connected=p(c.connected) if c.connected is not None else None, n_regions=len(c.regions),
                          n_peers=c.n_peers, n_frames=c.n_frames)
    return src, keep


def shim_sends(lib, c):
    """The shim on exactly sized inputs with canary words behind both outputs and the counters:
    (peer_offsets, frames_out, counters, key width)."""
    po = np.full(c.n_peers + 1 + 8, CANARY, np.uint32)
    fo = np.full(c.n_elems + 8, CANARY, np.uint32)
    cnt = np.full(16 + 8, CANARY, np.uint32)
    src, keep = host_call(c)
    width = ctypes.c_int(-1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.wq_test_tick_sends_host(ctypes.byref(src), p(po), p(fo), c.n_elems, p(cnt), ctypes.byref(width)) == 0
    assert (po[c.n_peers + 1:] == CANARY).all() and (fo[c.n_elems:] == CANARY).all() and (cnt[16:] == CANARY).all()
    rec = cnt[:16].view(abi.TICK_SENDS_COUNTERS_DTYPE)[0]
    assert int(rec["pad_"]) == 0 and int(rec["reserved_"]) == 0
    return po[:c.n_peers + 1], fo[:c.n_elems], {k: int(rec[k]) for k in rec.dtype.names if not k.endswith("_")}, width.value


@pytest.mark.parametrize("name", exact_names())
def test_kernel_arithmetic_matches_host_reference(shim, name):
    c = cases()[name]
    po, fo, cnt, _ = shim_sends(shim, c)
    w_po, w_frames, w_cnt = want(name)
    assert po.tobytes() == w_po.tobytes()
    assert fo[:len(w_frames)].tobytes() == w_frames.tobytes()
    assert cnt == w_cnt
    well_formed(c, po, fo, cnt)


def test_both_key_widths_run(shim):
    widths = {name: shim_sends(shim, cases()[name])[3] for name in exact_names()}
    assert widths["mixed_32bit"] == 32 and widths["exactly_32_bits"] == 32
    assert widths["mixed_64bit"] == 64 and widths["exactly_33_bits"] == 64 and widths["frames_2_pow_32"] == 64
    assert widths["no_regions"] == 0 and widths["no_elems"] == 0


@pytest.mark.parametrize("name", hostile_names())
def test_hostile_offsets_stay_well_formed(shim, name):
    c = cases()[name]
    po, fo, cnt, _ = shim_sends(shim, c)
    well_formed(c, po, fo, cnt)
    assert cnt["error"] & abi.SENDS_ERROR_ROWS
    again = shim_sends(shim, c)
    assert po.tobytes() == again[0].tobytes() and fo.tobytes() == again[1].tobytes() and cnt == again[2]


@pytest.mark.parametrize("name", sorted(invalid_cases()))
def test_invalid_calls_are_refused_and_write_nothing(shim, name):
    c = invalid_cases()[name]
    po = np.full(c.n_peers % 1000 + 1, CANARY, np.uint32)      # never written: its size does not matter
    fo = np.full(64, CANARY, np.uint32)
    cnt = np.full(16, CANARY, np.uint32)
    src, keep = host_call(c)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert shim.wq_test_tick_sends_host(ctypes.byref(src), p(po), p(fo), c.n_elems, p(cnt), None) == 1
    assert (po == CANARY).all() and (fo == CANARY).all() and (cnt == CANARY).all()
