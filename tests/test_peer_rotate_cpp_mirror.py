"""The fair share's arithmetic (csrc/rotate_ops.hpp) on the CPU, through
tests/cpp/peer_rotate_host_shim.hip: the occurrence rule, the bounds in the kept row, the folded scan
terms of a row, the cyclic rank, the running bytes, the chosen predicate and the error rules, in the
passes and tilings the kernels use, byte for byte against worldql_server_amd/interest.py
(peer_rotate_np) over the whole case list, with canary words behind every output. No GPU needed (the
GPU instance: tests/test_gpu_peer_rotate.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi

from test_peer_rotate_host import GRANULE, TILE, cases, exact_names, hostile_names, rows_ascend, want, well_formed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC0FFEE11
CANARY64 = 0xC0FFEE11C0FFEE11
NAMES = [n for n in abi.ROTATE_COUNTERS_DTYPE.names if n != "pad_"]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("peer_rotate_shim") / "libpeerrotateshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                           "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "peer_rotate_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp, sz, u32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64
    lib.wq_test_peer_rotate_host.restype = None
    lib.wq_test_peer_rotate_host.argtypes = [vp, vp, u32, sz, vp, vp, sz, vp, sz, ctypes.c_int, u32, vp, u64, vp, vp, vp,
                                             vp, vp, vp]
    lib.wq_test_rotate_granule.restype = u32
    lib.wq_test_rotate_tile.restype = u32
    return lib


def shim_peer_rotate(lib, c):
    """The shim on exactly sized inputs with canary words behind every output:
    (out_offsets, out_msgs[n_out], out_bytes or None, cursor after, counters)."""
    n_in, sizes = len(c.msgs), c.msg_size is not None
    oo = np.full(c.n_peers + 1 + 8, CANARY, np.uint32)
    om = np.full(n_in + 8, CANARY, np.uint32)
    ob = np.full(c.n_peers + 8, CANARY64, np.uint64)
    cursor = np.concatenate([c.cursor, np.full(8, CANARY, np.uint32)])
    cnt = np.full(9 + 8, CANARY64, np.uint64)
    inputs = [a.copy() for a in (c.offsets, c.msgs, c.koffsets, c.kmsgs)]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
    lib.wq_test_peer_rotate_host(p(inputs[0]), p(inputs[1]), c.n_peers, n_in, p(inputs[2]), p(inputs[3]), len(c.kmsgs),
                                 p(c.msg_size), len(c.msg_size) if sizes else 0, int(sizes), c.r, p(c.extra), c.v,
                                 p(c.extra_bytes), p(cursor), p(oo), p(om), p(ob) if sizes else None, p(cnt))
    for a, b in zip(inputs, (c.offsets, c.msgs, c.koffsets, c.kmsgs)):
        assert a.tobytes() == b.tobytes(), "an input was written"
    counters = dict(zip(NAMES, (int(x) for x in cnt[:9])))
    assert (cnt[9:] == CANARY64).all() and (oo[c.n_peers + 1:] == CANARY).all() and (cursor[c.n_peers:] == CANARY).all()
    assert counters["n_out"] <= n_in and (om[counters["n_out"]:] == CANARY).all(), "written behind out_msgs[n_out)"
    assert (ob[c.n_peers if sizes else 0:] == CANARY64).all()
    return oo[:c.n_peers + 1], om[:counters["n_out"]], ob[:c.n_peers] if sizes else None, cursor[:c.n_peers], counters


def same_as_definition(name, got):
    oo, om, ob, cursor, cnt = got
    w_oo, w_om, w_ob, w_cursor, w_cnt = want(name)
    assert cnt == w_cnt
    assert oo.tobytes() == w_oo.tobytes() and om.tobytes() == w_om.tobytes()
    assert cursor.tobytes() == w_cursor.tobytes()
    assert (ob is None) == (w_ob is None) and (ob is None or ob.tobytes() == w_ob.tobytes())


def test_thresholds_are_the_ones_the_cases_straddle(shim):
    assert shim.wq_test_rotate_granule() == GRANULE and shim.wq_test_rotate_tile() == TILE


@pytest.mark.parametrize("name", exact_names())
def test_kernel_arithmetic_matches_host_reference(shim, name):
    c = cases()[name]
    got = shim_peer_rotate(shim, c)
    same_as_definition(name, got)
    well_formed(c, got[0], got[1], got[3], got[4])


@pytest.mark.parametrize("name", hostile_names())
def test_hostile_input_stays_well_formed(shim, name):
    c = cases()[name]
    got = shim_peer_rotate(shim, c)
    well_formed(c, got[0], got[1], got[3], got[4])
    again = shim_peer_rotate(shim, c)
    for a, b in zip(got[:4], again[:4]):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    assert got[4] == again[4]
    if rows_ascend(c):      # the header's row rules are the definition's: the bytes are exact
        same_as_definition(name, got)
