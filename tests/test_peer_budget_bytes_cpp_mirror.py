"""The byte budgets' arithmetic (csrc/budget_ops.hpp) on the CPU, through
tests/cpp/peer_budget_bytes_host_shim.hip: the size of an element, the class of a row from its total, the
byte scans' terms, the weighted rank in a short row, the weighted radix select on u64 bins that are
zeroed on the pick, the keep predicate and the offsets from the keep words, in the passes the kernels
use, byte for byte against worldql_server_amd/interest.py (peer_budget_bytes_np). No GPU needed (the
GPU instance: tests/test_gpu_peer_budget_bytes.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi

from test_peer_budget_bytes_host import CHUNK, DIGIT_BITS, SHORT, TILE, cases, exact_names, hostile_names, want, well_formed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC0FFEE11
CANARY64 = 0xC0FFEE11C0FFEE11

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("peer_budget_bytes_shim") / "libpeerbudgetbytesshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                           "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "peer_budget_bytes_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp, sz, u32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64
    lib.wq_test_peer_budget_bytes_host.restype = u64
    lib.wq_test_peer_budget_bytes_host.argtypes = [vp, vp, u32, sz, vp, vp, sz, vp, sz, u64, vp, vp, vp, vp, vp, vp]
    for f in ("short", "digit_bits", "tile", "tiles"):
        getattr(lib, "wq_test_budget_bytes_" + f).restype = u32
    lib.wq_test_budget_bytes_slots.restype = sz
    lib.wq_test_budget_bytes_slots.argtypes = [sz]
    return lib


def shim_call(lib, c, hist=None, with_bytes=True):
    """The shim on exactly sized inputs with canary words behind the outputs: (out_offsets, out_msgs[n_in],
    out_bytes, counters, hist). `hist`: the histograms of an earlier call of the same n_in."""
    n_in = len(c.msgs)
    if hist is None:
        hist = np.zeros(lib.wq_test_budget_bytes_slots(n_in) * (1 << DIGIT_BITS), np.uint64)
    oo = np.full(c.n_peers + 1 + 8, CANARY, np.uint32)
    om = np.full(n_in + 8, CANARY, np.uint32)
    ob = np.full(c.n_peers + 8, CANARY64, np.uint64)
    cnt = np.zeros(6, np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
    dirty = lib.wq_test_peer_budget_bytes_host(p(c.offsets), p(c.msgs), c.n_peers, n_in, p(c.msg_pos), p(c.msg_size),
                                               len(c.msg_pos), p(c.peer_pos), len(c.peer_pos), c.w, p(c.budget), p(hist),
                                               p(oo), p(om), ob.ctypes.data_as(ctypes.c_void_p) if with_bytes else None,
                                               p(cnt))
    assert dirty == 0, "the histograms were not zero when the call began"
    assert not hist.any(), "the picks left a bin non-zero"
    assert (oo[c.n_peers + 1:] == CANARY).all() and (om[n_in:] == CANARY).all()
    assert (ob[c.n_peers if with_bytes else 0:] == CANARY64).all()
    counters = dict(zip(abi.BUDGET_BYTES_COUNTERS_DTYPE.names, (int(v) for v in cnt)))
    assert (om[int(counters["n_kept"]):] == CANARY).all(), "written behind out_msgs[n_kept)"
    return oo[:c.n_peers + 1], om[:n_in], ob[:c.n_peers], counters, hist


def same(name, got):
    oo, om, ob, cnt = got[:4]
    w_oo, w_om, w_ob, w_cnt = want(name)
    assert oo.tobytes() == w_oo.tobytes()
    assert om[:len(w_om)].tobytes() == w_om.tobytes()
    assert ob.tobytes() == w_ob.tobytes()
    assert cnt == w_cnt
    well_formed(cases()[name], oo, om[:cnt["n_kept"]], ob, cnt)


def test_thresholds_are_the_ones_the_cases_straddle(shim):
    assert shim.wq_test_budget_bytes_short() == SHORT and shim.wq_test_budget_bytes_digit_bits() == DIGIT_BITS
    assert shim.wq_test_budget_bytes_tile() == TILE
    assert shim.wq_test_budget_bytes_tile() * shim.wq_test_budget_bytes_tiles() == CHUNK
    assert abi.BUDGET_BYTES_COUNTERS_DTYPE.itemsize == 40


@pytest.mark.parametrize("name", exact_names())
def test_kernel_arithmetic_matches_host_reference(shim, name):
    """Twice on the same histograms: the second call must find every bin zero."""
    c = cases()[name]
    first = shim_call(shim, c)
    same(name, first)
    same(name, shim_call(shim, c, hist=first[4]))
    no_bytes = shim_call(shim, c, with_bytes=False)
    assert no_bytes[0].tobytes() == first[0].tobytes() and no_bytes[1].tobytes() == first[1].tobytes()


@pytest.mark.parametrize("name", hostile_names())
def test_hostile_offsets_stay_well_formed(shim, name):
    c = cases()[name]
    first = shim_call(shim, c)
    assert first[3]["error"] & abi.BUDGET_ERROR_ROWS
    same(name, first)     # the header's rule for overlapping rows (walked up to n_in elements) is the definition's
    same(name, shim_call(shim, c, hist=first[4]))
