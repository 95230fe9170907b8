"""The send budgets' arithmetic (csrc/budget_ops.hpp) on the CPU, through
tests/cpp/peer_budget_host_shim.hip: the clamped lengths and the ordinal space, the key with its NaN /
missing rule and u64 image, the class of a row, the rank by counting, the radix select's digit, match
and pick tests, the keep predicate and the flag-word prefix, in the passes the kernels use, byte for
byte against worldql_server_amd/interest.py (peer_budget_np). No GPU needed (the GPU instance:
tests/test_gpu_peer_budget.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi

from test_peer_budget_host import CHUNK, DIGIT_BITS, SHORT, TILE, cases, exact_names, hostile_names, want, well_formed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC0FFEE11

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("peer_budget_shim") / "libpeerbudgetshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                           "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "peer_budget_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.wq_test_peer_budget_host.restype = None
    lib.wq_test_peer_budget_host.argtypes = [vp, vp, u32, sz, vp, sz, vp, sz, u32, vp, vp, vp, vp]
    lib.wq_test_budget_short.restype = u32
    lib.wq_test_budget_digit_bits.restype = u32
    lib.wq_test_budget_tile.restype = u32
    lib.wq_test_budget_tiles.restype = u32
    return lib


def shim_peer_budget(lib, c):
    """The shim on exactly sized inputs with canary words behind both outputs:
    (out_offsets, out_msgs[n_in], counters)."""
    n_in = len(c.msgs)
    oo = np.full(c.n_peers + 1 + 8, CANARY, np.uint32)
    om = np.full(n_in + 8, CANARY, np.uint32)
    cnt = np.zeros(4, np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
    lib.wq_test_peer_budget_host(p(c.offsets), p(c.msgs), c.n_peers, n_in, p(c.msg_pos), len(c.msg_pos), p(c.peer_pos),
                                 len(c.peer_pos), c.k, p(c.budget), p(oo), p(om), p(cnt))
    assert (oo[c.n_peers + 1:] == CANARY).all() and (om[n_in:] == CANARY).all()
    counters = dict(zip(abi.BUDGET_COUNTERS_DTYPE.names, (int(v) for v in cnt)))
    assert (om[int(counters["n_kept"]):] == CANARY).all(), "written behind out_msgs[n_kept)"
    return oo[:c.n_peers + 1], om[:n_in], counters


def test_thresholds_are_the_ones_the_cases_straddle(shim):
    assert shim.wq_test_budget_short() == SHORT and shim.wq_test_budget_digit_bits() == DIGIT_BITS
    assert shim.wq_test_budget_tile() == TILE and shim.wq_test_budget_tile() * shim.wq_test_budget_tiles() == CHUNK


@pytest.mark.parametrize("name", exact_names())
def test_kernel_arithmetic_matches_host_reference(shim, name):
    c = cases()[name]
    oo, om, cnt = shim_peer_budget(shim, c)
    w_oo, w_om, w_cnt = want(name)
    assert oo.tobytes() == w_oo.tobytes()
    assert om[:len(w_om)].tobytes() == w_om.tobytes()
    assert cnt == w_cnt
    well_formed(c, oo, om[:cnt["n_kept"]], cnt)


@pytest.mark.parametrize("name", hostile_names())
def test_hostile_offsets_stay_well_formed(shim, name):
    c = cases()[name]
    oo, om, cnt = shim_peer_budget(shim, c)
    well_formed(c, oo, om[:cnt["n_kept"]], cnt)
    assert cnt["error"] & abi.BUDGET_ERROR_ROWS
    again = shim_peer_budget(shim, c)
    assert oo.tobytes() == again[0].tobytes() and om.tobytes() == again[1].tobytes() and cnt == again[2]
    # the header's rule for overlapping rows (walked up to n_in elements) is the host definition's
    w_oo, w_om, w_cnt = want(name)
    assert oo.tobytes() == w_oo.tobytes() and om[:len(w_om)].tobytes() == w_om.tobytes() and cnt == w_cnt
