"""The follow kernels' per-peer arithmetic (csrc/follow_ops.hpp) on the CPU, through
tests/cpp/follow_host_shim.hip: packed axis masks, closed-form op counts and the decode of an op's
ordinal, in the count / prefix / search shape the kernels use, byte for byte against
worldql_server_amd/follow.py. No GPU needed (the GPU instance: tests/test_gpu_follow.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi, follow

from test_follow_host import edge_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("follow_shim") / "libfollowshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-fPIC", "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "follow_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    lib.wq_test_follow_ops_host.restype = ctypes.c_size_t
    lib.wq_test_follow_ops_host.argtypes = [vp, vp, vp, vp, ctypes.c_size_t, ctypes.c_uint16, ctypes.c_uint32, vp,
                                            ctypes.c_size_t, vp]
    return lib


def shim_ops(lib, ow, old, nw, new, s, reach):
    ow = np.ascontiguousarray(ow, np.uint32)
    nw = np.ascontiguousarray(nw, np.uint32)
    old = np.ascontiguousarray(old, np.float64)
    new = np.ascontiguousarray(new, np.float64)
    n = len(nw)
    cap = 2 * (2 * reach + 1) ** 3 * n
    out = np.zeros(max(cap, 1), abi.OP_DTYPE)
    un = ctypes.c_uint64()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    total = lib.wq_test_follow_ops_host(p(ow), p(old), p(nw), p(new), n, s, reach, p(out), cap, ctypes.byref(un))
    assert total <= cap
    return out[:total], un.value


@pytest.mark.parametrize("cube_size", [16, 10])
@pytest.mark.parametrize("reach", [0, 1, 2])
def test_kernel_arithmetic_matches_host_reference_on_edges(shim, cube_size, reach):
    ow, old, nw, new = edge_cases()
    want = follow.follow_ops_np(ow, old, nw, new, cube_size, reach)
    got, n_unsub = shim_ops(shim, ow, old, nw, new, cube_size, reach)
    assert len(got) == len(want)
    assert n_unsub == int((want["kind"] == abi.OP_UNSUBSCRIBE).sum())
    assert got.tobytes() == want.tobytes()


def test_kernel_arithmetic_matches_host_reference_on_moves(shim):
    rng = np.random.default_rng(11)
    n = 3000
    old = rng.uniform(-100.0, 100.0, (n, 3))
    new = old + rng.uniform(-20.0, 20.0, (n, 3))
    ow = np.zeros(n, np.uint32)
    nw = np.where(rng.uniform(size=n) < 0.1, 1, 0).astype(np.uint32)
    ow[rng.uniform(size=n) < 0.05] = abi.WORLD_INVALID
    nw[rng.uniform(size=n) < 0.05] = abi.WORLD_INVALID
    for reach in (1, 2):
        want = follow.follow_ops_np(ow, old, nw, new, 16, reach)
        got, _ = shim_ops(shim, ow, old, nw, new, 16, reach)
        assert got.tobytes() == want.tobytes() and len(want) > n
