"""The per-peer send lists' arithmetic (csrc/peer_major_ops.hpp) on the CPU, through
tests/cpp/peer_major_host_shim.hip: the row that covers an element, the clamped bounds, the connected
test, the key with its sentinel, the key width and the per-peer lower bound, in the expand / stable
sort / lower bound shape the kernels use, byte for byte against worldql_server_amd/interest.py
(peer_major_np). No GPU needed (the GPU instance: tests/test_gpu_peers.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_peer_major_host import cases, exact_names, hostile_names, want, well_formed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC0FFEE11

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("peer_major_shim") / "libpeermajorshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "peer_major_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.wq_test_peer_major_host.restype = None
    lib.wq_test_peer_major_host.argtypes = [vp, vp, sz, sz, vp, ctypes.c_uint32, vp, vp]
    return lib


def shim_peer_major(lib, c):
    """The shim on exactly sized inputs with canary words behind both outputs: (peer_offsets, msgs_out)."""
    n_pairs = len(c.peers)
    po = np.full(c.n_peers + 1 + 8, CANARY, np.uint32)
    mo = np.full(n_pairs + 8, CANARY, np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.wq_test_peer_major_host(p(c.offsets) if c.n_msgs else None, p(c.peers), c.n_msgs, n_pairs,
                                p(c.connected) if c.connected is not None else None, c.n_peers, p(po), p(mo))
    assert (po[c.n_peers + 1:] == CANARY).all() and (mo[n_pairs:] == CANARY).all()
    return po[:c.n_peers + 1], mo[:n_pairs]


@pytest.mark.parametrize("name", exact_names())
def test_kernel_arithmetic_matches_host_reference(shim, name):
    c = cases()[name]
    po, mo = shim_peer_major(shim, c)
    w_po, w_rows = want(name)
    assert po.tobytes() == w_po.tobytes()
    assert mo[:len(w_rows)].tobytes() == w_rows.tobytes()
    well_formed(c, po, mo)


@pytest.mark.parametrize("name", hostile_names())
def test_hostile_offsets_stay_well_formed(shim, name):
    c = cases()[name]
    po, mo = shim_peer_major(shim, c)
    well_formed(c, po, mo)
    again = shim_peer_major(shim, c)
    assert po.tobytes() == again[0].tobytes() and mo.tobytes() == again[1].tobytes()
