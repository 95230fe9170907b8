"""The interest diff's arithmetic (csrc/csr_diff_ops.hpp) on the CPU, through
tests/cpp/csr_diff_host_shim.hip: clamped row bounds, the row of an ordinal, the membership search
and the rows' output offsets, in the rows / prefix / flag / prefix / emit shape the kernels use, byte
for byte against worldql_server_amd/interest.py. No GPU needed (the GPU instance:
tests/test_gpu_csr_diff.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi, interest

from test_csr_diff_host import cases, descending_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC0FFEE11

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("csr_diff_shim") / "libcsrdiffshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "csr_diff_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.wq_test_csr_diff_host.restype = None
    lib.wq_test_csr_diff_host.argtypes = [sz, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp]
    return lib


def shim_diff(lib, oo, op, no, npr, with_left=True, ent_cap=None, left_cap=None):
    """The shim on exactly sized arrays with canary words behind every output."""
    oo, op, no, npr = (np.ascontiguousarray(a, np.uint32) for a in (oo, op, no, npr))
    M = len(oo) - 1
    ce = len(npr) if ent_cap is None else ent_cap
    cl = (len(op) if left_cap is None else left_cap) if with_left else 0
    eo = np.full(M + 2, CANARY, np.uint32)
    lo = np.full(M + 2, CANARY, np.uint32)
    ep = np.full(ce + 8, CANARY, np.uint32)
    lp = np.full(cl + 8, CANARY, np.uint32)
    cnt = np.zeros(4, np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.wq_test_csr_diff_host(M, p(oo), p(op), len(op), p(no), p(npr), len(npr), p(eo), p(ep), ce,
                              p(lo) if with_left else None, p(lp) if with_left else None, cl, p(cnt))
    assert eo[M + 1] == CANARY and lo[M + 1] == CANARY
    assert (ep[ce:] == CANARY).all() and (lp[cl:] == CANARY).all()
    return eo[:M + 1], ep[:ce], lo[:M + 1], lp[:cl], [int(x) for x in cnt]


def _exact(got, want):
    eo, ep, lo, lp, cnt = got
    w_eo, w_ep, w_lo, w_lp = want
    assert cnt[0] == len(w_ep) and cnt[1] == len(w_lp) and cnt[2] == 0
    assert eo.tobytes() == w_eo.tobytes() and lo.tobytes() == w_lo.tobytes()
    assert ep[:cnt[0]].tobytes() == w_ep.tobytes() and lp[:cnt[1]].tobytes() == w_lp.tobytes()


@pytest.mark.parametrize("name", sorted(cases()))
def test_kernel_arithmetic_matches_host_reference(shim, name):
    oo, op, no, npr = cases()[name]
    got = shim_diff(shim, oo, op, no, npr)
    _exact(got, interest.csr_diff_np(oo, op, no, npr))
    assert got[4][3] == 0


def test_left_side_off_and_capacity(shim):
    oo, op, no, npr = cases()["random_2000"]
    w_eo, w_ep, w_lo, w_lp = interest.csr_diff_np(oo, op, no, npr)
    eo, ep, lo, lp, cnt = shim_diff(shim, oo, op, no, npr, with_left=False)
    assert cnt[:3] == [len(w_ep), 0, 0] and eo.tobytes() == w_eo.tobytes() and ep[:cnt[0]].tobytes() == w_ep.tobytes()
    assert (lo == CANARY).all()
    E = len(w_ep)
    for cap in (E - 1, 0):
        eo, ep, lo, lp, cnt = shim_diff(shim, oo, op, no, npr, ent_cap=cap)
        assert cnt[0] == E and cnt[2] == abi.DIFF_OVERFLOW_ENTERED
        assert eo.tobytes() == w_eo.tobytes() and ep.tobytes() == w_ep[:cap].tobytes()
        assert lo.tobytes() == w_lo.tobytes() and lp[:cnt[1]].tobytes() == w_lp.tobytes()


def test_offsets_outside_their_array_are_clamped(shim):
    oo, op, no, npr = cases()["rows_513"]
    # a truncated tick: the new peers array ends before new_offsets[n_rows]
    cap = int(no[-1]) * 2 // 3
    c_no, c_np, cut = interest.clamp_csr_np(no, npr[:cap], cap)
    assert cut
    got = shim_diff(shim, oo, op, no, npr[:cap].copy())
    _exact(got, interest.csr_diff_np(oo, op, c_no, c_np))
    assert got[4][3] == abi.DIFF_ERROR_ROWS
    # one row with offsets[m + 1] < offsets[m], on the old side
    bad, bad_p = descending_pair(oo, op)
    c_oo, c_op, cut = interest.clamp_csr_np(bad, bad_p)
    assert cut and len(c_op) == len(op) + 3
    got = shim_diff(shim, bad, bad_p, no, npr, left_cap=len(bad_p) + 3)
    _exact(got, interest.csr_diff_np(c_oo, c_op, no, npr))
    assert got[4][3] == abi.DIFF_ERROR_ROWS
    # offsets of 2^32 - 1 from row 300 on, the array ending where row 300 began: nothing outside is read
    wild = no.copy()
    wild[300:] = 0xFFFFFFFF
    short = npr[:int(no[300])].copy()
    c_no, c_np, cut = interest.clamp_csr_np(wild, short)
    assert cut and int(c_no[-1]) == len(short)
    got = shim_diff(shim, oo, op, wild, short)
    _exact(got, interest.csr_diff_np(oo, op, c_no, c_np))
    assert got[4][3] == abi.DIFF_ERROR_ROWS
