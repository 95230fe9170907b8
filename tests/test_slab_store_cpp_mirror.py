"""The record payload slab's arithmetic (csrc/slab_ops.hpp with csrc/pack_ops.hpp) on the CPU, through
tests/cpp/slab_store_host_shim.hip: sizes, scan, decision, entries and the copy in the kernel's tiles, windows
and block runs — byte for byte against worldql_server_amd/records.py (slab_store_np), on exactly sized arrays
with guard bytes around the slab. No GPU needed (the GPU instance: tests/test_gpu_slab_store.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi, records

from test_slab_store_host import CASES, IDS, E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
GUARD, FILL = 64, 0xC5

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("slab_shim") / "libslabshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-o", out, os.path.join(ROOT, "tests", "cpp", "slab_store_host_shim.hip")])
    lib = ctypes.CDLL(out)
    lib.wq_test_slab_store_host.restype = ctypes.c_uint64
    lib.wq_test_slab_store_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_size_t, ctypes.POINTER(abi.SlabView), ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_uint64]
    lib.wq_test_slab_sizes.restype = ctypes.c_uint32
    return lib


def aligned(n_bytes):
    """FILL bytes with GUARD bytes on both sides, the inner part 16-byte aligned: (buffer, inner view)."""
    raw = np.full(n_bytes + 2 * GUARD + 16, FILL, np.uint8)
    at = GUARD + (-(raw.ctypes.data + GUARD)) % 16
    return raw, raw[at:at + n_bytes]


def shim_call(lib, case, n_entries, n_bytes, cursor, blocks=0, counters=True):
    """(entries, payload, cursor, counters or None, fast tiles, guards intact) from the shim."""
    ops, refs, frames, fo = (np.array(a, copy=True) for a in case.arrays())
    eraw, ent = aligned(64 * n_entries)
    praw, pay = aligned(n_bytes)
    cur = np.array([cursor], np.uint64)
    cnt = np.full(abi.SLAB_COUNTERS_DTYPE.itemsize + 8, FILL, np.uint8)
    view = abi.SlabView(entries=ent.ctypes.data if n_entries else None, n_entries=n_entries,
                        payload=pay.ctypes.data if n_bytes else None, n_payload_bytes=n_bytes)
    p = lambda a: a.ctypes.data if a.size else None   # noqa: E731
    fast = lib.wq_test_slab_store_host(p(ops), p(refs), len(ops), p(frames), fo.ctypes.data, len(fo) - 1, ctypes.byref(view),
                                       cur.ctypes.data, cnt.ctypes.data if counters else None, blocks)
    inner = lambda raw, v: (v.ctypes.data - raw.ctypes.data, v.ctypes.data - raw.ctypes.data + v.size)   # noqa: E731
    guards = True
    for raw, v in ((eraw, ent), (praw, pay)):
        a, b = inner(raw, v)
        guards &= bool((raw[:a] == FILL).all() and (raw[b:] == FILL).all())
    guards &= bool((cnt[-8:] == FILL).all())
    return (ent.view(E).copy(), pay.copy(), int(cur[0]), records.slab_counters(cnt[:-8]) if counters else None, fast, guards)


def want(case, n_entries, n_bytes, cursor):
    ent = np.frombuffer(bytes([FILL]) * (64 * n_entries), dtype=E).copy()
    return records.slab_store_np(*case.arrays(), ent, np.full(n_bytes, FILL, np.uint8), cursor)


def same(got, exp):
    return (got[0].tobytes() == exp[0].tobytes() and np.array_equal(got[1], exp[1]) and got[2] == exp[2]
            and (got[3] is None or got[3] == exp[3]) and got[5])


def test_struct_sizes(shim):
    assert shim.wq_test_slab_sizes() == 64 | 32 << 8 | 56 << 16


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("cursor", [0, 5, 16, 1019, 1024, 2047])
def test_matches_definition(shim, case, cursor):
    ne, nb = case.need()
    for n_entries, n_bytes in ((ne, cursor + nb), (ne + 2, cursor + nb + 1500)):
        exp = want(case, n_entries, n_bytes, cursor)
        assert exp[3]["overflow"] == 0
        for blocks in (0, 1, 3):
            assert same(shim_call(shim, case, n_entries, n_bytes, cursor, blocks), exp), (n_entries, n_bytes, blocks)
    assert same(shim_call(shim, case, ne, cursor + nb, cursor, counters=False), want(case, ne, cursor + nb, cursor))


def test_whole_tile_path(shim):
    big = next(c for c in CASES if c.name == "1 MiB flex")
    ne, nb = big.need()
    got = shim_call(shim, big, ne, 9 + nb, 9)
    assert got[4] >= 1022 and same(got, want(big, ne, 9 + nb, 9))
    small = next(c for c in CASES if c.name == "0..40")
    assert shim_call(shim, small, *small.need(), 0)[4] == 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_all_or_nothing(shim, case):
    ne, nb = case.need()
    trials = [(ne, 3), (ne, 2)]
    if nb:
        trials += [(ne, 3 + nb - 1), (ne + 1, 3 + nb // 2)]
    if ne:
        trials += [(ne - 1, 3 + nb), (0, 3 + nb)]
    if nb and ne:
        trials += [(ne - 1, 3 + nb - 1), (0, 0)]
    for n_entries, n_bytes in trials:
        exp = want(case, n_entries, n_bytes, 3)
        assert exp[3]["overflow"] or not nb
        assert same(shim_call(shim, case, n_entries, n_bytes, 3), exp), (n_entries, n_bytes)


def test_every_capacity_of_a_small_case(shim):
    case = next(c for c in CASES if c.name == "one of each")
    ne, nb = case.need()
    for n_bytes in range(0, 11 + nb + 2):
        assert same(shim_call(shim, case, ne, n_bytes, 11), want(case, ne, n_bytes, 11)), n_bytes


def test_second_call_appends(shim):
    """Two shim calls into one slab: the second starts at the first's cursor, leaves the first's bytes and entries
    alone, and the slab is the definition's after both."""
    a, b = (next(c for c in CASES if c.name == n) for n in ("0..40", "around a tile"))
    (_, na), (_, nbb) = a.need(), b.need()
    ops, refs, frames, fo = (np.array(x, copy=True) for x in b.arrays())
    ops["handle"] += 100
    ent = np.frombuffer(bytes([FILL]) * (64 * 120), dtype=E).copy()
    e1, p1, c1, _ = records.slab_store_np(*a.arrays(), ent, np.full(na + nbb, FILL, np.uint8), 0)
    e2, p2, c2, cnt2 = records.slab_store_np(ops, refs, frames, fo, e1, p1, c1)
    assert c2 == na + nbb and np.array_equal(p2[:na], p1[:na]) and e2[100]["off"] == na
    eraw, dent = aligned(64 * 120)
    praw, dpay = aligned(na + nbb)
    cur = np.array([0], np.uint64)
    cnt = np.zeros(abi.SLAB_COUNTERS_DTYPE.itemsize, np.uint8)
    view = abi.SlabView(entries=dent.ctypes.data, n_entries=120, payload=dpay.ctypes.data, n_payload_bytes=na + nbb)
    for o, r, f, off in ([np.array(x, copy=True) for x in a.arrays()], [ops, refs, frames, fo]):
        shim.wq_test_slab_store_host(o.ctypes.data, r.ctypes.data, len(o), f.ctypes.data, off.ctypes.data, len(off) - 1,
                                     ctypes.byref(view), cur.ctypes.data, cnt.ctypes.data, 2)
    assert int(cur[0]) == c2 and records.slab_counters(cnt) == cnt2
    assert dent.tobytes() == e2.tobytes() and np.array_equal(dpay, p2)
    assert (eraw[:GUARD] == FILL).all() and (praw[-GUARD:] == FILL).all()
