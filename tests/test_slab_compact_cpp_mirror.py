"""The slab compaction's arithmetic (csrc/compact_ops.hpp with csrc/pack_ops.hpp) on the CPU, through
tests/cpp/slab_compact_host_shim.hip: terms by quads, scan, decision, entries and the copy in the kernel's tiles,
windows and block runs — byte for byte against worldql_server_amd/records.py (slab_compact_np), on exactly
sized arrays with guard bytes around both slabs. No GPU needed (the GPU instance: tests/test_gpu_slab_compact.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi, records

from test_slab_compact_host import CASES, IDS, E, by_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
GUARD, FILL = 64, 0xC5
CSIZE = abi.SLAB_COMPACT_COUNTERS_DTYPE.itemsize

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("slab_compact_shim") / "libslabcompactshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-o", out, os.path.join(ROOT, "tests", "cpp", "slab_compact_host_shim.hip")])
    lib = ctypes.CDLL(out)
    lib.wq_test_slab_compact_host.restype = ctypes.c_uint64
    lib.wq_test_slab_compact_host.argtypes = [ctypes.POINTER(abi.SlabView), ctypes.POINTER(abi.SlabView), ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_uint64]
    lib.wq_test_slab_compact_sizes.restype = ctypes.c_uint32
    return lib


def aligned(n_bytes, content=None):
    """FILL bytes with GUARD bytes on both sides, the inner part 16-byte aligned and exactly n_bytes: (buffer, inner view)."""
    raw = np.full(n_bytes + 2 * GUARD + 16, FILL, np.uint8)
    at = GUARD + (-(raw.ctypes.data + GUARD)) % 16
    inner = raw[at:at + n_bytes]
    if content is not None:
        inner[:] = content
    return raw, inner


def guards_ok(raw, inner):
    a = inner.ctypes.data - raw.ctypes.data
    return bool((raw[:a] == FILL).all() and (raw[a + inner.size:] == FILL).all())


CURSOR0 = 0x1234


def shim_call(lib, case, n_entries, n_bytes, blocks=0, counters=True):
    """(entries, payload, cursor, counters or None, fast tiles, guards intact and inputs unchanged) from the shim."""
    src_e, src_b = case.entries.view(np.uint8).reshape(-1), case.payload
    sraw, sent = aligned(src_e.size, src_e)
    braw, spay = aligned(src_b.size, src_b)
    eraw, ent = aligned(64 * n_entries)
    praw, pay = aligned(n_bytes)
    cur = np.array([CURSOR0], np.uint64)
    cnt = np.full(CSIZE + 8, FILL, np.uint8)
    p = lambda a: a.ctypes.data if a.size else None   # noqa: E731
    src = abi.SlabView(entries=p(sent), n_entries=len(case.entries), payload=p(spay), n_payload_bytes=src_b.size)
    dst = abi.SlabView(entries=p(ent), n_entries=n_entries, payload=p(pay), n_payload_bytes=n_bytes)
    fast = lib.wq_test_slab_compact_host(ctypes.byref(src), ctypes.byref(dst), cur.ctypes.data,
                                         cnt.ctypes.data if counters else None, blocks)
    ok = all(guards_ok(r, v) for r, v in ((sraw, sent), (braw, spay), (eraw, ent), (praw, pay))) and bool((cnt[-8:] == FILL).all())
    ok = ok and np.array_equal(sent, src_e) and np.array_equal(spay, src_b)
    return (ent.view(E).copy(), pay.copy(), int(cur[0]), records.slab_compact_counters(cnt[:-8]) if counters else None, fast, ok)


def want(case, n_entries, n_bytes):
    ent = np.frombuffer(bytes([FILL]) * (64 * n_entries), dtype=E).copy()
    return records.slab_compact_np(case.entries, case.payload, n_entries, n_bytes, dst=(ent, np.full(n_bytes, FILL, np.uint8), CURSOR0))


def same(got, exp):
    return (got[0].tobytes() == exp[0].tobytes() and np.array_equal(got[1], exp[1]) and got[2] == exp[2]
            and (got[3] is None or got[3] == exp[3]) and got[5])


def test_struct_sizes(shim):
    assert shim.wq_test_slab_compact_sizes() == 64 | 40 << 8 | 16 << 16


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matches_definition(shim, case):
    ne, nb = case.need()
    for n_entries, n_bytes in ((ne, nb), (len(case.entries) + 3, nb + 1500)):
        exp = want(case, n_entries, n_bytes)
        assert exp[3]["overflow"] == 0 and exp[2] == nb
        for blocks in (0, 1, 3):
            assert same(shim_call(shim, case, n_entries, n_bytes, blocks), exp), (n_entries, n_bytes, blocks)
    assert same(shim_call(shim, case, ne, nb, counters=False), want(case, ne, nb))


def test_whole_tile_path(shim):
    big = by_name("two 1 MiB payloads")
    got = shim_call(shim, big, *big.need())
    assert got[4] >= 2 * 1022 and same(got, want(big, *big.need()))
    small = by_name("0..40")
    assert shim_call(shim, small, *small.need())[4] == 0


def test_a_dead_run_costs_the_copy_no_windows(shim):
    """The copy's elements are the live entries: four of them around 100,000 dead handles are one window's work,
    and the result is the one of the same entries with 64 dead handles between them."""
    far, near = by_name("runs of 100000 dead"), by_name("runs of 64 dead")
    a, b = shim_call(shim, far, *far.need()), shim_call(shim, near, *near.need())
    assert same(a, want(far, *far.need())) and same(b, want(near, *near.need()))
    assert a[2] == b[2] == 4 * 9 and a[3]["n_live"] == 4


@pytest.mark.parametrize("case", [c for c in CASES if c.need()[0]], ids=lambda c: c.name)
def test_all_or_nothing(shim, case):
    ne, nb = case.need()
    trials = [(ne - 1, nb), (0, nb)]
    if nb:
        trials += [(ne, nb - 1), (ne + 1, nb // 2), (ne - 1, nb - 1), (ne, 0), (0, 0)]
    for n_entries, n_bytes in trials:
        exp = want(case, n_entries, n_bytes)
        assert exp[3]["overflow"] and exp[2] == CURSOR0
        assert same(shim_call(shim, case, n_entries, n_bytes), exp), (n_entries, n_bytes)


def test_every_destination_size_of_a_small_case(shim):
    case = by_name("65 entries")
    ne, nb = case.need()
    assert nb > 300 and ne > 40
    for n_bytes in range(0, nb + 3):
        assert same(shim_call(shim, case, ne, n_bytes, blocks=n_bytes % 3), want(case, ne, n_bytes)), n_bytes
    for n_entries in range(0, ne + 3):
        assert same(shim_call(shim, case, n_entries, nb, blocks=n_entries % 3), want(case, n_entries, nb)), n_entries


def test_hostile_and_shared_ranges(shim):
    for name in ("hostile ranges", "shared and overlapping ranges"):
        case = by_name(name)
        exp = want(case, *case.need())
        assert same(shim_call(shim, case, *case.need()), exp)
    assert want(by_name("hostile ranges"), 9, 64)[3]["error"] == abi.SLAB_COMPACT_ERROR_RANGE


def test_idempotent(shim):
    for name in ("257 entries", "around a tile", "hostile ranges", "descending arena order"):
        case = by_name(name)
        ne, nb = case.need()
        first = shim_call(shim, case, ne, nb)

        class Canon:
            entries, payload = first[0], first[1]
        again = shim_call(shim, Canon, ne, nb, blocks=2)
        assert again[0].tobytes() == first[0].tobytes() and np.array_equal(again[1], first[1]) and again[2] == first[2] == nb
