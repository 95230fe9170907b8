"""The record reply builder's arithmetic (csrc/reply_ops.hpp with frame_ops.hpp and pack_ops.hpp, unchanged) on the
CPU, through tests/cpp/record_frames_host_shim.hip: the kernels' passes, any bracketing of the segmented scan, tiles,
windows and block runs, byte for byte against worldql_server_amd/frames.py (build_record_frames_np) with guard bytes
behind every output. No GPU needed (the GPU instance, on the same cases: tests/test_gpu_record_frames.py)."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi, frames

from test_record_frames_host import WORLDS, Slab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY, TAIL = 0xC5, 64
E = abi.SLAB_ENTRY_DTYPE

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


class RCase:
    """One call: a slab, rows of handles and the message part; the definition's result for any capacity."""

    def __init__(self, name, slab, rows, **kw):
        self.name = name
        self.entries, self.payload = slab.arrays() if isinstance(slab, Slab) else slab
        self.n = len(rows)
        self.row_offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
        self.handles = np.array([h for r in rows for h in r], np.uint32)
        rng = np.random.default_rng(len(name) + self.n)
        self.kw = dict(worlds=WORLDS, sender_uuid=rng.integers(0, 256, (self.n, 16), dtype=np.uint8),
                       world=(np.arange(self.n, dtype=np.uint32) * 5 + 1) % len(WORLDS), instruction=10, replication=0, pos=None,
                       param=None, param_offsets=None, flex=None, flex_offsets=None, msg_flags=None, world_bytes=None,
                       world_off=None, world_len=None, flags=0, n_payload_bytes=None)
        for k in ("row_offsets", "handles"):
            if k in kw:
                setattr(self, k, np.asarray(kw.pop(k), np.uint32))
        self.kw.update(kw)
        self._want = {}

    def want(self, capacity=None):
        if capacity not in self._want:
            k = dict(self.kw)
            self._want[capacity] = frames.build_record_frames_np(
                k.pop("worlds"), k.pop("sender_uuid"), k.pop("world"), self.row_offsets, self.handles, self.entries, self.payload,
                capacity=capacity, **k)
        return self._want[capacity]

    def marshal(self, put):
        """(abi.FramesSrc, abi.FramesRecSrc, table bytes, table offsets) with every array placed by put(uint8 array)
        -> address (None for an empty array unless `keep`)."""
        k = self.kw
        u8 = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt).view(np.uint8).reshape(-1)   # noqa: E731
        arr = lambda v, dt: None if v is None or np.isscalar(v) else u8(v, dt)                                    # noqa: E731
        P = lambda a, keep=False: None if a is None else put(a, keep)                                             # noqa: E731
        src = abi.FramesSrc(instruction=P(arr(k["instruction"], np.uint8)), instruction_all=int(k["instruction"]) if np.isscalar(k["instruction"]) else 0,
                            replication=P(arr(k["replication"], np.uint8)), replication_all=int(k["replication"]) if np.isscalar(k["replication"]) else 0,
                            sender_uuid=P(u8(k["sender_uuid"], np.uint8)), world=P(u8(k["world"], np.uint32)),
                            pos=P(u8(k["pos"], np.float64)), param=P(u8(k["param"], np.uint8), True),
                            param_offsets=P(u8(k["param_offsets"], np.uint64)), n_param_bytes=0 if k["param"] is None else len(k["param"]),
                            flex=P(u8(k["flex"], np.uint8), True), flex_offsets=P(u8(k["flex_offsets"], np.uint64)),
                            n_flex_bytes=0 if k["flex"] is None else len(k["flex"]), msg_flags=P(u8(k["msg_flags"], np.uint8)))
        nb = len(self.payload) if k["n_payload_bytes"] is None else k["n_payload_bytes"]
        view = abi.SlabView(entries=P(u8(self.entries, E)), n_entries=len(self.entries),
                            payload=P(u8(self.payload, np.uint8)) if k["n_payload_bytes"] is None else None, n_payload_bytes=nb)
        rec = abi.FramesRecSrc(row_offsets=P(u8(self.row_offsets, np.uint32), True), handles=P(u8(self.handles, np.uint32)),
                               n_handles=len(self.handles), slab=view, world_bytes=P(u8(k["world_bytes"], np.uint8), True),
                               world_off=P(u8(k["world_off"], np.uint64)), world_len=P(u8(k["world_len"], np.uint32)),
                               n_world_bytes=0 if k["world_bytes"] is None else len(k["world_bytes"]), flags=k["flags"])
        return src, rec


def payload_slab(lens, seed):
    """Records whose payloads of the given lengths lie back to back in the arena, shapes cycling."""
    rng = np.random.default_rng(seed)
    slab, hs = Slab(), []
    for i, n in enumerate(lens):
        shape = (1, 2, 3, 5, 6, 7)[i % 6]
        data = bytes(rng.integers(97, 123, n, dtype=np.uint8)) if shape & 1 else b""
        flex = bytes(rng.integers(0, 256, n if not shape & 1 else i % 7, dtype=np.uint8)) if shape & 2 else b""
        hs.append(slab.add(shape, world=i % len(WORLDS), data=data, flex=flex))
    return slab, hs


def cases():
    out = []
    slab = Slab()
    one = [slab.add(s, world=1 + s % 4, data=b"d" * (s % 3), flex=b"f" * (s % 5)) for s in range(8)]
    rng = np.random.default_rng(3)
    mixed = [one[int(v)] for v in rng.integers(0, 8, 6000)]
    rows = [mixed[:k] for k in (0, 1, 2, 3, 63, 64, 65, 257)]
    out.append(RCase("row lengths", slab, rows, pos=rng.integers(-9, 9, (len(rows), 3)).astype(np.float64), replication=2))
    out.append(RCase("one row of 5000", slab, [mixed[5:9], mixed[100:5100], [], mixed[:2]]))
    out.append(RCase("512 triples", slab, [[one[a], one[b], one[c]] for a, b, c in itertools.product(range(8), repeat=3)]))
    out.append(RCase("a repeated handle", slab, [[one[7], one[7], one[2], one[7]], [one[2], one[2]]]))
    s2, h2 = payload_slab(list(range(41)), 5)
    out.append(RCase("payloads 0..40", s2, [h2[:20], h2[20:], h2[::3]]))
    s3, h3 = payload_slab([1022, 1023, 1024, 1025, 1026, 4095, 4096, 4097], 6)
    out.append(RCase("payloads around tiles", s3, [h3[:5], h3[5:], h3[::-1]]))
    s4 = Slab()
    big = [s4.add(2, world=2, flex=bytes(np.random.default_rng(8).integers(0, 256, 1 << 20, dtype=np.uint8))),
           s4.add(1, world=3, data=bytes(np.random.default_rng(9).integers(97, 123, 1 << 20, dtype=np.uint8)))]
    out.append(RCase("two 1 MiB payloads", s4, [[big[0]], [], [big[1], big[0]]]))
    out.append(RCase("message fields", slab, [[one[3]], [], [one[5], one[0]], [one[6]], []], instruction=np.array([0, 10, 3, 10, 255], np.uint8),
                     replication=np.array([0, 1, 2, 0, 1], np.uint8), pos=np.arange(15.0).reshape(5, 3),
                     param=np.frombuffer(b"12345abc", np.uint8), param_offsets=np.array([0, 5, 5, 8, 8, 8], np.uint64),
                     flex=np.arange(40, dtype=np.uint8), flex_offsets=np.array([0, 0, 17, 17, 40, 40], np.uint64),
                     msg_flags=np.array([7, 5, 2, 0, 6], np.uint8)))
    out.append(RCase("nil sender and world bytes", slab, [[one[1], one[4]], [], [one[7]]], sender_uuid=None, world=None,
                     world_bytes=np.frombuffer(b"overworldnether", np.uint8), world_off=np.array([0, 9, 9], np.uint64),
                     world_len=np.array([9, 6, 0], np.uint32)))
    out.append(RCase("skip empty", slab, [[], [one[2]], [], []], flags=frames.SKIP_EMPTY))
    out.append(RCase("all rows empty", slab, [[], [], []], pos=np.ones((3, 3))))
    out.append(RCase("no messages", slab, []))
    # error bits 0 and 4 - 6 (1 - 3 are the flat builder's, below)
    bad = Slab()
    ok = bad.add(3, data=b"abc", flex=b"defg")
    dead = bad.add(7, data=b"xyz", flex=b"q", live=False)
    far = bad.add(1, world=77, data=b"zz")
    out.append(RCase("bits 0 and 4", bad, [[ok, 99, dead, far], [dead], [far, ok]], world=np.array([1, 44, 2], np.uint32)))
    out.append(RCase("bits 0 and 4, skip empty", bad, [[ok, 99, dead, far], [dead], [far, ok]], flags=frames.SKIP_EMPTY))
    ent, arena = bad.arrays()
    out.append(RCase("bit 5", (ent, arena[:5].copy()), [[ok, far], [ok]]))
    out.append(RCase("bit 5, no arena", (ent, arena[:0].copy()), [[ok, far], [ok]]))
    out.append(RCase("bit 6", bad, [[ok], [ok], [ok]], row_offsets=[2, 1, 7, 3], handles=[ok, far, ok, ok]))
    out.append(RCase("bit 6, overlapping rows", bad, [[ok], [ok], [ok]], row_offsets=[0, 3, 0, 3], handles=[ok, far, ok]))
    out.append(RCase("bits 1 and 2", slab, [[one[1]], [one[2]]], param=np.frombuffer(b"12", np.uint8), param_offsets=np.array([2, 1, 9], np.uint64),
                     flex=np.arange(4, dtype=np.uint8), flex_offsets=np.array([0, 9, 4], np.uint64)))
    out.append(RCase("world bytes out of range", slab, [[one[1]], [one[2]]], world_bytes=np.frombuffer(b"abc", np.uint8),
                     world_off=np.array([1, 2], np.uint64), world_len=np.array([2, 2], np.uint32)))
    return out


def small_case():
    """About 400 bytes of frames: one message with two records and an empty one."""
    slab = Slab()
    hs = [slab.add(7, world=4, data=b"hello", flex=b"\x01\x02\x03"), slab.add(1, world=1, data=b""), slab.add(7, world=2, data=b"x", flex=b"")]
    return RCase("small", slab, [hs[:2], []], world=np.array([1, 0], np.uint32))


def too_large_case():
    """The 2^30 rule through the sizing call: claimed lengths, no payload memory."""
    big = np.zeros(2, E)
    big["bits"], big["flex_len"], big["off"] = abi.SLAB_LIVE | abi.SLAB_FLEX, (1 << 30) - 200, [0, 1 << 30]
    return RCase("too large", (big, np.zeros(0, np.uint8)), [[0], [0, 1]], n_payload_bytes=1 << 31)


CASES = cases()
IDS = [c.name for c in CASES]


class ShimIn(ctypes.Structure):  # struct wq_test_recframes_in
    _fields_ = [("src", abi.FramesSrc), ("rec", abi.FramesRecSrc), ("table_bytes", ctypes.c_void_p), ("table_off", ctypes.c_void_p),
                ("n_table_bytes", ctypes.c_uint64), ("n_worlds", ctypes.c_uint32), ("scan_block", ctypes.c_uint32),
                ("blocks", ctypes.c_uint64)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("recframes_shim") / "librecframesshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-o", out, os.path.join(ROOT, "tests", "cpp", "record_frames_host_shim.hip")])
    lib = ctypes.CDLL(out)
    lib.wq_test_record_frames_host.restype = ctypes.c_uint64
    lib.wq_test_record_frames_host.argtypes = [ctypes.POINTER(ShimIn), ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.wq_test_recframes_sizes.restype = ctypes.c_uint32
    return lib


def shim_call(lib, case, capacity, scan_block=0, blocks=0, with_size=True, with_counters=True):
    """(frames[:bytes_written], offsets, sizes or None, counters or None, whole tiles) with canary checks."""
    keep = []

    def put(a, always):
        a = np.array(a, copy=True)   # exactly sized
        keep.append(a)
        return a.ctypes.data if a.size else (1 if always else None)

    src, rec = case.marshal(put)
    tb, to = frames.world_table(WORLDS)
    tb = np.frombuffer(tb, np.uint8).copy()
    a = ShimIn(src=src, rec=rec, table_bytes=tb.ctypes.data, table_off=to.ctypes.data, n_table_bytes=len(tb), n_worlds=len(WORLDS),
               scan_block=scan_block, blocks=blocks)
    raw = np.full(capacity + TAIL + 16, CANARY, np.uint8)
    at = (-raw.ctypes.data) % 16
    out = raw[at:at + capacity + TAIL]
    offs = np.full(case.n + 2, 0xC0FFEE, np.uint64)
    size = np.full(case.n + 1, 0xC0FFEE, np.uint32)
    cnt = np.full(7, 0xC0FFEE, np.uint64)
    fast = lib.wq_test_record_frames_host(ctypes.byref(a), case.n, out.ctypes.data if capacity else None, capacity, offs.ctypes.data,
                                          size.ctypes.data if with_size else None, cnt.ctypes.data if with_counters else None)
    assert offs[-1] == 0xC0FFEE and size[-1] == 0xC0FFEE and cnt[-1] == 0xC0FFEE
    written = min(capacity, int(offs[case.n]))
    assert (out[written:] == CANARY).all() and (raw[:at] == CANARY).all(), "written outside the output"
    if not with_size:
        assert (size == 0xC0FFEE).all()
    names = ("n_frames", "n_complete", "bytes_need", "bytes_written", "overflow", "error")
    return (out[:written].copy(), offs[:-1].copy(), size[:-1].copy() if with_size else None,
            dict(zip(names, (int(v) for v in cnt[:6]))) if with_counters else None, fast)


def same(got, want):
    assert np.array_equal(got[1], want[1]), "offsets"
    assert got[2] is None or np.array_equal(got[2], want[2]), "sizes"
    assert got[3] is None or got[3] == want[3], (got[3], want[3])
    assert np.array_equal(got[0], want[0]), "frames"


def test_struct_sizes(shim):
    assert shim.wq_test_recframes_sizes() == 112 | 96 << 8


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matches_definition(shim, case):
    want = case.want()
    need = want[3]["bytes_need"]
    for scan_block, blocks in ((0, 0), (1, 1), (7, 3), (64, 2)):
        same(shim_call(shim, case, need, scan_block, blocks), want)
    same(shim_call(shim, case, need + 33, 5, 0, with_size=False, with_counters=False), want)
    same(shim_call(shim, case, 0), case.want(0))
    if need > 40:
        for cap in (need - 1, need // 2, (need // 2) & ~15, 17):
            same(shim_call(shim, case, cap, 3, 2), case.want(cap))


def test_error_bits_of_the_cases():
    bit = {c.name: c.want()[3]["error"] for c in CASES}
    assert bit["bits 0 and 4"] == frames.ERROR_WORLD | frames.ERROR_HANDLE == bit["bits 0 and 4, skip empty"]
    assert bit["bit 5"] == frames.ERROR_ARENA | frames.ERROR_WORLD == bit["bit 5, no arena"]
    assert bit["bit 6"] == frames.ERROR_ROWS | frames.ERROR_WORLD and bit["bit 6, overlapping rows"] & frames.ERROR_ROWS
    assert bit["bits 1 and 2"] == frames.ERROR_PARAM | frames.ERROR_FLEX and bit["world bytes out of range"] == frames.ERROR_WORLD
    assert all(bit[k] == 0 for k in ("row lengths", "one row of 5000", "512 triples", "two 1 MiB payloads", "skip empty"))


def test_whole_tile_path(shim):
    case = next(c for c in CASES if c.name == "two 1 MiB payloads")
    got = shim_call(shim, case, case.want()[3]["bytes_need"])
    assert got[4] >= 3 * 1020
    small = next(c for c in CASES if c.name == "512 triples")
    assert shim_call(shim, small, small.want()[3]["bytes_need"])[4] == 0


def test_every_capacity_of_a_small_case(shim):
    case = small_case()
    need = case.want()[3]["bytes_need"]
    assert 300 < need < 500
    for cap in range(0, need + 2):
        same(shim_call(shim, case, cap, 2, 1), case.want(cap))


def test_empty_rows_equal_the_flat_builder(shim):
    case = next(c for c in CASES if c.name == "all rows empty")
    k = case.kw
    flat = frames.build_frames_np(WORLDS, k["sender_uuid"], k["world"], instruction=10, pos=k["pos"])
    got = shim_call(shim, case, flat[3]["bytes_need"])
    same(got, flat)


def test_too_large_through_the_sizing_call(shim):
    case = too_large_case()
    want = case.want(0)
    assert want[3]["error"] == frames.ERROR_TOO_LARGE and want[2][1] == 0 and want[2][0] > (1 << 30) - 200
    same(shim_call(shim, case, 0), want)
