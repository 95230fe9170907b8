"""The send buffers' definition (worldql_server_amd/interest.py peer_pack_np, what wq_peer_pack_device
writes) against an independent restatement: per peer, b"".join of Python bytes slices with
struct.pack("<I", ...) prefixes. Also the shared case list of tests/test_peer_pack_cpp_mirror.py and
tests/test_gpu_peer_pack.py, with a test that the list really holds the conditions it is meant to:
frame sizes around every power of two up to the 1 KiB tile and far past it, every pair of (source,
destination) residues mod 16, runs of empty and one-byte frames longer than a window of 64, a frame
of a thousand tiles, repeated messages, empty rows, the degenerate sizes, every kind of capacity cut
and hostile rows, messages and frame offsets. Every case runs with and without the length prefix."""
import functools
import itertools
import struct
from types import SimpleNamespace

import numpy as np
import pytest

from worldql_server_amd import abi, interest

TILE = 1024      # bytes of output a wave owns (csrc/pack_ops.hpp kPackTile)
CHUNK = 16       # bytes a lane stores (kPackChunk)
WINDOW = 64      # elements a tile takes through LDS at a time (kPackWindow)
RUN = 4          # consecutive tiles a block takes: all but the first find their element from the tile before (kPackRun)
SIZES = [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099, 70001]
BIG = (1 << 20) + 5


def _frames(rng, sizes):
    """(frames u8, frame_offsets u64[n + 1]) of random bytes, contiguous as wq_serialize_messages leaves them."""
    fo = np.zeros(len(sizes) + 1, np.uint64)
    np.cumsum(np.asarray(sizes, np.uint64), out=fo[1:])
    return rng.integers(0, 256, size=int(fo[-1]), dtype=np.uint8), fo


def _case(rows, frames, fo, capacity="need", offsets=None, msgs=None, hostile=False):
    """rows: a list of message-index lists. capacity: "need", "need-1", "in_prefix", "in_frame",
    "peer_boundary", "zero" (cap_of resolves it, since bytes_need depends on the prefix)."""
    if offsets is None:
        offsets = np.zeros(len(rows) + 1, np.uint32)
        np.cumsum([len(r) for r in rows], out=offsets[1:])
        msgs = np.array([m for r in rows for m in r], dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, np.uint32)
    return SimpleNamespace(offsets=offsets, msgs=np.ascontiguousarray(msgs, np.uint32), n_peers=len(offsets) - 1,
                           frames=np.ascontiguousarray(frames, np.uint8), frame_offsets=np.ascontiguousarray(fo, np.uint64),
                           capacity=capacity, hostile=hostile)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261020)
    out = {}
    # every size of the list, forwards, backwards and thinned
    fr, fo = _frames(rng, SIZES)
    n = len(SIZES)
    out["sizes"] = _case([list(range(n)), list(range(n - 1, -1, -1)), list(range(0, n, 2)), [20, 0, 20]], fr, fo)
    # small odd frames in random rows: every pair of residues mod 16
    sz = rng.integers(1, 41, size=300)
    fr2, fo2 = _frames(rng, sz)
    rows = [rng.integers(0, 300, size=int(k)).tolist() for k in rng.choice([0, 0, 1, 5, 60, 200, 333], size=37)]
    out["residues"] = _case(rows, fr2, fo2)
    # runs of empty and one-byte frames, inside one row and across a row boundary
    fr3, fo3 = _frames(rng, [0, 1, 0, 1, 200, 0, 1, 37])
    empty, one = [0, 2, 5], [1, 3, 6]
    run_e = [empty[i % 3] for i in range(75)]
    run_1 = [one[i % 3] for i in range(40)]
    out["tiny_runs"] = _case([[4] + run_e + [7] + run_1 + [4], [7] + run_e[:40], run_e[:40] + [4], [4] + run_1[:20],
                              run_1[:20] + [7], run_e + run_e + run_1 + run_1] * 6, fr3, fo3)
    # one frame of a thousand tiles between two one-byte frames
    fr4, fo4 = _frames(rng, [1, BIG, 1, 9])
    out["big_frame"] = _case([[3], [0, 1, 2], [3, 3]], fr4, fo4)
    # one message many times in one row and in many rows
    fr5, fo5 = _frames(rng, [33, 100, 7])
    out["repeats"] = _case([[1] * 50] + [[1, 0]] * 30 + [[2, 1, 1, 2]], fr5, fo5)
    # empty rows first, last and in runs
    out["empty_rows"] = _case([[], [], [], [0, 1], [], [], [2], [1, 1, 0], [], [], [], []], fr5, fo5)
    # degenerate sizes
    out["no_peers"] = _case(None, fr5, fo5, offsets=[0], msgs=[0, 1, 2, 1, 0])
    out["no_elements"] = _case([[], [], [], []], fr5, fo5)
    out["no_messages"] = _case([[0, 1], [], [5, 0, 0]], np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    out["nothing"] = _case(None, np.zeros(0, np.uint8), np.zeros(1, np.uint64), offsets=[0], msgs=[])
    # capacity cuts on one mid-sized input
    fr6, fo6 = _frames(rng, [5, 100, 0, 33, 2000, 16, 1, 700])
    rows6 = [[0, 1, 2], [4, 3], [], [5, 6, 7, 4], [1, 1], [7, 2, 0]]
    for cap in ("need", "need-1", "in_prefix", "in_frame", "peer_boundary", "zero"):
        out["cap_" + cap.replace("-", "_minus_")] = _case(rows6, fr6, fo6, capacity=cap)
    # hostile rows: descending, overlapping, past the end
    base = out["cap_need"]
    out["rows_descending"] = _case(None, fr6, fo6, offsets=base.offsets[::-1].copy(), msgs=base.msgs, hostile=True)
    out["rows_overlapping"] = _case(None, fr6, fo6, offsets=[0, 9, 4, 12, 2, 16, 16], msgs=base.msgs, hostile=True)
    out["rows_past_the_end"] = _case(None, fr6, fo6, offsets=[0, 3, 0xFFFFFFFF, 0xFFFFFFFF, 7, 40, 16], msgs=base.msgs,
                                     hostile=True)
    # junk message indices
    out["msgs_junk"] = _case([[0, 8, 1], [0xFFFFFFFF, 4], [0xFFFFFFFE, 9, 7]], fr6, fo6)
    # frame offsets that descend (message 2) and reach past the frame bytes (message 7)
    bad = fo6.copy()
    bad[3] = bad[2] - 3                  # message 2 descends; message 3 starts earlier and stays valid
    bad[8] = len(fr6) + 7
    out["frames_bad"] = _case([[0, 2, 1], [3, 7, 4], [7, 2, 2, 5]], fr6, bad)
    # the same offsets, but no element references messages 2 and 7: error bit 2 stays clear
    out["frames_bad_unreferenced"] = _case([[0, 1], [3, 4], [5, 6, 3]], fr6, bad)
    return out


def names():
    return list(cases())


def exact_names():
    return [n for n, c in cases().items() if not c.hostile]


def hostile_names():
    return [n for n, c in cases().items() if c.hostile]


@functools.lru_cache(maxsize=None)
def uncut(name, prefix):
    c = cases()[name]
    return interest.peer_pack_np(c.offsets, c.msgs, c.frames, c.frame_offsets, len_prefix=prefix)


@functools.lru_cache(maxsize=None)
def cap_of(name, prefix):
    """The capacity in bytes that the case's `capacity` word means with or without the prefix."""
    c = cases()[name]
    _, pb, eb, cnt = uncut(name, prefix)
    need, pre = cnt["bytes_need"], 4 if prefix else 0
    if c.capacity == "need":
        return need
    if c.capacity == "need-1":
        return need - 1
    if c.capacity == "zero":
        return 0
    if c.capacity == "in_prefix":        # two bytes into the record of the first 2000-byte frame
        q = list(c.msgs).index(4)
        return int(eb[q]) + 2
    if c.capacity == "in_frame":
        q = list(c.msgs).index(4)
        return int(eb[q]) + pre + 1001
    if c.capacity == "peer_boundary":
        return int(pb[3])
    raise ValueError(c.capacity)


@functools.lru_cache(maxsize=None)
def want(name, prefix):
    """(out_bytes, peer_bytes, elem_bytes, counters) of the definition at the case's capacity."""
    c = cases()[name]
    return interest.peer_pack_np(c.offsets, c.msgs, c.frames, c.frame_offsets, len_prefix=prefix,
                                 capacity=cap_of(name, prefix))


def well_formed(c, prefix, out, pb, eb, counters):
    """The clauses that hold whatever the arrays are."""
    pb, eb = [int(v) for v in pb], [int(v) for v in eb]
    assert len(pb) == c.n_peers + 1 and pb[0] == 0
    assert all(a <= b for a, b in zip(pb, pb[1:])), "PB ascends"
    assert all(a <= b for a, b in zip(eb, eb[1:])), "elem_bytes ascend"
    assert len(eb) <= len(c.msgs)
    if counters is None:
        return
    need = counters["bytes_need"]
    assert pb[-1] == need and counters["n_in"] == len(eb)
    assert counters["bytes_written"] == len(out) <= need and counters["overflow"] == int(len(out) < need)
    assert counters["n_complete"] <= counters["n_in"]
    assert all(e <= need for e in eb)
    if prefix and not counters["overflow"]:
        raw = bytes(out)
        for p in range(c.n_peers):          # prefix by prefix through the run: lands exactly on PB[p + 1]
            at = pb[p]
            while at < pb[p + 1]:
                assert at + 4 <= pb[p + 1]
                at += 4 + struct.unpack_from("<I", raw, at)[0]
            assert at == pb[p + 1]


def restated(c, prefix):
    """Independent of peer_pack_np: (the peers' runs as bytes, error bits), for offsets that ascend."""
    off = [int(v) for v in c.offsets]
    fo = [int(v) for v in c.frame_offsets]
    raw = c.frames.tobytes()
    runs, error = [], 0
    for p in range(c.n_peers):
        parts = []
        for m in (int(v) for v in c.msgs[off[p]:off[p + 1]]):
            if m >= len(fo) - 1:
                error |= abi.PACK_ERROR_MSG
                frame = b""
            elif fo[m] > fo[m + 1] or fo[m + 1] > len(raw):
                error |= abi.PACK_ERROR_FRAME
                frame = b""
            else:
                frame = raw[fo[m]:fo[m + 1]]
            parts.append((struct.pack("<I", len(frame)) if prefix else b"") + frame)
        runs.append(parts)
    return runs, error


@pytest.mark.parametrize("prefix", [False, True])
@pytest.mark.parametrize("name", exact_names())
def test_reference_matches_restatement(name, prefix):
    c = cases()[name]
    out, pb, eb, cnt = want(name, prefix)
    runs, error = restated(c, prefix)
    whole = b"".join(b"".join(parts) for parts in runs)
    cap = cap_of(name, prefix)
    assert out.tobytes() == whole[:cap]
    assert cnt["error"] == error
    assert cnt == dict(n_in=sum(len(r) for r in runs), bytes_need=len(whole), bytes_written=min(cap, len(whole)),
                       overflow=int(len(whole) > cap), error=error,
                       n_complete=sum(1 for i in range(len(eb)) if (int(eb[i + 1]) if i + 1 < len(eb) else len(whole)) <= cap))
    starts, at = [], 0
    for parts in runs:
        starts.append(at)
        at += sum(len(x) for x in parts)
    assert [int(v) for v in pb] == starts + [len(whole)]
    flat = [len(x) for parts in runs for x in parts]
    assert [int(v) for v in eb] == list(itertools.accumulate([0] + flat[:-1])) if flat else len(eb) == 0
    if not cnt["overflow"]:
        for p, parts in enumerate(runs):
            assert out[int(pb[p]):int(pb[p + 1])].tobytes() == b"".join(parts)
    well_formed(c, prefix, out, pb, eb, cnt)


@pytest.mark.parametrize("prefix", [False, True])
@pytest.mark.parametrize("name", hostile_names())
def test_reference_walks_hostile_rows_as_the_budgets_do(name, prefix):
    """Descending and overlapping offsets: error bit 0, at most n_in elements walked, and the rows are
    peer_budget_np's (a budget that keeps everything returns the walked elements)."""
    c = cases()[name]
    out, pb, eb, cnt = want(name, prefix)
    assert cnt["error"] & abi.PACK_ERROR_ROWS and cnt["n_in"] <= len(c.msgs)
    n_msgs = len(c.frame_offsets) - 1
    oo, om, bc = interest.peer_budget_np(c.offsets, c.msgs, np.zeros((n_msgs, 3)), np.zeros((c.n_peers, 3)), k=1 << 31)
    assert bc["n_in"] == cnt["n_in"]
    fo = [int(v) for v in c.frame_offsets]
    raw, pre = c.frames.tobytes(), 4 if prefix else 0
    parts = [(struct.pack("<I", fo[m + 1] - fo[m]) if prefix else b"") + raw[fo[m]:fo[m + 1]] for m in om.tolist()]
    assert out.tobytes() == b"".join(parts)
    assert [int(v) for v in pb] == [sum(len(x) for x in parts[:int(k)]) for k in oo]
    assert pre * len(parts) + sum(fo[m + 1] - fo[m] for m in om.tolist()) == cnt["bytes_need"]
    well_formed(c, prefix, out, pb, eb, cnt)


def _elements(name, prefix):
    """(source residue, destination residue, size) of every non-empty frame placed by the case."""
    c = cases()[name]
    _, _, eb, _ = uncut(name, prefix)
    fo, n_msgs, pre = c.frame_offsets, len(c.frame_offsets) - 1, 4 if prefix else 0
    walked = c.msgs[:len(eb)] if not c.hostile else []
    return [(int(fo[m]) % 16, (int(e) + pre) % 16, int(fo[m + 1]) - int(fo[m])) for m, e in zip(walked, eb)
            if m < n_msgs and fo[m] < fo[m + 1] <= len(c.frames)]


def test_case_conditions():
    cs = cases()
    size_of = lambda c, m: int(c.frame_offsets[m + 1]) - int(c.frame_offsets[m])
    # every size of the list is placed, and all 16 x 16 residue pairs occur
    placed = {s for n in exact_names() for pf in (False, True) for _, _, s in _elements(n, pf)}
    assert set(SIZES) - {0} <= placed and 0 in [size_of(cs["sizes"], m) for m in cs["sizes"].msgs]
    pairs = {(a, b) for n in exact_names() for pf in (False, True) for a, b, _ in _elements(n, pf)}
    assert len(pairs) == 256
    assert TILE == CHUNK * 64 and max(SIZES) > 64 * TILE
    # runs of >= 70 empty and 40 one-byte frames inside a row and across a row boundary
    c = cs["tiny_runs"]
    sizes = [size_of(c, m) for m in c.msgs]
    row_of = np.repeat(np.arange(c.n_peers), np.diff(c.offsets.astype(np.int64)))

    def longest(value, same_row):
        best = cur = 0
        for i, s in enumerate(sizes):
            cur = cur + 1 if s == value and (cur == 0 or not same_row or row_of[i] == row_of[i - 1]) else int(s == value)
            best = max(best, cur)
        return best
    assert longest(0, True) >= 70 and longest(1, True) >= 40
    assert longest(0, False) > longest(0, True) or longest(0, False) >= 150     # a run continues across a boundary
    off = c.offsets
    assert any(sizes[off[p] - 1] == 0 and sizes[off[p]] == 0 for p in range(1, c.n_peers) if off[p - 1] < off[p] < off[p + 1])
    assert any(sizes[off[p] - 1] == 1 and sizes[off[p]] == 1 for p in range(1, c.n_peers) if off[p - 1] < off[p] < off[p + 1])
    # more than a window of elements in one tile, without and with the prefix, and chunks of >= 3 elements
    for pf in (False, True):
        eb = [int(v) for v in uncut("tiny_runs", pf)[2]]
        per_tile = np.bincount(np.array(eb) // TILE)
        assert per_tile.max() > WINDOW
        per_chunk = np.bincount(np.array(eb) // CHUNK)
        assert per_chunk.max() >= 3
    # runs of consecutive tiles: outputs of many times RUN tiles, with tiny, mixed and huge elements
    for n in ("residues", "sizes", "big_frame"):
        assert uncut(n, False)[3]["bytes_need"] > 4 * RUN * TILE
    assert uncut("tiny_runs", False)[3]["bytes_need"] > RUN * TILE and uncut("tiny_runs", True)[3]["bytes_need"] > 4 * RUN * TILE
    # a frame of about 1,025 tiles in a row between two one-byte frames
    c = cs["big_frame"]
    row = c.msgs[c.offsets[1]:c.offsets[2]].tolist()
    assert [size_of(c, m) for m in row] == [1, BIG, 1] and BIG // TILE >= 1024
    # one message many times in one row and in many rows
    c = cs["repeats"]
    rows = [c.msgs[c.offsets[p]:c.offsets[p + 1]].tolist() for p in range(c.n_peers)]
    assert max(r.count(1) for r in rows) >= 50 and sum(1 in r for r in rows) >= 30
    # empty rows first, last and in runs
    d = np.diff(cs["empty_rows"].offsets.astype(np.int64))
    assert d[0] == 0 and d[-1] == 0 and (d[:3] == 0).all() and (d[-4:] == 0).all() and d.any()
    # degenerate sizes
    assert cs["no_peers"].n_peers == 0 and len(cs["no_peers"].msgs) > 0
    assert len(cs["no_elements"].msgs) == 0 and cs["no_elements"].n_peers > 0
    c = cs["no_messages"]
    assert len(c.frame_offsets) == 1 and len(c.msgs) > 0
    for pf in (False, True):
        assert want("no_messages", pf)[3]["error"] == abi.PACK_ERROR_MSG
        assert want("no_messages", pf)[3]["bytes_need"] == (4 * len(c.msgs) if pf else 0)
    # capacities
    for pf in (False, True):
        pre = 4 if pf else 0
        _, pb, eb, cnt = uncut("cap_need", pf)
        need = cnt["bytes_need"]
        assert cap_of("cap_need", pf) == need and not want("cap_need", pf)[3]["overflow"]
        assert cap_of("cap_need_minus_1", pf) == need - 1 and want("cap_need_minus_1", pf)[3]["overflow"]
        assert want("cap_need_minus_1", pf)[3]["n_complete"] < cnt["n_in"]
        cap = cap_of("cap_in_frame", pf)
        inside = [q for q in range(len(eb)) if int(eb[q]) + pre < cap < (int(eb[q + 1]) if q + 1 < len(eb) else need)]
        assert len(inside) == 1 and cap % CHUNK != 0
        cap = cap_of("cap_peer_boundary", pf)
        assert 0 < cap < need and cap in [int(v) for v in pb]
        assert cap_of("cap_zero", pf) == 0 and want("cap_zero", pf)[3]["overflow"] and len(want("cap_zero", pf)[0]) == 0
    cap, eb = cap_of("cap_in_prefix", True), [int(v) for v in uncut("cap_in_prefix", True)[2]]
    assert any(e < cap < e + 4 for e in eb)
    # hostile rows set bit 0; junk messages bit 1; bad frame offsets bit 2 only when referenced
    for n in hostile_names():
        assert want(n, False)[3]["error"] & abi.PACK_ERROR_ROWS
    assert np.any(np.diff(cs["rows_descending"].offsets.astype(np.int64)) < 0)
    assert want("msgs_junk", False)[3]["error"] == abi.PACK_ERROR_MSG
    assert want("frames_bad", True)[3]["error"] == abi.PACK_ERROR_FRAME
    fo = cs["frames_bad"].frame_offsets
    assert fo[2] > fo[3] and fo[8] > len(cs["frames_bad"].frames)
    assert want("frames_bad_unreferenced", True)[3]["error"] == 0
    assert cs["frames_bad_unreferenced"].frame_offsets.tobytes() == fo.tobytes()
    assert not set(cs["frames_bad_unreferenced"].msgs.tolist()) & {2, 7}
    # the largest output stays a few MiB
    assert max(uncut(n, True)[3]["bytes_need"] for n in names()) < 4 << 20


def test_every_case_differs_with_the_prefix():
    for n in names():
        a, b = uncut(n, False)[3], uncut(n, True)[3]
        assert b["bytes_need"] == a["bytes_need"] + 4 * a["n_in"] and a["n_in"] == b["n_in"]


def test_abi_constants():
    assert abi.PACK_COUNTERS_DTYPE.itemsize == 40 and abi.PACK_LEN_PREFIX == 1
    assert (abi.PACK_ERROR_ROWS, abi.PACK_ERROR_MSG, abi.PACK_ERROR_FRAME) == (1, 2, 4)
    assert abi.PACK_COUNTERS_DTYPE.names == ("n_in", "n_complete", "bytes_need", "bytes_written", "overflow", "error")
