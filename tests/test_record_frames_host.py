"""frames.build_record_frames_np and record_frame_size_np: the definition of RecordReply frames read from the
payload slab. The closed-form size against the host serializer on every ordered triple, pair and single of the 8
record shapes, names of 0..4 bytes and payloads of 0..5 bytes; every field back out of the frames; each error bit
on a hand-made case. No GPU needed."""
import itertools
import uuid

import numpy as np
import pytest

from worldql_server_amd import abi, codec, frames, ingest, records

E = abi.SLAB_ENTRY_DTYPE
WORLDS = ["", "w", "ab", "abc", "four", "a_longer_world_name"]


class Slab:
    """Entries and an arena built record by record on the host."""

    def __init__(self):
        self.entries, self.arena = [], bytearray()

    def add(self, shape, world=1, data=b"", flex=b"", live=True, seed=None):
        k = len(self.entries) if seed is None else seed
        e = np.zeros(1, E)[0]
        e["uuid"] = np.frombuffer(uuid.UUID(int=(k * 0x9E3779B97F4A7C15F39CC0605CEDC835) % (1 << 128)).bytes, np.uint8)
        e["pos"] = (k + 0.5, -2.0 * k, 1e-3 * k)
        e["world"], e["off"] = world, len(self.arena)
        e["bits"] = (shape & 7) | (abi.SLAB_LIVE if live else 0)
        if shape & 1:
            e["data_len"] = len(data)
            self.arena += data
        if shape & 2:
            e["flex_len"] = len(flex)
            self.arena += flex
        self.entries.append(e)
        return len(self.entries) - 1

    def arrays(self):
        return np.array(self.entries, dtype=E).reshape(-1), np.frombuffer(bytes(self.arena), np.uint8)


def build(slab, rows, n=None, **kw):
    """Rows of handles -> build_record_frames_np's result."""
    ent, arena = slab.arrays()
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    hd = np.array([h for r in rows for h in r], np.uint32)
    n = len(rows)
    kw.setdefault("world", np.arange(n, dtype=np.uint32) % len(WORLDS))
    kw.setdefault("instruction", 10)
    return frames.build_record_frames_np(WORLDS, kw.pop("sender_uuid", None), kw.pop("world"), kw.pop("row_offsets", off),
                                         kw.pop("handles", hd), ent, arena, **kw)


def records_of(data, offsets, i):
    """Frame i's records as dicts, read back with the ingest reader."""
    fr = data[int(offsets[i]):int(offsets[i + 1])].tobytes()
    m = codec.decode_packed(np.frombuffer(fr, np.uint8), np.array([0, len(fr)], np.uint64))[0]
    assert m["status"] == 0
    out = []
    for r in range(int(m["n_records"])):
        mm = {k: m[k] for k in m.dtype.names}
        mm["instruction"] = 8   # deferred_event names the event by a record instruction; the records are read alike
        out.append(ingest.deferred_event(fr, mm, r)["records"][0])
    return m, fr, out


def test_sizes_on_every_ordered_triple_of_shapes():
    """512 rows of 3 records: every first-occurrence order and every 10 / 14-byte residue hand-over. The definition
    asserts record_frame_size_np against the serializer's sizes itself; the sizes are compared here once more."""
    slab = Slab()
    one = [slab.add(s, world=1 + s % 4, data=b"d" * (s % 3), flex=b"f" * (s % 5)) for s in range(8)]
    rows = [[one[a], one[b], one[c]] for a, b, c in itertools.product(range(8), repeat=3)]
    rows += [[one[a]] for a in range(8)] + [[one[a], one[b]] for a, b in itertools.product(range(8), repeat=2)] + [[]]
    data, offsets, sizes, cnt = build(slab, rows)
    assert cnt["error"] == 0 and cnt["n_frames"] == len(rows) == 512 + 8 + 64 + 1
    ent, _ = slab.arrays()
    for i, row in enumerate(rows):
        shapes = [(int(ent[h]["bits"]) & 7, len(WORLDS[int(ent[h]["world"])]), int(ent[h]["data_len"]), int(ent[h]["flex_len"])) for h in row]
        assert sizes[i] == frames.record_frame_size_np(False, 10, 0, len(WORLDS[i % len(WORLDS)]), None, None, shapes)
    assert int(offsets[-1]) == len(data) == int(sizes.sum())
    m, _, recs = records_of(data, offsets, 77)
    assert m["n_records"] == 3 and [r["uuid"] for r in recs] == [
        (int.from_bytes(bytes(ent[h]["uuid"][:8]), "big"), int.from_bytes(bytes(ent[h]["uuid"][8:]), "big")) for h in rows[77]]


@pytest.mark.parametrize("wl", range(5))
@pytest.mark.parametrize("dl", range(6))
def test_sizes_on_short_names_and_payloads(wl, dl):
    slab = Slab()
    hs = [slab.add(s, world=wl, data=b"x" * dl, flex=bytes(range(fl))) for s in range(8) for fl in range(6)]
    data, offsets, sizes, cnt = build(slab, [hs, hs[::-1], hs[::7]], world=np.array([wl, 0, 4], np.uint32))
    assert cnt["error"] == 0 and len(data) == int(sizes.sum())


def test_every_field_comes_back():
    slab = Slab()
    a = slab.add(7, world=4, data="dätä".encode(), flex=b"\x00\xff\x10")
    b = slab.add(4, world=2)
    c = slab.add(1, world=0, data=b"")
    d = slab.add(2, world=5, flex=b"")
    su = np.frombuffer(uuid.UUID(int=0x1234).bytes + bytes(16), np.uint8).reshape(2, 16)
    pos = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    data, offsets, sizes, cnt = build(slab, [[a, b, c, d, a], []], sender_uuid=su, pos=pos, replication=2,
                                      param=np.frombuffer(b"42", np.uint8), param_offsets=np.array([0, 2, 2], np.uint64))
    assert cnt["error"] == 0
    m, fr, recs = records_of(data, offsets, 0)
    w0 = int(m["world_off"])
    assert bytes(m["sender_uuid"]) == uuid.UUID(int=0x1234).bytes and fr[w0:w0 + int(m["world_len"])] == b""
    assert m["instruction"] == 10 and m["replication"] == 2 and tuple(m["position"]) == (1.0, 2.0, 3.0) and m["n_entities"] == 0
    assert fr[int(m["param_off"]):int(m["param_off"]) + int(m["param_len"])] == b"42"
    ent, _ = slab.arrays()
    want = [("four", "dätä", b"\x00\xff\x10", True), ("ab", None, None, True), ("", "", None, False), ("a_longer_world_name", None, b"", False)]
    want.append(want[0])   # the same handle twice gives the record twice
    assert len(recs) == 5
    for r, h, (wn, dt, fx, has_pos) in zip(recs, [a, b, c, d, a], want):
        assert (r["world_name"], r["data"], r["flex"]) == (wn, dt, fx)
        assert r["position"] == (tuple(ent[h]["pos"]) if has_pos else None)
    m2, _, recs2 = records_of(data, offsets, 1)
    assert m2["n_records"] == 0 and recs2 == [] and bytes(m2["sender_uuid"]) == bytes(16)
    # without a sender the nil uuid
    data3, offsets3, _, _ = build(slab, [[b]])
    assert bytes(records_of(data3, offsets3, 0)[0]["sender_uuid"]) == bytes(16)


def test_empty_rows_equal_the_flat_builder():
    slab = Slab()
    su = np.arange(48, dtype=np.uint8).reshape(3, 16)
    kw = dict(world=np.array([1, 2, 9], np.uint32), instruction=np.array([0, 3, 10], np.uint8), replication=1,
              pos=np.arange(9.0).reshape(3, 3), msg_flags=np.array([1, 0, 1], np.uint8))
    got = build(slab, [[], [], []], sender_uuid=su, **kw)
    flat = frames.build_frames_np(WORLDS, su, **kw)
    assert np.array_equal(got[0], flat[0]) and np.array_equal(got[1], flat[1]) and got[3] == flat[3]
    assert got[3]["error"] == frames.ERROR_WORLD
    skipped = build(slab, [[], [], []], sender_uuid=su, flags=frames.SKIP_EMPTY, **kw)
    assert skipped[3]["bytes_need"] == 0 and not skipped[2].any() and skipped[3]["n_complete"] == 3


def test_error_bits():
    slab = Slab()
    ok = slab.add(3, data=b"abc", flex=b"defg")
    dead = slab.add(3, data=b"abc", flex=b"defg", live=False)
    far = slab.add(1, world=77, data=b"zz")
    ent, arena = slab.arrays()
    # bit 4: a handle past the entries, an entry that is not live: left out, frame i stays query i's
    d, o, s, c = build(slab, [[ok, 99, dead], [dead], [ok]])
    assert c["error"] == frames.ERROR_HANDLE and [records_of(d, o, i)[0]["n_records"] for i in range(3)] == [1, 0, 1]
    d, o, s, c = build(slab, [[ok, 99, dead], [dead], [ok]], flags=frames.SKIP_EMPTY)
    assert c["error"] == frames.ERROR_HANDLE and s[1] == 0 and s[0] > 0 and s[2] > 0 and o[1] == o[2]
    # bit 0: the entry's world outside the table
    d, o, s, c = build(slab, [[far]])
    assert c["error"] == frames.ERROR_WORLD and records_of(d, o, 0)[2][0]["world_name"] == ""
    # bit 5: the payload leaves the arena: present and empty
    short = frames.build_record_frames_np(WORLDS, None, np.zeros(1, np.uint32), np.array([0, 1], np.uint32), np.array([ok], np.uint32),
                                          ent, arena[:5], instruction=10)
    assert short[3]["error"] == frames.ERROR_ARENA
    r = records_of(short[0], short[1], 0)[2][0]
    assert r["data"] == "abc" and r["flex"] == b""
    # bit 6: rows that descend or pass n_handles are clamped
    d, o, s, c = build(slab, [[ok], [ok]], row_offsets=np.array([0, 5, 1], np.uint32))
    assert c["error"] == frames.ERROR_ROWS and [records_of(d, o, i)[0]["n_records"] for i in range(2)] == [2, 0]
    # bit 3: the 2^30 rule through a sizing call with claimed lengths and no arena
    big = np.zeros(2, E)
    big["bits"], big["flex_len"] = abi.SLAB_LIVE | abi.SLAB_FLEX, (1 << 30) - 200
    big["off"] = [0, 1 << 30]
    out = frames.build_record_frames_np(WORLDS, None, np.zeros(2, np.uint32), np.array([0, 1, 3], np.uint32), np.array([0, 0, 1], np.uint32),
                                        big, None, instruction=10, capacity=0, n_payload_bytes=1 << 31)
    assert out[3]["error"] == frames.ERROR_TOO_LARGE and out[2][1] == 0 and (1 << 30) - 200 < out[2][0] <= 1 << 30
    # per-message world names as bytes replace the ids; a range outside them is an empty name
    wb = np.frombuffer(b"alphaomega", np.uint8)
    d, o, s, c = build(slab, [[ok], [ok]], world_bytes=wb, world_off=np.array([0, 5], np.uint64), world_len=np.array([5, 6], np.uint32))
    m, fr, _ = records_of(d, o, 0)
    assert fr[int(m["world_off"]):int(m["world_off"]) + 5] == b"alpha" and c["error"] == frames.ERROR_WORLD
    assert records_of(d, o, 1)[0]["world_len"] == 0
