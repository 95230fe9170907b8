"""The ingest decoder's definition (worldql_server_amd/ingest.py decode_frames_np) on the CPU: the host
decoder under the call's offset rules plus world and sender resolution, flags, flex_range and counters,
against the committed golden frames, the Python restatement oracle/fbs_oracle.py, the C sanitizer and
the frames' own field values. Also the shared case list of the decoder's CPU mirror
(tests/test_frames_decode_cpp_mirror.py) and its GPU tests (tests/test_gpu_frames_decode.py)."""
import functools
import os
import random
import struct
import sys
import uuid

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from fbs_builder import message  # noqa: E402
from fbs_cases import UUIDS_BAD, UUIDS_OK, cases as fbs_frames  # noqa: E402
from oracle import fbs_oracle  # noqa: E402

from worldql_server_amd import abi, codec, ingest  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "fbs_frames.npz")
SEEDS = (1, 2, 3)
MIB = 1 << 20
L, CHUNK, TILE = abi.INGEST_LANE_STRING, abi.INGEST_CHUNK, 4096   # lane strings, a lane's chunk, a block's step
U0 = "67e55044-10b1-426f-9247-bb680e5fe0c8"

# The world table: "world" twice (the lowest id wins), "dupe" twice, sanitized forms of the corpus' names;
# "w00" is a valid name the table does not hold.
WORLDS = ["world", "chat_fs_server_1", "a_b", "x" * 63, "world", "dupe", "dupe", "home_at_north_cl_1_bs_2", "overworld"]
# The sender table: the corpus' fixed uuids under ids that are not their index; its random uuids are unknown.
PEER_UUIDS = [uuid.UUID(U0), uuid.UUID(int=0), uuid.UUID(int=(1 << 128) - 1), uuid.UUID(int=0x1234), uuid.UUID(int=1 << 127)]
PEER_IDS = [7, 0, 3, 4000000000, 12]


def golden():
    g = np.load(GOLDEN)
    return g["data"].astype(np.uint8), g["offsets"].astype(np.uint64)


@functools.lru_cache(maxsize=None)
def corpus(seed):
    return codec.pack_frames(fbs_frames(seed, 400, 600))


@functools.lru_cache(maxsize=None)
def definition(name):
    """decode_frames_np of a named case over the shared tables, computed once."""
    data, offsets, nb = batches()[name]
    return ingest.decode_frames_np(data, offsets, WORLDS, PEER_UUIDS, PEER_IDS, n_frame_bytes=nb)


def flat(parameter=None, world_name="world", sender_uuid=U0, **kw):
    kw.setdefault("instruction", 7)
    kw.setdefault("position", (1.0, -2.5, 3.0))
    return message(parameter=parameter, sender_uuid=sender_uuid, world_name=world_name, **kw)


@functools.lru_cache(maxsize=None)
def frame_136():
    """A valid flat frame of exactly 136 bytes (C5's size)."""
    f = flat(world_name="overworld")
    assert len(f) == 136
    return f


def with_byte(n, at, value=0xFF, fill=b"a"):
    b = bytearray(fill * n)
    b[at] = value
    return bytes(b)


def long_string_pairs():
    """(frame, status) for parameters of L - 1, L, L + 1, 4095 .. 4097 and 1 MiB bytes: valid, and with a
    bad byte first, last and on each side of a chunk and of a tile boundary."""
    out = []
    for n in (L - 1, L, L + 1, TILE - 1, TILE, TILE + 1, MIB):
        out.append((flat(parameter=b"a" * n), 0))
        for at in sorted({0, n - 1, CHUNK - 1, CHUNK, L - 1, L, TILE - 1, TILE, n - CHUNK - 1, n - CHUNK} & set(range(n))):
            out.append((flat(parameter=with_byte(n, at)), 1))
    return out


SEQS = ("é".encode(), "€".encode(), "😀".encode())


def straddle_pairs():
    """(frame, status): 2-, 3- and 4-byte sequences across a chunk boundary (inside a 300-byte parameter,
    so the chunked pass sees them) and across a tile boundary at every split, whole, with the last byte
    broken and with the lead replaced by a continuation byte; the same inside a short parameter, which
    the walking lane checks; a sequence cut by the string's end; a continuation byte too many."""
    out = []
    for n, edge in ((300, 272), (5000, TILE), (40, 16)):
        for s in SEQS:
            for split in range(0, len(s) + 1):
                b = bytearray(b"a" * n)
                b[edge - split:edge - split + len(s)] = s
                out.append((flat(parameter=bytes(b)), 0))
                b[edge - split + len(s) - 1] = ord("a")
                out.append((flat(parameter=bytes(b)), 1))
                b[edge - split] = 0x80
                out.append((flat(parameter=bytes(b)), 1))
    for n in (20, 300):
        for s in SEQS:
            out.append((flat(parameter=b"a" * (n - len(s) + 1) + s[:-1]), 1))
            out.append((flat(parameter=b"a" * (n - len(s)) + s), 0))
        out.append((flat(parameter=b"a" * (n - 5) + b"\xf0\x9f\x98\x80\x80"), 1))
        out.append((flat(parameter=b"\x80" + b"a" * n), 1))
    return out


def nul_frames():
    """A missing NUL, and a string that ends on the frame's last byte, short and long."""
    out = []
    for n in (5, 300):
        world = b"w" * n
        f = bytearray(flat(world_name=world))
        at = bytes(f).rindex(world) + n
        assert f[at] == 0
        g = bytearray(f)
        g[at] = 1
        out += [bytes(f), bytes(g), bytes(f[:at]), bytes(f[:at + 1])]
    return out


def rec(i=0, entity=False, **over):
    d = dict(uuid=str(uuid.UUID(int=i + 1)), world_name="world", data="d%d" % i, flex=b"\x01\x02",
             position=(float(i), 0.5, -2.0) if entity or i % 2 else None)
    d.update(over)
    return d


def record_frames():
    out = [flat(records=[rec(i) for i in range(k)], entities=[rec(i, True) for i in range(k % 4)]) for k in (0, 1, 3, 300)]
    # a bad record uuid together with an entity missing its position: records rank first
    out.append(flat(records=[rec(0), rec(1, uuid="nope")], entities=[rec(0, True, position=None)]))
    out.append(flat(records=[rec(0)], entities=[rec(0, True, position=None), rec(1, True, uuid="nope")]))
    out.append(flat(records=[rec(0, world_name=None)], entities=[rec(1, True, uuid="nope")]))
    out.append(flat(records=[rec(0, data="x" * 300), rec(1, data=with_byte(300, 299))]))   # long strings in records
    return out


def shared_data_frame(n_records, data_len):
    """One Message whose n_records records all point their `data` (and uuid, world) at the same strings:
    the verifier counts the string once per reference (its apparent size), the frame holds it once."""
    b = bytearray(4)
    vt_m = len(b)                                   # Message vtable: sender, world, records
    b += struct.pack("<HH", 4 + 2 * 9, 16) + struct.pack("<9H", 0, 0, 4, 8, 0, 12, 0, 0, 0)
    while len(b) % 4:
        b += b"\0"
    t_m = len(b)
    b += struct.pack("<i", t_m - vt_m) + bytes(12)
    struct.pack_into("<I", b, 0, t_m)
    vt_r = len(b)                                   # Record vtable, shared: uuid, world, data
    b += struct.pack("<HH", 4 + 2 * 5, 16) + struct.pack("<5H", 4, 0, 8, 12, 0)
    while len(b) % 4:
        b += b"\0"
    vec = len(b)
    struct.pack_into("<I", b, t_m + 12, vec - (t_m + 12))
    b += struct.pack("<I", n_records) + bytes(4 * n_records)
    tabs = []
    for i in range(n_records):
        tabs.append(len(b))
        struct.pack_into("<I", b, vec + 4 + 4 * i, len(b) - (vec + 4 + 4 * i))
        b += struct.pack("<i", len(b) - vt_r) + bytes(12)
    strings = {}
    for key, raw in (("uuid", U0.encode()), ("world", b"world"), ("data", b"z" * data_len)):
        while len(b) % 4:
            b += b"\0"
        strings[key] = len(b)
        b += struct.pack("<I", len(raw)) + raw + b"\0"
    for slot, key in ((4, "uuid"), (8, "world")):
        struct.pack_into("<I", b, t_m + slot, strings[key] - (t_m + slot))
    for t in tabs:
        for slot, key in ((4, "uuid"), (8, "world"), (12, "data")):
            struct.pack_into("<I", b, t + slot, strings[key] - (t + slot))
    while len(b) % 4:
        b += b"\0"
    return bytes(b)


def truncations(frame):
    return [frame[:k] for k in range(len(frame))] + [frame]


def corruptions(frame, values=(0x00, 0xFF)):
    out = []
    for k in range(len(frame)):
        for v in values:
            b = bytearray(frame)
            b[k] = v
            out.append(bytes(b))
    return out


def hand_frames():
    """@global, every sanitize error, an absent world, duplicate table names, unknown senders, the three
    uuid text forms (and the refused ones), every field present or absent."""
    worlds = ["@global", "@Global", "", "0bad", "_bad", "été", "bad-char", "badé", "x" * 63, "x" * 64, "x" * 70,
              "a/" * 16, "w00", "world", "dupe", "chat/server_1", "a b", "home@north:1\\2", "World", "world ", "x" * 300]
    out = [flat(world_name=w) for w in worlds]
    out += [flat(sender_uuid=u) for u in UUIDS_OK + UUIDS_BAD]
    out += [flat(sender_uuid=str(u)) for u in PEER_UUIDS] + [flat(sender_uuid=str(uuid.UUID(int=77)))]
    out += [flat(sender_uuid=PEER_UUIDS[3].hex), flat(sender_uuid="urn:uuid:" + str(PEER_UUIDS[4])),
            flat(sender_uuid=str(PEER_UUIDS[4]).upper())]
    for flex in (None, b"", b"\x00", b"\xff" * 5, bytes(range(256)) * 9):
        for param in (None, "", "p"):
            out.append(flat(parameter=param, flex=flex, position=None if param == "" else (0.0, 1.0, 2.0),
                            instruction=13 if flex else 7, replication=3 if param else 2))
    out += [flat(sender_uuid=None), flat(world_name=None), b"", b"\x04\0\0\0"]
    return out


@functools.lru_cache(maxsize=None)
def batches():
    """name -> (data, offsets, n_frame_bytes or None)."""
    pk = lambda frames: codec.pack_frames(frames) + (None,)
    out = {"golden": golden() + (None,)}
    for s in SEEDS:
        out["corpus_%d" % s] = corpus(s) + (None,)
    out["hand"] = pk(hand_frames())
    out["long_strings"] = pk([f for f, _ in long_string_pairs()])
    out["straddle"] = pk([f for f, _ in straddle_pairs()])
    out["nul"] = pk(nul_frames())
    out["records"] = pk(record_frames())
    out["records_among_flat"] = pk([frame_136()] * 500 + [flat(records=[rec(i) for i in range(300)])] + [frame_136()] * 500)
    out["truncations_136"] = pk(truncations(frame_136()))
    out["truncations_nested"] = pk(truncations(flat(records=[rec(0), rec(1)], entities=[rec(0, True), rec(1, True)])))
    out["corruptions_136"] = pk(corruptions(frame_136()))
    out["empty"] = (np.zeros(0, np.uint8), np.zeros(1, np.uint64), None)
    # both offset errors: descending, past the end, the frames those make ambiguous, and 2^32
    d, o, _ = out["hand"]
    bad = o[:12].copy()
    bad[3], bad[4] = o[4], o[3]           # frames 2 .. 4 see a descent
    bad[8] = len(d) + 5                   # frames 7 and 8 reach past the end
    out["offsets_descend_past"] = (d, bad, None)
    out["offsets_cut_buffer"] = (d, o[:12].copy(), int(o[10]) + 3)      # n_frame_bytes inside frame 10
    huge = np.array([0, 136, 136 + (1 << 32)], np.uint64)
    out["offsets_huge"] = (np.frombuffer(frame_136(), np.uint8), huge, 136 + (1 << 32))   # claimed, never read
    return out


def small_names():
    return [k for k in batches() if k != "offsets_huge"]


def same(got, want, what=""):
    """Every output and the counters byte for byte."""
    for k in ingest.OUT_FIELDS:
        if got.get(k) is None:
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.tobytes() != b.tobytes():
            i = int(np.flatnonzero(a.reshape(len(b), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8))[0]) \
                // max(a.reshape(len(b), -1).view(np.uint8).shape[1], 1)
            raise AssertionError(f"{what}: {k} differs first at frame {i}: {a[i]} != {b[i]}")
    if got.get("counters") is not None:
        assert got["counters"] == want["counters"], what


# ---- the definition against independent restatements ------------------------------------------------

def expected_world(name: bytes):
    """World id by the C sanitizer (not world_names.py) and a plain list search."""
    text = name.decode("utf-8")
    if text == "@global":
        return abi.WORLD_GLOBAL
    try:
        return WORLDS.index(codec.sanitize_world_name(text))
    except (codec.SanitizeCError, ValueError):
        return abi.WORLD_INVALID


def check_against_oracle(data, offsets, d):
    peers = {u.bytes: i for u, i in zip(PEER_UUIDS, PEER_IDS)}
    n = len(offsets) - 1
    counts = dict(n_frames=n, n_ok=0, n_invalid=0, n_missing=0, n_bad_uuid=0, n_world_unresolved=0, n_sender_unknown=0, error=0)
    for i in range(n):
        f = data[int(offsets[i]):int(offsets[i + 1])].tobytes()
        o = fbs_oracle.decode(f)
        assert d["msg"]["status"][i] == o["status"], i
        counts[("n_ok", "n_invalid", "n_missing", "n_bad_uuid")[o["status"]]] += 1
        if o["status"] != 0:
            assert d["flags"][i] == 0 and d["world"][i] == abi.WORLD_INVALID and d["sender"][i] == abi.INGEST_NO_PEER
            assert not d["pos"][i].view(np.uint64).any() and not d["sender_uuid"][i].any() and not d["flex_range"][i].any()
            assert d["repl"][i] == 0 and d["instruction"][i] == 0
            assert d["msg"][i].tobytes() == struct.pack("<i", o["status"]) + bytes(68)
            continue
        w = expected_world(o["world"])
        s = peers.get(o["sender_uuid"], abi.INGEST_NO_PEER)
        assert (d["world"][i], d["sender"][i]) == (w, s), i
        assert d["instruction"][i] == o["instruction"] and d["repl"][i] == o["replication"]
        assert d["sender_uuid"][i].tobytes() == o["sender_uuid"]
        want_pos = struct.pack("<3d", *o["position"]) if o["position"] is not None else bytes(24)
        assert d["pos"][i].tobytes() == want_pos or (o["position"] is not None and any(x != x for x in o["position"]))
        flags = d["flags"][i]
        assert flags & 1 and bool(flags & 2) == (o["position"] is not None) and bool(flags & 4) == (o["parameter"] is not None)
        assert bool(flags & 16) == (w == abi.WORLD_GLOBAL) and bool(flags & 32) == (w < abi.WORLD_GLOBAL)
        assert bool(flags & 64) == (s != abi.INGEST_NO_PEER)
        counts["n_world_unresolved"] += w == abi.WORLD_INVALID
        counts["n_sender_unknown"] += s == abi.INGEST_NO_PEER
        off, ln = map(int, d["flex_range"][i])
        assert bool(flags & 8) or (off, ln) == (0, 0)
    assert d["counters"] == counts


def test_golden_frames():
    data, offsets = golden()
    d = definition("golden")
    g = np.load(GOLDEN)
    assert len(d["msg"]) == 624 and set(g["status"].tolist()) == {0, 1, 2, 3}
    np.testing.assert_array_equal(d["msg"]["status"], g["status"])
    ok = g["status"] == 0
    np.testing.assert_array_equal(d["instruction"][ok], g["instruction"][ok])
    np.testing.assert_array_equal(d["repl"][ok], g["replication"][ok])
    np.testing.assert_array_equal(d["sender_uuid"][ok], g["sender_uuid"][ok])
    np.testing.assert_array_equal(d["flags"][ok] & 2, 2 * g["has_position"][ok])
    check_against_oracle(data, offsets, d)


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_corpus_against_the_oracle(seed):
    data, offsets = corpus(seed)
    # the corpus still exercises every status, by the host decoder alone
    by_status = np.bincount(codec.decode_packed(data, offsets)["status"], minlength=4)
    assert by_status[0] >= 300 and (by_status[1:] >= 20).all(), by_status
    d = definition("corpus_%d" % seed)
    check_against_oracle(data, offsets, d)
    c = d["counters"]
    assert c["n_world_unresolved"] >= 20 and c["n_sender_unknown"] >= 20
    assert c["n_ok"] - c["n_world_unresolved"] >= 20 and c["n_ok"] - c["n_sender_unknown"] >= 20


def test_hand_made_worlds_and_senders():
    data, offsets, _ = batches()["hand"]
    d = definition("hand")
    check_against_oracle(data, offsets, d)
    world = lambda name: int(ingest.decode_frames_np(*codec.pack_frames([flat(world_name=name)]), WORLDS, [])["world"][0])
    G, X = abi.WORLD_GLOBAL, abi.WORLD_INVALID
    assert [world(w) for w in ("@global", "@Global", "", "0bad", "été", "bad-char", "x" * 64, "a/" * 16)] == [G] + [X] * 7
    assert [world(w) for w in ("world", "dupe", "chat/server_1", "a b", "x" * 63, "home@north:1\\2", "w00")] == \
        [0, 5, 1, 2, 3, 7, X]
    for form in (str(PEER_UUIDS[3]), PEER_UUIDS[3].hex, "urn:uuid:" + str(PEER_UUIDS[3]), str(PEER_UUIDS[3]).upper()):
        r = ingest.decode_frames_np(*codec.pack_frames([flat(sender_uuid=form)]), WORLDS, PEER_UUIDS, PEER_IDS)
        assert r["sender"][0] == 4000000000 and r["flags"][0] & 64
    r = ingest.decode_frames_np(*codec.pack_frames([flat()]), [], PEER_UUIDS)             # ids default to the index
    assert (r["sender"][0], r["world"][0], r["flags"][0] & 0x70) == (0, X, 64)
    r = ingest.decode_frames_np(*codec.pack_frames([flat()]), None, None)                # no tables at all
    assert (r["sender"][0], r["world"][0], r["counters"]["n_world_unresolved"], r["counters"]["n_sender_unknown"]) == \
        (abi.INGEST_NO_PEER, X, 1, 1)
    with pytest.raises(ValueError):
        ingest.decode_frames_np(*codec.pack_frames([flat()]), WORLDS, [PEER_UUIDS[0], PEER_UUIDS[0]])


def test_offset_errors():
    d = definition("offsets_descend_past")
    ref = definition("hand")
    st = d["msg"]["status"]
    assert d["counters"]["error"] == abi.INGEST_ERROR_OFFSETS
    # 2 and 4 share an offset with the descending pair of 3; 9 shares one with 8, whose pair descends too
    assert st[[2, 3, 4, 7, 8, 9]].tolist() == [1] * 6
    for i in (0, 1, 5, 6, 10):          # no suspect offset: as in the clean batch
        assert d["msg"][i].tobytes() == ref["msg"][i].tobytes() and d["world"][i] == ref["world"][i]
    d = definition("offsets_cut_buffer")
    assert d["msg"]["status"][10] == 1 and d["counters"]["error"] == abi.INGEST_ERROR_OFFSETS
    assert d["msg"][:10].tobytes() == ref["msg"][:10].tobytes()
    d = definition("offsets_huge")
    assert d["msg"]["status"].tolist() == [0, 1] and d["counters"]["error"] == abi.INGEST_ERROR_HUGE
    # the host form refuses descending offsets for the whole call: the one documented difference
    data, bad, _ = batches()["offsets_descend_past"]
    with pytest.raises(ValueError):
        codec.decode_packed(data, bad)


def test_flex_range_is_where_the_builder_put_it():
    r = random.Random(5)
    frames, flexes = [], []
    for k in range(200):
        flex = r.choice([None, b"", bytes(r.randrange(256) for _ in range(r.randrange(1, 40)))])
        frames.append(flat(parameter=r.choice([None, "", "pq" * r.randrange(9)]), flex=flex,
                           records=[rec(0, flex=b"\x09" * 7)] if k % 5 == 0 else None))
        flexes.append(flex)
    data, offsets = codec.pack_frames(frames)
    d = ingest.decode_frames_np(data, offsets, WORLDS, PEER_UUIDS, PEER_IDS)
    for f, flex, (off, ln), flags in zip(frames, flexes, d["flex_range"], d["flags"]):
        assert bool(flags & abi.INGEST_HAS_FLEX) == (flex is not None)
        if flex is None:
            assert (off, ln) == (0, 0)
        else:
            assert ln == len(flex) and off > 0 and f[off:off + ln] == flex
            assert struct.unpack_from("<I", f, off - 4)[0] == ln


def test_long_string_and_record_cases_have_the_statuses_they_were_built_for():
    for name, pairs in (("long_strings", long_string_pairs()), ("straddle", straddle_pairs())):
        assert definition(name)["msg"]["status"].tolist() == [st for _, st in pairs], name
    assert definition("nul")["msg"]["status"].tolist() == [0, 1, 1, 0] * 2   # whole, NUL overwritten, cut before the NUL, cut behind it
    d = definition("records")
    assert d["msg"]["status"].tolist() == [0, 0, 0, 0, 3, 2, 2, 1]
    assert d["msg"]["n_records"][:4].tolist() == [0, 1, 3, 300] and d["msg"]["n_entities"][:4].tolist() == [0, 1, 3, 0]
    d = definition("records_among_flat")
    assert (d["msg"]["status"] == 0).all() and d["msg"]["n_records"][500] == 300
    for name in ("truncations_136", "truncations_nested"):   # only the final padding may go
        st = definition(name)["msg"]["status"]
        assert (st[:-4] == 1).all() and st[-1] == 0 and len(st) > 130
    c = definition("corruptions_136")["counters"]
    assert c["n_frames"] == 272 and min(c["n_ok"], c["n_invalid"], c["n_bad_uuid"]) > 0


def test_shared_string_passes_the_apparent_size_limit():
    assert codec.decode_batch([shared_data_frame(3, 300)])["status"][0] == 0
    f = shared_data_frame(2049, MIB)
    assert 1.0 * MIB < len(f) < 1.2 * MIB
    assert codec.decode_batch([f])["status"][0] == 1        # 2,049 x 1 MiB > 2^31 apparent bytes
