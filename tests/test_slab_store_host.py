"""records.slab_store_np, the definition of wq_slab_store_device: placement, the entries' fields, all-or-nothing
on both overflows, hostile references and skipped deletes. No GPU needed. The case list is shared with
tests/test_slab_store_cpp_mirror.py (the ops header on the CPU) and tests/test_gpu_slab_store.py."""
import uuid

import numpy as np
import pytest

from worldql_server_amd import abi, records

E, C = abi.SLAB_ENTRY_DTYPE, records.CREATE


class Case:
    """Frames of random bytes and ops / references into them."""

    def __init__(self, name, frame_sizes, seed=1):
        self.name, self.rng = name, np.random.default_rng(seed)
        self.frames = self.rng.integers(0, 256, int(sum(frame_sizes)), dtype=np.uint8)
        self.offsets = np.concatenate([[0], np.cumsum(frame_sizes)]).astype(np.uint64)
        self.ops, self.refs = [], []

    def add(self, frame, data=None, flex=None, kind=C, handle=None, bits=None):
        """data / flex: (off, len) inside the frame, or None when absent."""
        h = len(self.ops) if handle is None else handle
        u = uuid.UUID(int=int.from_bytes(self.rng.bytes(16), "big")).int
        pos = tuple(float(v) for v in self.rng.integers(-500, 500, 3))
        self.ops.append((kind, int(self.rng.integers(0, 5)), pos, u >> 64, u & (2**64 - 1), 1234, h, 0))
        b = ((data is not None) | 2 * (flex is not None)) if bits is None else bits
        d, f = data or (0, 0), flex or (0, 0)
        self.refs.append((frame, len(self.refs), d[0], d[1], f[0], f[1], b, 0))
        return self

    def arrays(self):
        return (np.array(self.ops, dtype=records.REC_OP_DTYPE).reshape(-1), np.array(self.refs, dtype=abi.REC_OP_REF_DTYPE).reshape(-1),
                self.frames, self.offsets)

    def need(self):
        """(entries, payload bytes) the case needs from cursor 0."""
        _, _, _, c = records.slab_store_np(*self.arrays(), np.zeros(0, E), np.zeros(0, np.uint8), 0)
        return c["entries_need"], c["bytes_stored"]


def back_to_back(name, lens, seed):
    """One frame; payloads of the given lengths back to back in it, alternating data and flex."""
    c = Case(name, [int(sum(lens)) + 7], seed)
    at = 3
    for i, n in enumerate(lens):
        c.add(0, data=(at, n)) if i % 2 else c.add(0, flex=(at, n))
        at += n
    return c


def cases():
    out = [Case("no ops", [40]), Case("no frames", [])]
    out.append(Case("one of each", [100, 50], 2).add(0, (4, 10), (20, 30)).add(1, (0, 50)).add(1, None, (49, 1)).add(0))
    out.append(Case("deletes skipped", [64], 3).add(0, (0, 8), kind=records.DELETE, handle=0).add(0, (8, 8), (16, 8), handle=5)
               .add(0, (1, 60), kind=records.DELETE, handle=5).add(0, (30, 3), handle=2))
    out.append(Case("empty payloads", [16], 4).add(0, (3, 0), (5, 0)).add(0, (16, 0)).add(0).add(0, None, (0, 16)))
    out.append(back_to_back("0..40", list(range(41)), 5))
    out.append(back_to_back("around a tile", [1022, 1023, 1024, 1025, 1026], 6))
    out.append(back_to_back("around four tiles", [4095, 4096, 4097], 7))
    many = Case("a thousand empty then one", [300], 8)
    for i in range(1000):
        many.add(0, (i % 300, 0), (0, 0))
    out.append(many.add(0, (0, 300), (10, 200)))
    big = Case("1 MiB flex", [(1 << 20) + 100, 80], 9)
    out.append(big.add(1, (0, 80)).add(0, (3, 17), (37, 1 << 20)).add(1, (5, 5)))
    two = Case("two 1 MiB payloads", [(1 << 20) + 5, (1 << 20) + 9], 10)
    out.append(two.add(0, None, (5, 1 << 20)).add(1, (9, 1 << 20)))
    h = Case("hostile references", [100, 60], 11)
    h.add(2, (0, 4), (4, 4)).add(0xFFFFFFFF, (0, 1)).add(0, (90, 11), (0, 10)).add(1, (0, 60), (60, 1))
    h.add(0, (0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 2)).add(1, (1, 2), (3, 4)).add(0, (100, 0), (101, 0))
    h.add(1, (0, 61), bits=0).add(1, (7, 9), (9, 9), bits=1)   # lengths without their bit count for nothing
    out.append(h)
    d = Case("descending frame offsets", [30, 30, 30], 12).add(0, (0, 30)).add(1, (0, 30)).add(2, (0, 30))
    d.offsets[1], d.offsets[2] = d.offsets[2], d.offsets[1]
    out.append(d)
    return out


CASES = cases()
IDS = [c.name for c in CASES]


def definition(case, n_entries=None, n_bytes=None, cursor=0, fill=0xEE):
    ne, nb = case.need()
    ent = np.frombuffer(bytes([fill]) * (64 * (ne if n_entries is None else n_entries)), dtype=E).copy()
    pay = np.full(cursor + nb if n_bytes is None else n_bytes, fill, np.uint8)
    return records.slab_store_np(*case.arrays(), ent, pay, cursor), (ent, pay)


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("cursor", [0, 5, 1024])
def test_placement_and_entries(case, cursor):
    (ent, pay, cur, cnt), (ent0, pay0) = definition(case, cursor=cursor)
    ops, refs, frames, fo = case.arrays()
    assert cnt["overflow"] == 0 and cnt["n_ops"] == len(ops) and cur == cnt["cursor"] == cursor + cnt["bytes_stored"]
    assert np.array_equal(pay[:cursor], pay0[:cursor])
    at, written = cursor, set()
    for op, ref in zip(ops, refs):
        if op["kind"] != C:
            continue
        e = ent[op["handle"]]
        written.add(int(op["handle"]))
        assert bytes(e["uuid"]) == uuid.UUID(int=(int(op["uuid_hi"]) << 64) | int(op["uuid_lo"])).bytes
        assert tuple(e["pos"]) == tuple(op["pos"]) and e["world"] == op["world"] and e["off"] == at
        assert e["bits"] == (int(ref["bits"]) & 3) | abi.SLAB_POSITION | abi.SLAB_LIVE
        for key, off, ln, bit in (("data_len", "data_off", "data_len", 1), ("flex_len", "flex_off", "flex_len", 2)):
            f = int(ref["frame"])
            inside = (int(ref["bits"]) & bit and f < len(fo) - 1 and fo[f] <= fo[f + 1]
                      and int(ref[off]) + int(ref[ln]) <= int(fo[f + 1]) - int(fo[f]))
            n = int(ref[ln]) if inside else 0
            assert e[key] == n
            a = int(fo[f]) + int(ref[off]) if n else 0
            assert np.array_equal(pay[at:at + n], frames[a:a + n])
            at += n
    assert at == cur
    for hd in range(len(ent)):
        if hd not in written:
            assert ent[hd] == ent0[hd]


def test_error_bits():
    h = next(c for c in CASES if c.name == "hostile references")
    (_, _, _, cnt), _ = definition(h)
    assert cnt["error"] == abi.SLAB_ERROR_FRAME | abi.SLAB_ERROR_DATA | abi.SLAB_ERROR_FLEX
    one = lambda **kw: definition(Case("x", [10, 10]).add(**kw))[0][3]   # noqa: E731
    assert one(frame=2, data=(0, 1))["error"] == abi.SLAB_ERROR_FRAME
    assert one(frame=2, data=(0, 0))["error"] == 0                       # nothing to copy: the frame is not looked at
    assert one(frame=0, data=(5, 6))["error"] == abi.SLAB_ERROR_DATA
    assert one(frame=1, data=(5, 5), flex=(10, 1))["error"] == abi.SLAB_ERROR_FLEX
    assert one(frame=1, data=(0, 10), flex=(0, 10))["error"] == 0
    d = next(c for c in CASES if c.name == "descending frame offsets")
    (ent, _, _, cnt), _ = definition(d)
    assert cnt["error"] == abi.SLAB_ERROR_FRAME and cnt["bytes_stored"] == 60 and ent[1]["data_len"] == 0
    assert ent[1]["bits"] & abi.SLAB_DATA   # present and empty


@pytest.mark.parametrize("case", [c for c in CASES if c.name in ("one of each", "deletes skipped", "0..40")], ids=lambda c: c.name)
def test_all_or_nothing(case):
    ne, nb = case.need()
    for kw, bit in ((dict(n_bytes=7 + nb - 1), 1), (dict(n_entries=ne - 1), 2), (dict(n_bytes=7, n_entries=0), 3),
                    (dict(n_bytes=6), 1)):
        (ent, pay, cur, cnt), (ent0, pay0) = definition(case, cursor=7, **dict(dict(n_bytes=7 + nb), **kw))
        assert cnt["overflow"] == bit and cur == cnt["cursor"] == 7
        assert cnt["bytes_need"] == 7 + nb and cnt["entries_need"] == ne and cnt["bytes_stored"] == nb
        assert np.array_equal(ent, ent0) and np.array_equal(pay, pay0)
    (_, _, cur, cnt), _ = definition(case, cursor=7, n_bytes=7 + nb, n_entries=ne)   # exactly enough
    assert cnt["overflow"] == 0 and cur == 7 + nb


def test_deletes_are_skipped():
    c = next(c for c in CASES if c.name == "deletes skipped")
    (ent, pay, cur, cnt), (ent0, _) = definition(c)
    assert cnt["n_creates"] == 2 and cnt["entries_need"] == 6 and cur == 16 + 3
    assert ent[0] == ent0[0] and ent[5]["data_len"] == 8 and ent[5]["flex_len"] == 8 and ent[2]["off"] == 16
