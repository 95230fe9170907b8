"""records.slab_compact_np, the definition of wq_slab_compact_device: placement in handle order, zeroed dead
entries, destinations longer and shorter than the source, all-or-nothing on both overflows, the sizing call,
hostile and shared ranges, idempotence and canonicity. No GPU needed. The case list is shared with
tests/test_slab_compact_cpp_mirror.py (the ops header on the CPU) and tests/test_gpu_slab_compact.py."""
import numpy as np
import pytest

from worldql_server_amd import abi, records

from test_slab_store_host import CASES as STORE_CASES

E, LIVE = abi.SLAB_ENTRY_DTYPE, abi.SLAB_LIVE


class Case:
    """A source slab: entries with random uuids, positions and worlds, and an arena of random bytes in which
    the payloads of the given (data_len, flex_len) pairs lie, dead ones included. order: the handles in arena
    order ("asc", "desc": how handles from a free list look, or "shuffle"); gap: junk bytes before each payload, so
    the sources sit at odd arena offsets."""

    def __init__(self, name, lens, live=None, order="asc", gap=0, seed=1, tail=0):
        self.name = name
        rng = np.random.default_rng(seed)
        n = len(lens)
        live = np.ones(n, bool) if live is None else np.asarray(live, bool)
        ent = np.zeros(n, E)
        ent["uuid"] = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        ent["pos"] = rng.integers(-500, 500, (n, 3)).astype(np.float64)
        ent["world"] = rng.integers(0, 5, n)
        dl = np.array([a for a, _ in lens], np.uint64).reshape(-1)
        fl = np.array([b for _, b in lens], np.uint64).reshape(-1)
        seq = {"asc": np.arange(n), "desc": np.arange(n)[::-1], "shuffle": rng.permutation(n)}[order]
        size = (dl + fl)[seq] + np.uint64(gap)
        start = np.concatenate([[0], np.cumsum(size)]).astype(np.uint64)
        ent["off"][seq] = start[:-1] + np.uint64(gap)
        ent["data_len"], ent["flex_len"] = dl, fl
        # a payload of length 0 is present or absent by the handle's parity
        ent["bits"] = (np.where((dl > 0) | (np.arange(n) % 2 == 0), abi.SLAB_DATA, 0) | np.where((fl > 0) | (np.arange(n) % 3 == 0), abi.SLAB_FLEX, 0)
                       | abi.SLAB_POSITION | np.where(live, LIVE, 0)).astype(np.uint32)
        self.entries = ent
        self.payload = rng.integers(0, 256, int(start[-1]) + tail, dtype=np.uint8)

    def need(self):
        """(entries, payload bytes) a destination needs."""
        c = records.slab_compact_np(self.entries, self.payload, 0, 0)[3]
        return c["entries_need"], c["bytes_live"]


def separated(run):
    """Live entries separated by runs of `run` dead ones."""
    live = np.zeros(3 * run + 4, bool)
    live[[0, run + 1, 2 * run + 2, 3 * run + 3]] = True
    return live


def hostile_case():
    c = Case("hostile ranges", [(10, 6)] * 9, seed=20, tail=5)
    n = len(c.payload)
    e = c.entries
    e["off"][1], e["data_len"][1], e["flex_len"][1] = n - 15, 10, 6            # off + len == n + 1
    e["off"][2] = n + 1                                                       # off > n
    e["off"][3], e["data_len"][3], e["flex_len"][3] = 2**64 - 8, 16, 0         # wraps in u64 when added
    e["off"][4], e["data_len"][4], e["flex_len"][4] = 0, 0xFFFFFFFF, 0xFFFFFFFF
    e["off"][5], e["data_len"][5], e["flex_len"][5] = n - 16, 10, 6            # ends with the arena: fine
    e["off"][6], e["data_len"][6], e["flex_len"][6] = n, 0, 0                  # empty at the end: fine
    e["off"][7], e["data_len"][7], e["flex_len"][7] = 2**64 - 1, 0, 0          # empty and outside
    e["off"][8], e["bits"][8] = 2**63, abi.SLAB_DATA                           # dead: not looked at
    return c


def shared_case():
    c = Case("shared and overlapping ranges", [(8, 8)] * 5, seed=21)
    c.entries["off"][[1, 3]] = c.entries["off"][0]       # three entries on one range
    c.entries["off"][4] = c.entries["off"][2] + 5         # and two that overlap
    c.payload = c.payload[:int(c.entries["off"][2]) + 21]
    return c


def cases():
    out = [Case("no entries", [])]
    for n in (1, 3, 63, 64, 65, 257, 5000):
        r = np.random.default_rng(n)
        lens = [(int(a), int(b)) for a, b in zip(r.integers(0, 24, n), r.integers(0, 9, n))]
        live = r.random(n) < 0.6 if n > 3 else None
        out.append(Case(f"{n} entries", lens, live, order="shuffle", gap=n % 3, seed=n))
    few = [(5, 3)] * 130
    out.append(Case("all live", few, None, seed=30))
    out.append(Case("none live", few, np.zeros(130, bool), seed=31))
    out.append(Case("alternating", few, np.arange(130) % 2 == 0, gap=1, seed=32))
    out.append(Case("only the first", few, np.arange(130) == 0, gap=3, seed=33))
    out.append(Case("only the last", few, np.arange(130) == 129, gap=3, seed=34))
    for run in (64, 65, 100000):
        live = separated(run)
        out.append(Case(f"runs of {run} dead", [(7, 2) if x else (0, 0) for x in live], live, gap=5, seed=run))
    out.append(Case("0..40", [(k, 0) if k % 2 else (0, k) for k in range(41)], gap=1, seed=40))
    out.append(Case("around a tile", [(n, 0) for n in (1022, 1023, 1024, 1025, 1026)], gap=3, seed=41))
    out.append(Case("around four tiles", [(4095, 0), (0, 4096), (4000, 97)], gap=7, seed=42))
    out.append(Case("a thousand without payload", [(0, 0)] * 1000 + [(300, 200)], seed=43))
    out.append(Case("two 1 MiB payloads", [(0, 1 << 20), (3, 0), (1 << 20, 0)], [True, False, True], order="desc", gap=9, seed=44))
    out.append(Case("1 MiB flex", [(80, 0), (17, 1 << 20), (5, 0)], gap=1, seed=45))
    out.append(Case("descending arena order", [(k % 50, k % 7) for k in range(200)], np.arange(200) % 5 != 1, order="desc", gap=1, seed=46))
    out.append(Case("trailing dead", [(9, 4)] * 40, np.arange(40) < 23, order="shuffle", seed=47))
    out.append(hostile_case())
    out.append(shared_case())
    return out


CASES = cases()
IDS = [c.name for c in CASES]
SMALL = [c for c in CASES if len(c.entries) <= 300]


def by_name(name):
    return next(c for c in CASES if c.name == name)


def definition(case, n_entries=None, n_bytes=None, fill=0xEE, cursor=77):
    """The call into a destination of `fill` bytes: (result, the destination before)."""
    ne, nb = case.need()
    ne, nb = ne if n_entries is None else n_entries, nb if n_bytes is None else n_bytes
    ent = np.frombuffer(bytes([fill]) * (64 * ne), dtype=E).copy()
    pay = np.full(nb, fill, np.uint8)
    return records.slab_compact_np(case.entries, case.payload, ne, nb, dst=(ent, pay, cursor)), (ent, pay, cursor)


def live_records(entries, payload):
    """{handle: (uuid, pos, world, bits, data, flex)} of the live entries whose range is inside."""
    out = {}
    for h, e in enumerate(entries):
        if int(e["bits"]) & LIVE:
            off, dl, fl = int(e["off"]), int(e["data_len"]), int(e["flex_len"])
            out[h] = (bytes(e["uuid"]), tuple(e["pos"]), int(e["world"]), int(e["bits"]), payload[off:off + dl].tobytes(),
                      payload[off + dl:off + dl + fl].tobytes())
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_placement_in_handle_order_and_zeroed_dead_entries(case):
    (ent, pay, cur, cnt), _ = definition(case, n_entries=len(case.entries) + 2)
    src, arena = case.entries, case.payload
    assert cnt["overflow"] == 0 and cnt["n_entries"] == len(src) and cur == cnt["bytes_live"] == len(pay)
    at, n_live, top = 0, 0, 0
    for h, e in enumerate(src):
        if not int(e["bits"]) & LIVE:
            assert ent[h].tobytes() == bytes(64)
            continue
        off, n = int(e["off"]), int(e["data_len"]) + int(e["flex_len"])
        inside = off + n <= len(arena)
        g = ent[h]
        assert g["off"] == at and g["bits"] == e["bits"] and bytes(g["uuid"]) == bytes(e["uuid"])
        assert g["pos"].tobytes() == e["pos"].tobytes() and g["world"] == e["world"]
        assert (int(g["data_len"]), int(g["flex_len"])) == ((int(e["data_len"]), int(e["flex_len"])) if inside else (0, 0))
        if inside:
            assert np.array_equal(pay[at:at + n], arena[off:off + n])
            at += n
        n_live, top = n_live + 1, h + 1
    assert at == cur and cnt["n_live"] == n_live and cnt["entries_need"] == top
    assert ent[len(src):].tobytes() == bytes(128)   # a destination longer than the source: zeros behind it


def test_arena_order_reversed():
    c = by_name("descending arena order")
    live = np.flatnonzero(c.entries["bits"] & LIVE)
    assert (np.diff(c.entries["off"][live].astype(np.int64)) < 0).all()        # the source: descending
    (ent, _, _, _), _ = definition(c)
    assert (np.diff(ent["off"][live].astype(np.int64)) >= 0).all() and ent["off"][live[0]] == 0


def test_shorter_destination_trims_trailing_dead():
    c = by_name("trailing dead")
    assert c.need()[0] == 23 < len(c.entries)
    (ent, pay, cur, cnt), _ = definition(c)
    assert len(ent) == 23 and cnt["overflow"] == 0 and cnt["n_entries"] == 40
    (ent40, pay40, _, _), _ = definition(c, n_entries=40)
    assert ent40[:23].tobytes() == ent.tobytes() and ent40[23:].tobytes() == bytes(64 * 17) and np.array_equal(pay, pay40)


@pytest.mark.parametrize("case", [c for c in SMALL if c.need()[0]], ids=lambda c: c.name)
def test_all_or_nothing(case):
    ne, nb = case.need()
    trials = [(dict(n_entries=ne - 1), 2), (dict(n_entries=0), 2)]
    if nb:
        trials += [(dict(n_bytes=nb - 1), 1), (dict(n_bytes=0), 1), (dict(n_bytes=nb - 1, n_entries=ne - 1), 3)]
    for kw, bit in trials:
        (ent, pay, cur, cnt), (ent0, pay0, cur0) = definition(case, **kw)
        assert cnt["overflow"] == bit and cur == cur0 == 77
        assert cnt["bytes_live"] == nb and cnt["entries_need"] == ne
        assert ent.tobytes() == ent0.tobytes() and np.array_equal(pay, pay0)
    (_, _, cur, cnt), _ = definition(case)   # exactly enough
    assert cnt["overflow"] == 0 and cur == nb


def test_sizing_call():
    c = by_name("257 entries")
    ent, pay, cur, cnt = records.slab_compact_np(c.entries, c.payload, 0, 0)
    assert len(ent) == 0 and len(pay) == 0 and cur == 0 and cnt["overflow"] == 3
    assert (cnt["entries_need"], cnt["bytes_live"]) == c.need() and cnt["bytes_live"] > 1000
    got = records.slab_compact_np(c.entries, c.payload, cnt["entries_need"], cnt["bytes_live"])
    assert got[3]["overflow"] == 0 and got[2] == cnt["bytes_live"]
    none = by_name("none live")
    assert records.slab_compact_np(none.entries, none.payload, 0, 0)[3] == dict(
        n_entries=130, n_live=0, bytes_live=0, entries_need=0, overflow=0, error=0)


def test_hostile_ranges():
    c = hostile_case()
    (ent, pay, cur, cnt), _ = definition(c)
    assert cnt["error"] == abi.SLAB_COMPACT_ERROR_RANGE and cnt["n_live"] == 8 and cnt["entries_need"] == 8
    assert cur == 16 + 16 + 0 == cnt["bytes_live"]       # handles 0 and 5; 6 is empty
    for h in (1, 2, 3, 4, 7):
        assert ent[h]["bits"] == c.entries[h]["bits"] and ent[h]["data_len"] == 0 and ent[h]["flex_len"] == 0
        assert ent[h]["off"] == (16 if h < 5 else 32)
    n = len(c.payload)
    assert ent[5]["off"] == 16 and np.array_equal(pay[16:32], c.payload[n - 16:]) and ent[6]["off"] == 32
    # each hostile shape alone sets the bit; none alone does not
    for h, bad in ((1, True), (2, True), (3, True), (4, True), (7, True), (5, False), (6, False), (8, False)):
        one = hostile_case()
        keep = one.entries[h].copy()
        one.entries["bits"] &= ~np.uint32(LIVE)
        one.entries[h] = keep
        assert (records.slab_compact_np(one.entries, one.payload, 9, 64)[3]["error"] != 0) == bad, h


def test_shared_ranges_are_each_copied():
    c = shared_case()
    (ent, pay, cur, cnt), _ = definition(c)
    assert cnt["error"] == 0 and cur == 5 * 16 > len(c.payload)
    a = int(c.entries["off"][0])
    for h in (0, 1, 3):
        assert np.array_equal(pay[16 * h:16 * h + 16], c.payload[a:a + 16])
    assert np.array_equal(pay[64:80], c.payload[int(c.entries["off"][4]):][:16])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_idempotent(case):
    (ent, pay, cur, cnt), _ = definition(case)
    again = records.slab_compact_np(ent, pay, len(ent), len(pay))
    assert again[0].tobytes() == ent.tobytes() and np.array_equal(again[1], pay) and again[2] == cur
    assert again[3] == dict(cnt, n_entries=len(ent), error=0)


def test_two_histories_with_equal_live_records_compact_to_equal_bytes():
    """Stores and frees in two orders, through slab_store_np: the same live records under the same handles, other
    arenas; the canonical forms are equal bytes."""
    a, b = (next(c for c in STORE_CASES if c.name == n) for n in ("0..40", "one of each"))

    def shifted(case, by):
        ops, refs, frames, fo = case.arrays()
        ops = ops.copy()
        ops["handle"] += by
        return ops, refs, frames, fo

    def free(ent, handles):
        ent["bits"][handles] &= ~np.uint32(LIVE)

    # history 1: a, then b behind it; free some of each
    ent, pay, cur = np.zeros(64, E), np.zeros(4096, np.uint8), 0
    ent, pay, cur, _ = records.slab_store_np(*shifted(a, 0), ent, pay, cur)
    ent, pay, cur, _ = records.slab_store_np(*shifted(b, 41), ent, pay, cur)
    free(ent, [3, 4, 10, 42])
    one = (ent, pay[:cur])
    # history 2: b first, a twice (the first copy freed whole, then overwritten), the same frees, a larger slab
    ent, pay, cur = np.zeros(90, E), np.full(8192, 0x5A, np.uint8), 13
    ent, pay, cur, _ = records.slab_store_np(*shifted(b, 41), ent, pay, cur)
    ent, pay, cur, _ = records.slab_store_np(*shifted(a, 0), ent, pay, cur)
    free(ent, list(range(41)))
    ent, pay, cur, _ = records.slab_store_np(*shifted(a, 0), ent, pay, cur)
    free(ent, [42, 10, 4, 3])
    two = (ent, pay[:cur])
    assert live_records(*one) == live_records(*two) and len(two[1]) > len(one[1])
    ne, nb = records.slab_compact_np(*one, 0, 0)[3]["entries_need"], records.slab_compact_np(*one, 0, 0)[3]["bytes_live"]
    c1, c2 = records.slab_compact_np(*one, ne, nb), records.slab_compact_np(*two, ne, nb)
    assert c1[3]["overflow"] == 0 and c1[0].tobytes() == c2[0].tobytes() and np.array_equal(c1[1], c2[1]) and c1[2] == c2[2] == nb
    assert live_records(c1[0], c1[1]) == live_records(*one)


def test_snapshot_file_round_trip(tmp_path):
    c = by_name("65 entries")
    ent, pay, _, _ = records.slab_compact_np(c.entries, c.payload, *c.need())
    rows = np.zeros(3, records.REC_ROW_DTYPE)
    rows["handle"], rows["seq"] = [4, 9, 2], [1, 2, 3]
    names = [b"world", b"", b"caf\xc3\xa9"]
    snap = dict(rows=rows, ops_seen=np.array([17], np.uint64), store_shape=np.array([16, 16, 16, 1024], np.uint32),
                dedupe=np.array([1], np.uint8), slab_entries=ent, slab_payload=pay, free=np.array([7, 3], np.uint32),
                next=np.array([65], np.uint64), totals=np.arange(5, dtype=np.uint64),
                world_bytes=np.frombuffer(b"".join(names), np.uint8), world_off=np.array([0, 5, 5, 10], np.uint64))
    path = tmp_path / "records.npz"
    records.save_snapshot(path, snap)
    got = records.load_snapshot(path)
    assert set(got) == set(snap)
    for k, v in snap.items():
        assert got[k].dtype == v.dtype and got[k].tobytes() == v.tobytes(), k
    np.savez(tmp_path / "other.npz", rows=np.zeros(3))
    with pytest.raises(ValueError):
        records.load_snapshot(tmp_path / "other.npz")
