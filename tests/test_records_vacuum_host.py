"""Vacuum, export and import of the record store on the CPU (worldql_server_amd/records.py
RecordStoreRef.vacuum / export_rows / import_rows).

The property that carries the weight is invisibility: every shared script of test_records_host.py
cases(), replayed with a vacuum after step k (every k on the small scripts, every 5th step on
random_stream), returns byte for byte what wants() holds: offsets, handles, ts_us, the result
counters, the drained dead list, at the end the totals; rows_stored == rows_live straight after each
vacuum. The same with "drain, export, open a second store, import, go on there" in place of the
vacuum. The hand-written cases compare a store that vacuums with a twin that never does.

`replay` and the `case_*` functions are shared: test_gpu_records_vacuum.py runs them on the GPU store
through an adapter with RefStore's interface.
"""
import itertools

import numpy as np
import pytest

from worldql_server_amd import records as R

from test_records_host import CFG, cases, region_kats, ref_step, wants

CFG16 = (16, 16, 16, 1024)
READ_KEYS = ("returned", "deduped_rows", "rejected", "scanned", "overflow", "error")


class RefStore:
    """RecordStoreRef behind the interface the shared cases use."""
    refused = ValueError

    def __init__(self, cfg):
        self.cfg, self.s = tuple(cfg), R.RecordStoreRef(*cfg)
        self.raw = self.s  # what a RecordProcessor takes

    def step(self, step, want_res):
        return ref_step(self.s, step)

    def read(self, qs, dedupe=False):
        return self.s.read([(w, p, None) for w, p in qs], dedupe=dedupe)

    def close(self):
        pass

    def __getattr__(self, name):
        return getattr(self.s, name)


def open_ref(cfg, which=0):
    return RefStore(cfg)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


def same_result(got, want, what):
    """A call's result against the reference's: arrays byte for byte, counters as integers."""
    if "offsets" in want:
        for k in READ_KEYS:
            assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
        for k in ("offsets", "handles", "ts_us"):
            same(got[k], want[k], (what, k))
    else:
        assert {k: int(v) for k, v in got.items()} == {k: int(v) for k, v in want.items()}, what


def add_totals(a, b):
    return {k: a[k] + b[k] for k in a}


def replay(open_store, name, form, points):
    """The script `name` with a vacuum (form "vacuum") or an export / import into a second store
    (form "snapshot") after every step in `points`; everything compared with wants() after every
    step. Returns how many rows the vacuums dropped or the snapshots left behind."""
    s = cases()[name]
    res, ref = wants()[name]
    store, which = open_store(s.cfg, 0), 0
    totals = {k: 0 for k in ref.totals()}
    dropped = 0
    try:
        for i, (step, (w_res, w_dead, w_stats)) in enumerate(zip(s.steps, res)):
            what = (name, form, sorted(points)[:3], i, step[0])
            same_result(store.step(step, w_res), w_res, what)
            same(store.drain_dead(), w_dead, (what, "dead list"))
            live, stored, ops = store.stats()
            assert (live, ops) == (int(w_stats[0]), int(w_stats[2])) and stored <= int(w_stats[1]), (what, "stats")
            if i not in points:
                continue
            if form == "vacuum":
                v = store.vacuum()
                assert v["rows_before"] == stored and v["rows_after"] == live, (what, v)
            else:
                rows, ops_seen = store.export_rows()
                assert len(rows) == live and ops_seen == ops, what
                assert (np.diff(rows["seq"].astype(np.int64)) > 0).all(), (what, "row order")
                totals = add_totals(totals, store.totals())
                store.close()
                which ^= 1
                store = open_store(s.cfg, which)
                assert store.import_rows(rows, ops_seen) == {"imported": live, "rejected": 0}, what
                assert all(v == 0 for v in store.totals().values()), (what, "a snapshot carries no history")
            dropped += stored - live
            assert store.stats() == (live, live, ops), (what, "stats after")
        assert add_totals(totals, store.totals()) == ref.totals(), (name, form, "totals")
    finally:
        store.close()
    return dropped


def points_of(name):
    """Where the vacuums go: after every 5th step of random_stream, else one run per step."""
    n = len(cases()[name].steps)
    if name == "random_stream":
        return [set(range(4, n, 5))]
    return [{k} for k in range(n)]


@pytest.mark.parametrize("form", ["vacuum", "snapshot"])
@pytest.mark.parametrize("name", sorted(cases()))
def test_invisible_in_every_shared_script(name, form):
    dropped = sum(replay(open_ref, name, form, pts) for pts in points_of(name))
    if name in ("random_stream", "deletes", "duplicates", "capacity", "one_region_many_queries"):
        assert dropped > 0, "the script has dead rows to drop"


# ---- hand-written cases: the store under test vacuums, its twin (a RecordStoreRef) never does ----

P = (1.0, 1.0, 1.0)


def creates(n, first=0, pos=P, ts=10):
    return R.make_ops(R.CREATE, 0, [pos] * n, 0, np.arange(first, first + n), ts, np.arange(first, first + n))


def deletes(uuids, pos=P):
    return R.make_ops(R.DELETE, 0, [pos] * len(uuids), 0, np.asarray(uuids, dtype=np.uint64))


def agree(store, twin, qs, what, dedupe=False):
    """A read, the drained dead list, the live count, the op counter and a snapshot: all as the twin's."""
    a, b = store.read(qs, dedupe=dedupe), twin.read([(w, p, None) for w, p in qs], dedupe=dedupe)
    same_result(a, b, what)
    same(store.drain_dead(), twin.drain_dead(), (what, "dead"))
    assert (store.stats()[0], store.stats()[2]) == (twin.stats()[0], twin.stats()[2]), what
    rows, ops_seen = store.export_rows()
    t_rows, t_ops = twin.export_rows()
    same(rows, t_rows, (what, "snapshot"))
    assert ops_seen == t_ops, what


def case_small_stores(open_store):
    """1, 2, 3, 5 and 7 rows (no multiple of 4: the dead share live words with the living), every
    subset dead at 3 rows; the vacuum runs between the delete and the next read (views still dirty)
    and with the dead handles undrained; then an apply grows the shrunk arrays."""
    for n in (1, 2, 3, 5, 7):
        masks = list(itertools.product((0, 1), repeat=n)) if n == 3 else \
            [(0,) * n, (1,) * n, tuple(i % 2 for i in range(n)), (1,) + (0,) * (n - 1), (0,) * (n - 1) + (1,)]
        for mask in masks:
            store, twin = open_store(CFG, 0), R.RecordStoreRef(*CFG)
            try:
                dead = [i for i in range(n) if mask[i]]
                for st in (store, twin):
                    st.apply(creates(n))
                    st.apply(deletes(dead))
                v = store.vacuum()
                assert (v["rows_before"], v["rows_after"]) == (n, n - len(dead)), (n, mask)
                assert store.stats() == (n - len(dead), n - len(dead), n + len(dead))
                agree(store, twin, [(0, P)], (n, mask, "after the vacuum"))  # the undrained handles too
                for st in (store, twin):
                    st.apply(creates(1500, first=100))  # past the shrunk capacity
                    st.apply(deletes([100, 1599] + [i for i in range(n) if not mask[i]][:1]))
                agree(store, twin, [(0, P)], (n, mask, "after the growth"))
                assert store.vacuum()["rows_after"] == twin.stats()[0]
                agree(store, twin, [(0, P)], (n, mask, "after the second vacuum"))
            finally:
                store.close()


def case_none_dead_and_twice(open_store):
    """Nothing dead: the vacuum is the identity and the export the input order. Twice: the same."""
    store, twin = open_store(CFG, 0), R.RecordStoreRef(*CFG)
    try:
        ops = R.make_ops(R.CREATE, [0, 1, 0, 2, 0], [P, P, (17.0, 1.0, 1.0), P, (-1.0, -1.0, -1.0)], [3, 1, 4, 1, 5],
                         [9, 2, 6, 5, 3], [50, 40, 30, 20, 10], [0, 1, 2, 3, 4])
        for st in (store, twin):
            st.apply(ops)
        before = store.export_rows()[0]
        assert list(before["handle"]) == [0, 1, 2, 3, 4] and list(before["seq"]) == [0, 1, 2, 3, 4]
        assert list(before["ts_us"]) == [50, 40, 30, 20, 10] and list(before["world"]) == [0, 1, 0, 2, 0]
        for _ in range(2):
            v = store.vacuum()
            assert v["rows_before"] == v["rows_after"] == 5
            if "bytes_before" in v:
                assert v["bytes_before"] == v["bytes_after"]
            same(store.export_rows()[0], before, "identity")
        agree(store, twin, [(0, P), (1, P), (0, (-1.0, -1.0, -1.0))], "none dead")
        for st in (store, twin):
            st.apply(R.make_ops(R.DELETE, 0, [P], 3, 9))
        for _ in range(2):  # the second finds nothing dead
            assert store.vacuum()["rows_after"] == 4
        agree(store, twin, [(0, P), (1, P)], "twice")
    finally:
        store.close()
    store = open_store(CFG, 0)
    try:  # an empty store
        assert store.vacuum()["rows_after"] == 0 and store.stats() == (0, 0, 0) and len(store.export_rows()[0]) == 0
    finally:
        store.close()


def case_all_dead(open_store):
    store, twin = open_store(CFG, 0), R.RecordStoreRef(*CFG)
    try:
        for st in (store, twin):
            st.apply(creates(6))
            st.apply(deletes(range(6)))
        assert store.vacuum()["rows_after"] == 0 and store.stats() == (0, 0, 12)
        agree(store, twin, [(0, P)], "all dead")
        for st in (store, twin):
            st.apply(creates(3, first=50, ts=7))
        agree(store, twin, [(0, P)], "rows after all died")
        assert list(store.export_rows()[0]["seq"]) == [12, 13, 14]
    finally:
        store.close()


def case_dedupe_then_vacuum(open_store):
    """Rows killed by a read's dedupe leave with the vacuum; the winner and equal-time order stay."""
    store, twin = open_store(CFG, 0), R.RecordStoreRef(*CFG)
    try:
        ops = R.make_ops(R.CREATE, 0, [P] * 6, 0, [1, 1, 1, 2, 2, 3], [50, 50, 40, 9, 8, 1], [0, 1, 2, 3, 4, 5])
        for st in (store, twin):
            st.apply(ops)
        agree(store, twin, [(0, P)], "dedupe", dedupe=True)
        assert store.vacuum()["rows_after"] == 4  # the equal-time pair both survive
        agree(store, twin, [(0, P)], "after", dedupe=True)
        same(store.read([(0, P)])["handles"], np.array([1, 3, 5], np.uint32), "winners")
    finally:
        store.close()


def case_export_regions(open_store):
    """Negative regions export the corner the reference's own vectors give; rows ascend in seq."""
    conv = region_kats()["conversion"]
    sizes = tuple(conv["region_sizes"])
    store = open_store(sizes + (1024,), 0)
    try:
        pos = [c[0] for c in conv["cases"]] + [(-16.0, -0.1, -15.5), (-0.0, -256.0, 15.9)]
        want = [c[1] for c in conv["cases"]] + [[R.region_coord(c, s) for c, s in zip(p, sizes)] for p in pos[-2:]]
        assert any(v < 0 for w in want for v in w)
        n = len(pos)
        res = store.apply(R.make_ops(R.CREATE, 3, pos, 7, np.arange(n), np.arange(n) + 100, np.arange(n) + 1000))
        assert res["created"] == n
        rows, ops_seen = store.export_rows()
        assert ops_seen == n and rows["region"].tolist() == want
        assert list(rows["seq"]) == list(range(n)) and list(rows["handle"]) == list(range(1000, 1000 + n))
        assert (rows["world"] == 3).all() and (rows["uuid_hi"] == 7).all() and list(rows["ts_us"]) == list(range(100, 100 + n))
        same(store.export_rows()[0], rows, "two exports, the same bytes")
    finally:
        store.close()


def snapshot_rows(rows):
    """REC_ROW_DTYPE from (world, handle, region, uuid_hi, uuid_lo, ts, seq) tuples."""
    out = np.zeros(len(rows), dtype=R.REC_ROW_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def case_import_rejections(open_store):
    top = (1 << 23) * 16
    good = (0, 5, (16, -32, 0), 1, 2, 10, 3)
    rows = snapshot_rows([
        good,
        (0, 6, (8, 0, 0), 1, 3, 10, 4),            # a corner off the grid
        (0, 7, (0, 0, -17), 1, 3, 10, 4),
        (0, 8, (top, 0, 0), 1, 4, 10, 5),          # region index 2^23
        (0, 9, (0, -top - 16, 0), 1, 4, 10, 5),    # region index -2^23 - 1
        ((1 << 24) - 1, 10, (0, 0, 0), 1, 5, 10, 6),  # a world without a packed key
        (0, 11, (0, 0, 0), 1, 6, 10, 20),          # seq == ops_seen
        (0, 12, (0, 0, 0), 1, 6, 10, 21),
        ((1 << 24) - 2, 13, (top - 16, -top, 0), 1, 7, 10, 19),  # the last world, the extreme indices: taken
    ])
    store = open_store(CFG16, 0)
    try:
        assert store.import_rows(rows, 20) == {"imported": 2, "rejected": 7}
        assert store.stats() == (2, 2, 20) and all(v == 0 for v in store.totals().values())
        same(store.export_rows()[0], rows[[0, 8]], "the accepted rows, as given")
        same(store.read([(0, (17.0, -20.0, 1.0))])["handles"], np.array([5], np.uint32), "found by position")
        with pytest.raises(store.refused):  # a used store
            store.import_rows(rows[:1], 20)
        assert store.stats() == (2, 2, 20)
    finally:
        store.close()
    store = open_store(CFG16, 0)
    try:
        dup = snapshot_rows([good, (0, 6, (16, -32, 16), 1, 2, 10, 3), (0, 99, (16, -32, 0), 1, 2, 10, 3)])
        with pytest.raises(store.refused):  # rows 0 and 2 share the full key (the handle is no part of it)
            store.import_rows(dup, 20)
        assert store.stats() == (0, 0, 0) and len(store.export_rows()[0]) == 0 and len(store.drain_dead()) == 0
        assert store.read([(0, (17.0, -20.0, 1.0))])["returned"] == 0
        assert store.import_rows(dup[:2], 20) == {"imported": 2, "rejected": 0}  # still unused: it takes a snapshot
        assert store.stats() == (2, 2, 20)
        store.apply(creates(1))
        with pytest.raises(store.refused):
            store.import_rows(dup[:1], 30)
    finally:
        store.close()
    store = open_store(CFG16, 0)
    try:  # an op makes a store used, rows or not
        store.apply(R.make_ops(R.CREATE, 0, [(float("nan"), 0.0, 0.0)], 0, 1, 1, 1))
        with pytest.raises(store.refused):
            store.import_rows(rows[:1], 20)
    finally:
        store.close()


def case_import_other_sizes(open_store):
    """The tables are the target's: x regions 1008 | 1024 lie in two tables of 1,024 and in one of
    2,048, so the dedupe across that border acts in the second store only. A target with regions of
    32 along x takes the corners on its grid and counts the rest."""
    A, B = (1010.0, 0.0, 0.0), (1030.0, 0.0, 0.0)
    src = open_store(CFG16, 0)
    try:
        src.apply(R.make_ops(R.CREATE, 0, [A, B, A], 0, [1, 1, 2], [10, 20, 5], [0, 1, 2]))
        assert src.read([(0, B)], dedupe=True)["deduped_rows"] == 0
        rows, ops_seen = src.export_rows()
        assert rows["region"].tolist() == [[1008, 0, 0], [1024, 0, 0], [1008, 0, 0]]
    finally:
        src.close()
    wide, twin = open_store((16, 16, 16, 2048), 1), R.RecordStoreRef(16, 16, 16, 2048)
    try:
        for st in (wide, twin):
            assert st.import_rows(rows, ops_seen) == {"imported": 3, "rejected": 0}
        r = wide.read([(0, B)], dedupe=True)
        assert r["deduped_rows"] == 1 and list(wide.drain_dead()) == [0]
        twin.read([(0, B, None)], dedupe=True), twin.drain_dead()
        agree(wide, twin, [(0, A), (0, B)], "one table now")
        for st in (wide, twin):
            st.apply(R.make_ops(R.CREATE, 0, [A], 0, 2, 6, 7))  # the next op is number ops_seen
        assert list(wide.export_rows()[0]["seq"]) == [1, 2, 3]
        agree(wide, twin, [(0, A)], "an apply after the import", dedupe=True)
    finally:
        wide.close()
    coarse = open_store((32, 16, 16, 1024), 0)
    try:
        assert coarse.import_rows(rows, ops_seen) == {"imported": 1, "rejected": 2}  # 1008 is off a grid of 32
        assert coarse.read([(0, (1050.0, 0.0, 0.0))])["returned"] == 1
    finally:
        coarse.close()


def case_equal_times_keep_their_winner(open_store):
    """seq is preserved, so among equal times the op met later still wins after an export and an
    import; the given order of the rows does not matter, only their seq."""
    a = open_store(CFG, 0)
    try:
        a.apply(R.make_ops(R.CREATE, 0, [P] * 4, 0, [9, 9, 9, 4], [50, 50, 50, 1], [0, 1, 2, 3]))
        assert list(a.read([(0, P)])["handles"]) == [3, 2]
        rows, ops_seen = a.export_rows()
    finally:
        a.close()
    for order in ([0, 1, 2, 3], [2, 3, 1, 0], [1, 0, 3, 2]):
        b = open_store(CFG, 1)
        try:
            assert b.import_rows(rows[order], ops_seen)["imported"] == 4
            same(b.export_rows()[0], rows[order], "stored in the given order")
            r = b.read([(0, P)], dedupe=True)
            assert list(r["handles"]) == [3, 2] and r["deduped_rows"] == 0
            b.apply(R.make_ops(R.CREATE, 0, [P], 0, 9, 50, 8))  # the same time again: met later still
            assert list(b.read([(0, P)])["handles"]) == [3, 8]
        finally:
            b.close()


def case_processor_vacuums_unseen(open_store):
    """RecordProcessor with vacuum_dead_fraction replies exactly as without it."""
    rec = lambda u, pos, data: {"uuid": (0, u), "world_name": "w", "position": pos, "data": data, "flex": None}
    ev = lambda ins, records=(), position=None: {"instruction": ins, "world_name": "w", "sender_uuid": b"s" * 16,
                                                 "parameter": None, "position": position, "records": list(records)}
    A, B = (3.0, 0.0, 0.0), (19.0, 0.0, 0.0)
    ticks = [[ev("RecordCreate", [rec(u, A, f"a{u}.0") for u in range(30)] + [rec(1, B, "b1")])]]
    for t in range(1, 6):  # every tick re-creates the records, reads them (dedupe) and deletes a few
        ticks.append([ev("RecordCreate", [rec(u, A, f"a{u}.{t}") for u in range(30)]), ev("RecordRead", position=A),
                      ev("RecordDelete", [rec(t, A, None)]), ev("RecordRead", position=A), ev("RecordRead", position=B)])
    store = open_store(CFG, 0)
    try:
        plain, vac = R.RecordProcessor(R.RecordStoreRef(*CFG)), R.RecordProcessor(store.raw, vacuum_dead_fraction=0.25)
        for i, tick in enumerate(ticks):
            a, b = plain.process(tick, now_us=1000 * (i + 1)), vac.process(tick, now_us=1000 * (i + 1))
            assert [(s, w, [r["data"] for r in rs]) for s, w, rs in a] == [(s, w, [r["data"] for r in rs]) for s, w, rs in b]
            assert sorted(plain.free) == sorted(vac.free) and plain.dropped == vac.dropped
            assert plain.store.stats()[0] == store.stats()[0]
        assert vac.vacuums >= 3 and plain.vacuums == 0 and store.stats()[1] < plain.store.stats()[1]
        assert len(a) == 2  # both reads of A; B's copy of uuid 1 died by the dedupe of a newer one in A
    finally:
        store.close()


CASES = [case_small_stores, case_none_dead_and_twice, case_all_dead, case_dedupe_then_vacuum, case_export_regions,
         case_import_rejections, case_import_other_sizes, case_equal_times_keep_their_winner,
         case_processor_vacuums_unseen]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_hand_written(case):
    case(open_ref)


def test_vacuum_drops_the_lookup_entries_too():
    """After a vacuum the definition holds live rows only, in the lookups as well."""
    ref = R.RecordStoreRef(*CFG)
    ref.apply(creates(8))
    ref.apply(deletes([0, 3, 7]))
    ref.vacuum()
    assert [r["handle"] for r in ref.rows] == [1, 2, 4, 5, 6] and all(r["live"] for r in ref.rows)
    assert sorted(i for v in ref.by_region.values() for i in v) == [0, 1, 2, 3, 4]
    assert sorted(i for v in ref.by_table_uuid.values() for i in v) == [0, 1, 2, 3, 4]
    assert list(ref.drain_dead()) == [0, 3, 7]
