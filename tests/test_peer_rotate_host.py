"""The host definition of the fair share (worldql_server_amd/interest.py peer_rotate_np) against a
deliberately naive restatement: per row, Python lists, a merge of the kept row into the full one and an
explicit rotation of the cut list. `cases()` is shared with the C++ mirror
(tests/test_peer_rotate_cpp_mirror.py) and the GPU instance (tests/test_gpu_peer_rotate.py). No GPU
needed.

A case is the argument list of one wq_peer_rotate_device call: the full CSR (offsets, msgs), the kept
CSR (koffsets, kmsgs), the cursors before the call, r or the per-peer extra, and optionally msg_size
with v or the per-peer extra_bytes; and its kind: "exact" (offsets that ascend in both CSRs and rows
that ascend: the bytes are peer_rotate_np's) or "hostile" (offsets that descend, wrap or pass their
array, or rows that do not ascend: `well_formed` states what include/wq_router.h promises then, and
the bytes are still the definition's wherever every walked row ascends, see `rows_ascend`)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from worldql_server_amd import interest

U32_MAX = 0xFFFFFFFF
# csrc/rotate_ops.hpp (the C++ mirror checks them against the shim's exports):
GRANULE = 64       # kRotGranule: the cut and keep flags are one word per this many ordinals
TILE = 256         # kRotTile: ordinals per block
EDGE_LENS = [0, 1, 2, 63, 64, 65, 255, 256, 257]


def _csr(rows):
    offsets = np.zeros(len(rows) + 1, dtype=np.uint32)
    if rows:
        np.cumsum([len(r) for r in rows], out=offsets[1:])
    msgs = np.concatenate([np.asarray(r, dtype=np.uint32) for r in rows]) if rows else np.zeros(0, np.uint32)
    return offsets, msgs.astype(np.uint32)


def _rows(rng, lengths, n_msgs):
    """Ascending distinct message indices per row, as wq_peer_major_device writes them."""
    return [np.sort(rng.choice(n_msgs, size=n, replace=False)).astype(np.uint32) for n in lengths]


def _subset(rng, row, k):
    """k elements of the row, in the row's order: what a budget leaves."""
    row = np.asarray(row, dtype=np.uint32)
    if k >= len(row):
        return row.copy()
    return row[np.sort(rng.choice(len(row), size=k, replace=False))]


def _cut_counts(rows, krows):
    """T per row for ascending rows: len - sum over values of min(cf, ck)."""
    out = []
    for row, krow in zip(rows, krows):
        vals, cf = np.unique(np.asarray(row, dtype=np.int64), return_counts=True)
        kv, ck = np.unique(np.asarray(krow, dtype=np.int64), return_counts=True)
        have = dict(zip(kv.tolist(), ck.tolist()))
        out.append(int(sum(c - min(c, have.get(v, 0)) for v, c in zip(vals.tolist(), cf.tolist()))))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> SimpleNamespace(offsets, msgs, n_peers, koffsets, kmsgs, cursor, r, extra, msg_size, v,
    extra_bytes, kind); built once, never modified (the arrays are read-only)."""
    rng = np.random.default_rng(61)
    out = {}

    def add(name, full, kept, cursor, r=0, extra=None, msg_size=None, v=0, extra_bytes=None, kind="exact"):
        offsets, msgs = (np.ascontiguousarray(a, np.uint32) for a in full)
        koffsets, kmsgs = (np.ascontiguousarray(a, np.uint32) for a in kept)
        n_peers = len(offsets) - 1
        assert len(koffsets) == n_peers + 1
        cursor = np.ascontiguousarray(np.broadcast_to(np.asarray(cursor, dtype=np.uint32), (n_peers,)))
        arrays = [offsets, msgs, koffsets, kmsgs, cursor]
        if extra is not None:
            extra = np.ascontiguousarray(extra, np.uint32)
            assert len(extra) == n_peers
            arrays.append(extra)
        if msg_size is not None:
            msg_size = np.ascontiguousarray(msg_size, np.uint32)
            arrays.append(msg_size)
        if extra_bytes is not None:
            assert msg_size is not None
            extra_bytes = np.ascontiguousarray(extra_bytes, np.uint64)
            assert len(extra_bytes) == n_peers
            arrays.append(extra_bytes)
        for a in arrays:
            a.setflags(write=False)
        assert name not in out
        out[name] = SimpleNamespace(offsets=offsets, msgs=msgs, n_peers=n_peers, koffsets=koffsets, kmsgs=kmsgs,
                                    cursor=cursor, r=int(r), extra=extra, msg_size=msg_size, v=int(v),
                                    extra_bytes=extra_bytes, kind=kind)

    # ---- row lengths around the granule and the tile, R around every row's T
    n_msgs = 600
    rows = _rows(rng, EDGE_LENS + [70, 5], n_msgs)
    sizes = rng.integers(1, 300, size=n_msgs).astype(np.uint32)
    for tag, krows in (("kept_some", [_subset(rng, r, len(r) // 3) for r in rows]),
                       ("kept_none", [r[:0] for r in rows]),
                       ("kept_all", [r.copy() for r in rows]),
                       ("kept_but_one", [_subset(rng, r, max(len(r) - 1, 0)) for r in rows])):
        T = _cut_counts(rows, krows)
        curs = rng.integers(0, n_msgs, size=len(rows)).astype(np.uint32)
        for rname, r in (("r0", 0), ("r1", 1), ("r3", 3), ("rmax", U32_MAX)):
            add(f"lens_{tag}_{rname}", _csr(rows), _csr(krows), curs, r=r)
        for rname, extra in (("Tm1", [max(t - 1, 0) for t in T]), ("T", T), ("Tp1", [t + 1 for t in T])):
            add(f"lens_{tag}_extra_{rname}", _csr(rows), _csr(krows), curs, r=9, extra=extra)
        add(f"lens_{tag}_sizes", _csr(rows), _csr(krows), curs, r=40, msg_size=sizes, v=1500)
    add("extra_mixed", _csr(rows), _csr([_subset(rng, r, 4) for r in rows]), U32_MAX,
        r=5, extra=[0, 1, U32_MAX, 2, 0, 7, 300, 1, U32_MAX, 3, 2])

    # ---- the cursor: below the first element, equal to a cut one, equal to a kept one, between two,
    # equal to the last, above the last, 0xFFFFFFFF
    base = np.arange(10, 10 + 3 * 40, 3, dtype=np.uint32)          # 10, 13, ..., 127
    kept = base[::4]                                               # 10, 22, ...: kept; the others cut
    places = {"below": 3, "on_cut": 13, "on_kept": 22, "between": 24, "on_last": 127, "above": 500, "max": U32_MAX,
              "zero": 0}
    for r in (1, 3, 29, 30, 31):
        add(f"cursor_places_r{r}", _csr([base] * len(places)), _csr([kept] * len(places)), list(places.values()), r=r)
    add("cursor_places_sizes", _csr([base] * len(places)), _csr([kept] * len(places)), list(places.values()), r=6,
        msg_size=np.full(200, 100, np.uint32), v=350)

    # ---- one long row among empty rows
    for n_long in (5_000, 70_000):
        lens = [0] * 40
        lens[17] = n_long
        lrows = _rows(rng, lens, 100_000)
        lkept = [_subset(rng, r, min(len(r), 100)) for r in lrows]
        lsize = rng.integers(0, 2000, size=100_000).astype(np.uint32)
        add(f"long_row_{n_long}", _csr(lrows), _csr(lkept), 50_000, r=8)
        add(f"long_row_{n_long}_sizes", _csr(lrows), _csr(lkept), 99_990, r=64, msg_size=lsize, v=20_000)
        add(f"long_row_{n_long}_rmax", _csr(lrows), _csr(lkept), U32_MAX, r=U32_MAX)

    # ---- the kept rows are the budgets' real output
    n_msgs, n_peers = 300, 12
    mp = rng.integers(0, 8, size=(n_msgs, 3)).astype(np.float64)
    pp = rng.integers(0, 8, size=(n_peers, 3)).astype(np.float64)
    brows = _rows(rng, [40, 300, 0, 41, 299, 5, 40, 300, 0, 41, 257, 5], n_msgs)
    boff, bmsgs = _csr(brows)
    bsize = rng.integers(0, 400, size=n_msgs).astype(np.uint32)
    ko, km, _ = interest.peer_budget_np(boff, bmsgs, mp, pp, k=17)
    add("after_count_budget", (boff, bmsgs), (ko, km), rng.integers(0, n_msgs, size=n_peers), r=3)
    add("after_count_budget_sizes", (boff, bmsgs), (ko, km), U32_MAX, r=5, msg_size=bsize, v=600)
    ko, km, _, _ = interest.peer_budget_bytes_np(boff, bmsgs, mp, bsize, pp, w=3000)
    add("after_byte_budget", (boff, bmsgs), (ko, km), rng.integers(0, n_msgs, size=n_peers), r=4, msg_size=bsize,
        v=900)
    add("after_byte_budget_per_peer", (boff, bmsgs), (ko, km), 150, r=2, extra=rng.integers(0, 9, size=n_peers),
        msg_size=bsize, v=1, extra_bytes=rng.integers(0, 2000, size=n_peers))

    # ---- repeated message indices split between kept and cut
    add("repeats_small", _csr([[5, 5, 5, 7, 7, 9], [], [7, 7, 7], [5, 5, 9, 9, 9, 9, 11]]),
        _csr([[5, 5, 7], [], [7], [5, 9, 9]]), [5, 0, 7, 9], r=2)
    rep = np.sort(rng.integers(0, 20, size=700)).astype(np.uint32)
    for r in (1, 50, 699):
        add(f"repeats_long_r{r}", _csr([rep, rep[:300], rep[100:165]]),
            _csr([_subset(rng, rep, 123), _subset(rng, rep[:300], 290), rep[100:165][:0]]), [7, 19, 3], r=r)
    add("repeats_long_sizes", _csr([rep, rep[:300]]), _csr([_subset(rng, rep, 123), _subset(rng, rep[:300], 10)]),
        [7, U32_MAX], r=200, msg_size=rng.integers(0, 50, size=20), v=900)

    # ---- sizes
    srow = np.arange(0, 60, dtype=np.uint32)
    skept = srow[:10]
    ssize = np.full(60, 10, np.uint32)
    big = ssize.copy()
    big[10] = 5000                                                  # the first cut frame is larger than V
    add("sizes_first_larger_than_v", _csr([srow, srow]), _csr([skept, skept]), [U32_MAX, 30], r=8, msg_size=big, v=100)
    add("sizes_v_zero", _csr([srow, srow]), _csr([skept, skept]), [U32_MAX, 30], r=8, msg_size=ssize, v=0)
    zero = ssize.copy()
    zero[10:20] = 0                                                 # zero-size frames: V = 0 takes them all
    add("sizes_zero_frames_v_zero", _csr([srow, srow]), _csr([skept, skept]), [U32_MAX, 14], r=30, msg_size=zero, v=0)
    add("sizes_zero_frames", _csr([srow, srow]), _csr([skept, skept]), [U32_MAX, 14], r=30, msg_size=zero, v=25)
    huge = np.full(60, U32_MAX, np.uint32)                          # the running sums need u64
    add("sizes_need_u64", _csr([srow, srow]), _csr([skept, skept]), [U32_MAX, 57], r=50, msg_size=huge,
        v=20 * U32_MAX + 5)
    add("sizes_need_u64_per_peer", _csr([srow, srow]), _csr([skept, skept]), [U32_MAX, 57], r=50, msg_size=huge, v=0,
        extra_bytes=[3 * U32_MAX, (1 << 64) - 1])
    add("sizes_no_messages", _csr([srow, srow]), _csr([skept, skept]), 5, r=4, msg_size=ssize[:0], v=7)   # bit 1

    # ---- error bits
    bad = bmsgs.copy()
    bad[rng.choice(len(bad), size=60, replace=False)] = rng.choice([300, 301, U32_MAX, U32_MAX - 1, 1 << 31], size=60)
    bad_rows = [np.sort(bad[boff[p]:boff[p + 1]]) for p in range(n_peers)]
    add("error_message_index", _csr(bad_rows), _csr([_subset(rng, r, 9) for r in bad_rows]), 100, r=6,
        msg_size=bsize, v=1000)
    add("error_message_index_no_sizes", _csr(bad_rows), _csr([_subset(rng, r, 9) for r in bad_rows]), 100, r=6)
    add("error_kept_absent", _csr([[1, 3, 5, 7], [2, 4]]), _csr([[3, 4, 7], [2]]), U32_MAX, r=1)        # 4 is not there
    add("error_kept_too_many", _csr([[1, 3, 3, 7], [2, 4]]), _csr([[3, 3, 3], [2]]), U32_MAX, r=1)      # ck > cf
    add("error_kept_longer", _csr([[1, 3], []]), _csr([[0, 1, 2, 3, 4, 9], [8]]), 1, r=5)

    # ---- degenerate sizes
    add("size_no_peers", (np.zeros(1, np.uint32), bmsgs[:100]), (np.zeros(1, np.uint32), bmsgs[:7]), [], r=3)
    add("size_no_elements", (np.zeros(1001, np.uint32), bmsgs[:0]), (np.zeros(1001, np.uint32), bmsgs[:0]), 7, r=3)
    add("size_no_elements_sizes", (np.zeros(11, np.uint32), bmsgs[:0]), (np.zeros(11, np.uint32), bmsgs[:0]), 7, r=3,
        msg_size=bsize, v=9)
    add("size_nothing", (np.zeros(1, np.uint32), bmsgs[:0]), (np.zeros(1, np.uint32), bmsgs[:0]), [], r=3)
    add("size_kept_longer_array", (boff, bmsgs), (np.zeros(n_peers + 1, np.uint32), bmsgs), 0, r=2)  # rows empty

    # ---- hostile offsets, in either CSR, and rows that do not ascend
    ko, km, _ = interest.peer_budget_np(boff, bmsgs, mp, pp, k=17)
    curs = rng.integers(0, n_msgs, size=n_peers)
    H = dict(r=4, msg_size=bsize, v=700, kind="hostile")
    one = boff.copy()
    one[4] = 10
    sums = np.cumsum(np.concatenate([[0], rng.integers(0, 1 << 31, size=n_peers)]).astype(np.uint64))
    assert int(sums[-1]) > 1 << 32
    wrapped = (sums & np.uint64(U32_MAX)).astype(np.uint32)
    overlapping = [0, 1300, 0, 1300, 0, 1300, 20, 10, 1369, 0, 5, 0, 700]
    for tag, hoff in (("descending", boff[::-1]), ("one_descent", one), ("all_ones", np.full(n_peers + 1, U32_MAX)),
                      ("wrapped", wrapped), ("overlapping", overlapping)):
        add(f"hostile_full_{tag}", (hoff, bmsgs), (ko, km), curs, **H)
        add(f"hostile_kept_{tag}", (boff, bmsgs), (np.minimum(hoff, U32_MAX), km), curs, **H)
    add("hostile_full_past_n_in", (boff, bmsgs[:500]), (ko, km), curs, **H)
    add("hostile_kept_past_n_in", (boff, bmsgs), (ko, km[:90]), curs, **H)
    add("hostile_both_descending", (boff[::-1], bmsgs), (ko[::-1], km), curs, **H)
    shuffled = bmsgs.copy()
    rng.shuffle(shuffled)
    add("hostile_rows_unsorted", (boff, shuffled), (ko, km), curs, **H)
    kshuf = km.copy()
    rng.shuffle(kshuf)
    add("hostile_kept_rows_unsorted", (boff, bmsgs), (ko, kshuf), curs, r=4, kind="hostile")
    add("hostile_rows_unsorted_repeats", _csr([rng.integers(0, 9, size=500), rng.integers(0, 9, size=70)]),
        _csr([rng.integers(0, 9, size=100), rng.integers(0, 12, size=70)]), [4, 8], r=17, kind="hostile")
    return out


def exact_names():
    return sorted(n for n, c in cases().items() if c.kind == "exact")


def hostile_names():
    return sorted(n for n, c in cases().items() if c.kind == "hostile")


def walked_rows(offsets, n):
    """Per row (start, length) of a CSR over n elements by the header's rule."""
    return interest._walk_rows(offsets, n)[0]


def rows_ascend(c):
    """Every walked row of both CSRs ascends: the definition's bytes hold whatever the offsets are."""
    for off, arr in ((c.offsets, c.msgs), (c.koffsets, c.kmsgs)):
        for a, n in walked_rows(off, len(arr)):
            if n > 1 and (np.diff(arr[a:a + n].astype(np.int64)) < 0).any():
                return False
    return True


def shares(c):
    """(R per peer, V per peer) as Python ints."""
    R = c.extra.tolist() if c.extra is not None else [c.r] * c.n_peers
    V = [int(x) for x in c.extra_bytes] if c.extra_bytes is not None else [c.v] * c.n_peers
    return R, V


@functools.lru_cache(maxsize=None)
def want(name):
    """peer_rotate_np of a case, computed once: (out_offsets, out_msgs, out_bytes or None, cursor after,
    counters)."""
    c = cases()[name]
    cursor = c.cursor.copy()
    oo, om, ob, cnt = interest.peer_rotate_np(c.offsets, c.msgs, c.koffsets, c.kmsgs, cursor, r=c.r, extra=c.extra,
                                              msg_size=c.msg_size, v=c.v, extra_bytes=c.extra_bytes)
    for a in (oo, om, ob, cursor):
        if a is not None:
            a.setflags(write=False)
    return oo, om, ob, cursor, cnt


def well_formed(c, oo, om, cursor, counters=None):
    """What include/wq_router.h promises whatever the arrays hold. oo: out_offsets[n_peers + 1], om:
    out_msgs[:n_out], cursor: the cursors after the call."""
    n_in = len(c.msgs)
    assert len(oo) == c.n_peers + 1 and int(oo[0]) == 0
    lens = np.diff(oo.astype(np.int64))
    assert (lens >= 0).all() and int(oo[-1]) == len(om) <= n_in
    rows = walked_rows(c.offsets, n_in)
    for p, (a, n) in enumerate(rows):
        assert lens[p] <= n, p
        full = c.msgs[a:a + n]
        vals, cnt = np.unique(om[oo[p]:oo[p + 1]], return_counts=True)         # a sub-multiset of the full row
        fv, fc = np.unique(full, return_counts=True)
        have = dict(zip(fv.tolist(), fc.tolist()))
        assert all(have.get(v, 0) >= k for v, k in zip(vals.tolist(), cnt.tolist())), p
        assert cursor[p] == c.cursor[p] or int(cursor[p]) in have, p
    if counters is not None:
        assert int(counters["n_out"]) == int(oo[-1]) and int(counters["n_in"]) <= n_in
        assert int(counters["n_out"]) == int(counters["n_kept_in"]) + int(counters["n_chosen"])
        descends = False
        for off, n in ((c.offsets.astype(np.int64), n_in), (c.koffsets.astype(np.int64), len(c.kmsgs))):
            descends |= bool(((off[1:] < off[:-1]) | (off[1:] > n)).any())
        assert (int(counters["error"]) & 1) == int(descends)
        assert int(counters["rows_rotated"]) >= int((cursor != c.cursor).sum())   # a cursor may land where it stood


# ---- the naive restatement --------------------------------------------------------------------

def restated(c, cursor=None):
    """Per row: merge the kept row into the full one (both ascend), rotate the list of cut positions
    so that the first message index above the cursor leads, take R, drop from the end while the bytes
    exceed V and more than one is left. Returns (out_offsets, out_msgs, cursor after)."""
    off, msgs, koff, kmsgs = c.offsets.tolist(), c.msgs.tolist(), c.koffsets.tolist(), c.kmsgs.tolist()
    cursor = (c.cursor if cursor is None else cursor).tolist()
    R, V = shares(c)
    size = c.msg_size.tolist() if c.msg_size is not None else None
    oo, om = [0], []
    for p in range(c.n_peers):
        row, krow = msgs[off[p]:off[p + 1]], kmsgs[koff[p]:koff[p + 1]]
        cut, j = [], 0
        for i, m in enumerate(row):
            while j < len(krow) and krow[j] < m:
                j += 1                                  # a kept element without a partner
            if j < len(krow) and krow[j] == m:
                j += 1
            else:
                cut.append(i)
        lead = sum(1 for i in cut if row[i] <= cursor[p])
        rotated = cut[lead:] + cut[:lead]
        take = rotated[:R[p]]
        if size is not None:
            sz = lambda i: size[row[i]] if row[i] < len(size) else 0
            while len(take) > 1 and sum(sz(i) for i in take) > V[p]:
                take.pop()
        if take:
            cursor[p] = row[take[-1]]
        gone = set(cut) - set(take)
        om += [m for i, m in enumerate(row) if i not in gone]
        oo.append(len(om))
    return np.array(oo, np.uint32), np.array(om, np.uint32), np.array(cursor, np.uint32)


@pytest.mark.parametrize("name", exact_names())
def test_reference_matches_restatement(name):
    c = cases()[name]
    oo, om, ob, cursor, cnt = want(name)
    r_oo, r_om, r_cursor = restated(c)
    assert oo.dtype == np.uint32 and om.dtype == np.uint32 and cursor.dtype == np.uint32
    assert oo.tobytes() == r_oo.tobytes() and om.tobytes() == r_om.tobytes()
    assert cursor.tobytes() == r_cursor.tobytes()
    well_formed(c, oo, om, cursor, cnt)
    assert (ob is None) == (c.msg_size is None)
    if ob is not None:
        size = np.concatenate([c.msg_size.astype(np.uint64), np.zeros(1, np.uint64)])
        at = np.minimum(om.astype(np.int64), len(c.msg_size))
        per_row = [int(sum(int(x) for x in size[at[oo[p]:oo[p + 1]]])) for p in range(c.n_peers)]
        assert [int(x) for x in ob] == per_row and cnt["bytes_out"] == sum(per_row)


@pytest.mark.parametrize("name", hostile_names())
def test_reference_is_well_formed_on_hostile_input(name):
    c = cases()[name]
    oo, om, ob, cursor, cnt = want(name)
    well_formed(c, oo, om, cursor, cnt)
    again = interest.peer_rotate_np(c.offsets, c.msgs, c.koffsets, c.kmsgs, c.cursor.copy(), r=c.r, extra=c.extra,
                                    msg_size=c.msg_size, v=c.v, extra_bytes=c.extra_bytes)
    assert again[0].tobytes() == oo.tobytes() and again[1].tobytes() == om.tobytes() and again[3] == cnt


def test_case_conditions():
    """What the rows are there for, from the reference alone."""
    c = cases()
    lens = np.diff(c["lens_kept_some_r3"].offsets.astype(np.int64)).tolist()
    for edge in (GRANULE, TILE):
        assert {edge - 1, edge, edge + 1} <= set(lens)
    assert {0, 1, 2} <= set(lens)
    assert max(np.diff(c["long_row_5000"].offsets.astype(np.int64))) == 5_000
    assert max(np.diff(c["long_row_70000"].offsets.astype(np.int64))) == 70_000
    # R around T: T - 1 leaves one row element behind, T and T + 1 leave none
    assert want("lens_kept_some_extra_Tm1")[4]["rows_behind"] > 0
    assert want("lens_kept_some_extra_T")[4]["rows_behind"] == 0 and want("lens_kept_some_extra_Tp1")[4]["rows_behind"] == 0
    assert want("lens_kept_some_rmax")[4]["rows_behind"] == 0 and want("lens_kept_some_r0")[4]["n_chosen"] == 0
    assert want("lens_kept_all_rmax")[4]["n_chosen"] == 0 and want("lens_kept_all_rmax")[4]["rows_rotated"] == 0
    full = c["lens_kept_none_rmax"]
    assert want("lens_kept_none_rmax")[1].tobytes() == full.msgs.tobytes()
    assert want("lens_kept_none_r0")[4]["n_out"] == 0
    # the cursor's places: with R = 3 the chosen are the three cut elements after each place
    oo, om, _, cursor, _ = want("cursor_places_r3")
    cc = c["cursor_places_r3"]
    kept = set(cc.kmsgs[:int(cc.koffsets[1])].tolist())
    chosen = [[m for m in om[oo[p]:oo[p + 1]].tolist() if m not in kept] for p in range(cc.n_peers)]
    assert chosen == [[13, 16, 19], [16, 19, 25], [25, 28, 31], [25, 28, 31], [13, 16, 19], [13, 16, 19],
                      [13, 16, 19], [13, 16, 19]]
    assert cursor.tolist() == [19, 25, 31, 31, 19, 19, 19, 19]
    assert want("cursor_places_r30")[4]["rows_behind"] == 0 and want("cursor_places_r29")[4]["rows_behind"] == 8
    # repeats: 5 occurs three times, two are kept, the third is cut and chosen first behind cursor 4 < 5
    oo, om, _, cursor, cnt = want("repeats_small")
    assert om[:int(oo[1])].tolist() == [5, 5, 7, 7, 9] and cnt["error"] == 0
    # sizes
    oo, om, ob, cursor, cnt = want("sizes_first_larger_than_v")
    assert om[:int(oo[1])].tolist() == list(range(10)) + [10] and int(ob[0]) == 100 + 5000     # chosen alone
    assert om[int(oo[1]):].tolist() == list(range(10)) + list(range(31, 39)) and int(ob[1]) == 180
    oo, om, ob, cursor, cnt = want("sizes_v_zero")
    assert cnt["n_chosen"] == 2 and cursor.tolist() == [10, 31]                                # the first only
    oo, om, ob, cursor, cnt = want("sizes_zero_frames_v_zero")
    assert cursor.tolist() == [19, 19] and cnt["n_chosen"] == 10 + 5
    assert want("sizes_need_u64")[4]["bytes_chosen"] == 40 * U32_MAX > 1 << 32
    assert [int(x) for x in want("sizes_need_u64_per_peer")[2]] == [13 * U32_MAX, 60 * U32_MAX]
    assert want("sizes_no_messages")[4]["error"] == 2 and want("sizes_no_messages")[4]["bytes_out"] == 0
    # error bits
    assert want("error_message_index")[4]["error"] == 2 and want("error_message_index_no_sizes")[4]["error"] == 0
    for name in ("error_kept_absent", "error_kept_too_many", "error_kept_longer"):
        assert want(name)[4]["error"] == 4, name
    assert want("error_kept_too_many")[1].tolist() == [1, 3, 3, 2, 4]
    for name in hostile_names():
        bit0 = name.startswith(("hostile_full_", "hostile_kept_", "hostile_both_")) and "unsorted" not in name
        assert (want(name)[4]["error"] & 1) == int(bit0), name
    assert rows_ascend(c["hostile_full_past_n_in"]) and rows_ascend(c["hostile_kept_past_n_in"])
    assert not rows_ascend(c["hostile_rows_unsorted"]) and not rows_ascend(c["hostile_kept_rows_unsorted"])
    # sizes
    for name in ("size_no_peers", "size_no_elements", "size_nothing", "size_no_elements_sizes"):
        assert not want(name)[0].any() and len(want(name)[1]) == 0
    # the budgets' real output is a sub-multiset of the full rows: no bit 2
    for name in ("after_count_budget", "after_byte_budget", "after_count_budget_sizes", "after_byte_budget_per_peer"):
        assert want(name)[4]["error"] == 0 and want(name)[4]["n_chosen"] > 0 and want(name)[4]["rows_behind"] > 0


def _appearances(c, calls):
    """The cut (peer, position) pairs seen in some output of `calls` consecutive calls on one list."""
    cursor = c.cursor.copy()
    seen = [set() for _ in range(c.n_peers)]
    for _ in range(calls):
        oo, om, _, _ = interest.peer_rotate_np(c.offsets, c.msgs, c.koffsets, c.kmsgs, cursor, r=c.r, extra=c.extra,
                                               msg_size=c.msg_size, v=c.v, extra_bytes=c.extra_bytes)
        for p in range(c.n_peers):
            seen[p] |= set(om[oo[p]:oo[p + 1]].tolist())
    return seen


@pytest.mark.parametrize("start", [0, 9, 13, 64, 126, 127, 128, U32_MAX])
@pytest.mark.parametrize("R", [1, 2, 7, 29, 30, 1000])
def test_every_cut_element_arrives_within_ceil_T_over_R_calls(R, start):
    """A fixed list with T cut elements and a count share R >= 1: after ceil(T / R) consecutive calls
    every element of the list has been in some output, for every starting cursor."""
    base = cases()["cursor_places_r3"]
    c = SimpleNamespace(**{**vars(base), "r": R, "cursor": np.full(base.n_peers, start, np.uint32)})
    T = 30
    assert _cut_counts([base.msgs[:40]], [base.kmsgs[:10]]) == [T]
    calls = -(-T // R)
    seen = _appearances(c, calls)
    assert all(s == set(base.msgs[:40].tolist()) for s in seen)
    if calls > 1:                                   # and one call fewer is not enough: the bound is tight
        assert all(s != set(base.msgs[:40].tolist()) for s in _appearances(c, calls - 1))


@pytest.mark.parametrize("start", [0, 13, 127, U32_MAX])
@pytest.mark.parametrize("V", [0, 99, 100, 250, 10_000])
def test_with_a_byte_share_every_cut_element_arrives_within_T_calls(V, start):
    base = cases()["cursor_places_sizes"]
    size = base.msg_size.copy()
    size[[13, 16, 40, 100]] = [0, 5000, 0, 101]
    c = SimpleNamespace(**{**vars(base), "v": V, "msg_size": size, "cursor": np.full(base.n_peers, start, np.uint32)})
    seen = _appearances(c, 30)
    assert all(s == set(base.msgs[:40].tolist()) for s in seen)


def test_rows_with_repeats_arrive_too():
    """With repeats the cursor, a message index, starts behind the whole run of its value: a run that the
    share splits is taken up again a cycle later, and every call passes at least one distinct cut value.
    So with R = 1 every message index of a row has been sent after as many calls as it has distinct
    values."""
    c = cases()["repeats_long_r1"]
    seen = _appearances(c, 20)
    for (a, n), s in zip(walked_rows(c.offsets, len(c.msgs)), seen):
        assert s == set(c.msgs[a:a + n].tolist())


def test_arguments():
    off, msgs = np.array([0, 4, 4, 6], np.uint32), np.array([0, 1, 2, 5, 0, 2], np.uint32)
    koff, kmsgs = np.array([0, 1, 1, 1], np.uint32), np.array([1], np.uint32)
    cursor = np.array([U32_MAX, 3, 0], np.uint32)
    oo, om, ob, cnt = interest.peer_rotate_np(off, msgs, koff, kmsgs, cursor, r=2)
    assert oo.tolist() == [0, 3, 3, 5] and om.tolist() == [0, 1, 2, 0, 2] and ob is None
    assert cursor.tolist() == [2, 3, 0]
    assert cnt == dict(n_in=6, n_kept_in=1, n_chosen=4, n_out=5, bytes_chosen=0, bytes_out=0, rows_rotated=2,
                       rows_behind=1, error=0)
    oo, om, ob, cnt = interest.peer_rotate_np(off, msgs, koff, kmsgs, cursor, r=2)      # the next tick
    assert om.tolist() == [0, 1, 5, 0, 2] and cursor.tolist() == [0, 3, 0]
    oo, om, ob, cnt = interest.peer_rotate_np(off, msgs, koff, kmsgs, cursor, extra=[9, 9, 0],
                                              msg_size=[7, 7, 7, 7, 7, 7], v=14)
    assert om.tolist() == [1, 2, 5] and ob.tolist() == [21, 0, 0] and cnt["bytes_chosen"] == 14
    with pytest.raises(ValueError):
        interest.peer_rotate_np(off, msgs, koff, kmsgs, cursor)
    with pytest.raises(ValueError):
        interest.peer_rotate_np(off, msgs, koff, kmsgs, cursor, r=1, msg_size=[1] * 6)
    with pytest.raises(ValueError):
        interest.peer_rotate_np(off, msgs, koff, kmsgs, cursor.astype(np.int64), r=1)
    with pytest.raises(ValueError):
        interest.peer_rotate_np(off, msgs, koff[:-1], kmsgs, cursor, r=1)
