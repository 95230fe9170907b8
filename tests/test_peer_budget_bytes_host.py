"""The host definition of the byte budgets (worldql_server_amd/interest.py peer_budget_bytes_np) against
an independent restatement: a plain Python sort of (key bits, position) tuples and a running sum.
`cases()` is shared with the C++ mirror (tests/test_peer_budget_bytes_cpp_mirror.py) and the GPU
instance (tests/test_gpu_peer_budget_bytes.py). No GPU needed.

A case is the argument list of one wq_peer_budget_bytes_device call: the count budget's case
(tests/test_peer_budget_host.py) with msg_size[n_msgs], w and the per-peer byte budget (u64, or None)
in place of k and budget. The expected bytes of either kind, "exact" or "hostile", are
peer_budget_bytes_np's (`want`)."""
import functools
import struct
from types import SimpleNamespace

import numpy as np
import pytest

from worldql_server_amd import interest

import test_peer_budget_host as count
from test_peer_budget_host import CHUNK, DIGIT_BITS, INF_BITS, SHORT, TILE, _csr, _grid_world, _rows, py_keys

U32_MAX = 0xFFFFFFFF
U64_MAX = 0xFFFFFFFFFFFFFFFF


def _sizes(rng, n, zeros=0.0):
    """The bench's mix: most frames 100 - 200 B, a few percent 2 - 16 KB; `zeros`: the share of 0 B."""
    s = rng.integers(100, 201, size=n)
    big = rng.random(n) < 0.04
    s[big] = rng.integers(2048, 16385, size=int(big.sum()))
    s[rng.random(n) < zeros] = 0
    return s.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> SimpleNamespace(offsets, msgs, n_peers, msg_pos, msg_size, peer_pos, w, budget, kind);
    built once, never modified (the arrays are read-only)."""
    rng = np.random.default_rng(77)
    out = {}

    def add(name, offsets, msgs, msg_pos, peer_pos, msg_size, w=0, budget=None, kind="exact"):
        offsets, msgs = np.ascontiguousarray(offsets, np.uint32), np.ascontiguousarray(msgs, np.uint32)
        msg_pos = np.ascontiguousarray(msg_pos, np.float64).reshape(-1, 3)
        peer_pos = np.ascontiguousarray(peer_pos, np.float64).reshape(-1, 3)
        msg_size = np.ascontiguousarray(msg_size, np.uint32)
        assert len(msg_size) == len(msg_pos)
        arrays = [offsets, msgs, msg_pos, peer_pos, msg_size]
        if budget is not None:
            budget = np.array([int(b) for b in budget], dtype=np.uint64)
            assert len(budget) == len(offsets) - 1
            arrays.append(budget)
        for a in arrays:
            a.setflags(write=False)
        assert name not in out
        out[name] = SimpleNamespace(offsets=offsets, msgs=msgs, n_peers=len(offsets) - 1, msg_pos=msg_pos,
                                    msg_size=msg_size, peer_pos=peer_pos, w=int(w), budget=budget, kind=kind)

    def totals(offsets, msgs, msg_size):
        return [int(msg_size[msgs[a:b]].astype(np.uint64).sum()) for a, b in zip(offsets[:-1], offsets[1:])]

    # ---- the count budget's shapes with sizes: rows of 63 .. 2 CHUNK + 37 elements, 255 / 256 / 257 among
    # them, rows that start mid-tile and pass tile and block boundaries
    cc = count.cases()
    c = cc["len_edges_k64"]
    sz = _sizes(rng, len(c.msg_pos), zeros=0.1)
    for w in (3000, 60000):
        add(f"len_edges_w{w}", c.offsets, c.msgs, c.msg_pos, c.peer_pos, sz, w=w)
    # a long row that starts mid-tile (ordinal 100) and spans tile boundaries and the block boundary at
    # CHUNK; two long rows inside the second block; short rows around them
    lens = [100, CHUNK + 252, 300, 300, 7, 0, 255]
    mp, pp = _grid_world(rng, 3000, len(lens), side=14)
    off, msgs = _csr(_rows(rng, lens, 3000))
    sz = _sizes(rng, 3000, zeros=0.05)
    for w in (20000, 150):
        add(f"mid_tile_w{w}", off, msgs, mp, pp, sz, w=w)

    # ---- W around a row's total: total - 1, total, total + 1 on the same row, at the short / long boundary
    lens = [255, 256, 257, 700]
    mp, _ = _grid_world(rng, 900, 1, side=9)
    sz = _sizes(rng, 900, zeros=0.1)
    base = _rows(rng, lens, 900)
    rows3 = [r for r in base for _ in range(3)]
    off, msgs = _csr(rows3)
    tot = totals(off, msgs, sz)
    add("w_around_total", off, msgs, mp, np.full((len(rows3), 3), 2.0), sz,
        budget=[t + d for t, d in zip(tot, [-1, 0, 1] * len(lens))])

    # ---- zero sizes. Messages on a line seen from the origin: message i at x = 1 + i / 8 (d2 ascends with i)
    def line(n_msgs):
        mp = np.zeros((n_msgs, 3))
        mp[:, 0] = 1.0 + np.arange(n_msgs) / 8.0
        return mp

    mp = line(40)
    sz = rng.integers(100, 200, size=40).astype(np.uint32)
    sz[[0, 1]] = 0                     # the two nearest messages are empty frames
    with_lead = [rng.integers(0, 40, size=n) for n in (90, 600)]
    without = [rng.integers(2, 40, size=n) for n in (90, 600)]
    off, msgs = _csr(with_lead + without)
    assert all((r < 2).any() for r in with_lead)
    add("w_zero", off, msgs, mp, np.zeros((4, 3)), sz, w=0)
    # W one below the nearest element's size: rows without a zero-size head lose everything
    nearest = [int(sz[r.min()]) for r in without]
    add("w_below_nearest", off, msgs, mp, np.zeros((4, 3)), sz, budget=[nearest[0] - 1, nearest[1] - 1] * 2)
    # zero-size elements before, at and after the cut: 8 distinct keys, a third of the messages empty,
    # several messages per key so the threshold key's ties differ in size
    mp = line(8).repeat(4, axis=0)     # messages 4 i .. 4 i + 3 share key i
    sz = np.tile(np.array([0, 120, 0, 3000], np.uint32), 8)
    sz[5] = 77
    rows_z = [rng.integers(0, 32, size=n) for n in (120, 700, 2500)]
    off, msgs = _csr(rows_z)
    tot = totals(off, msgs, sz)
    add("zero_sizes_at_cut", off, msgs, mp, np.zeros((3, 3)), sz, budget=[t // 2 for t in tot])
    add("zero_sizes_at_cut_small_w", off, msgs, mp, np.zeros((3, 3)), sz, w=2000)
    # a whole bin of zero-size elements below the picked bin: d2 = 2^(16 j) differ in the top digit, and the
    # nearest message (a bin of its own in the first pass) is empty
    mp = np.zeros((11, 3))
    mp[:, 0] = [2.0 ** (8 * j) for j in range(-5, 6)]
    sz = np.full(11, 150, np.uint32)
    sz[0] = 0
    rows_b = [rng.integers(0, 11, size=n) for n in (60, 700)]
    off, msgs = _csr(rows_b)
    tot = totals(off, msgs, sz)
    add("zero_bin_below_pick", off, msgs, mp, np.zeros((2, 3)), sz, budget=[t // 2 for t in tot])

    # ---- ties
    # all keys equal: the ties' bytes alone decide
    mp = np.zeros((30, 3)) + 3.0
    sz = _sizes(rng, 30, zeros=0.2)
    rows_t = [rng.integers(0, 30, size=n) for n in (100, 600, CHUNK + 100)]
    off, msgs = _csr(rows_t)
    tot = totals(off, msgs, sz)
    add("ties_all_equal", off, msgs, mp, np.zeros((3, 3)), sz, budget=[t // 2 for t in tot])
    add("ties_all_equal_w1", off, msgs, mp, np.zeros((3, 3)), sz, w=1)
    # keys that differ only in the last of the eight digits: d2 = 1 + i^2 2^-52
    mp = np.array([[1.0, i * 2.0 ** -26, 0.0] for i in range(16)])
    sz = _sizes(rng, 16)
    rows_d = [rng.integers(0, 16, size=n) for n in (40, 700)]
    off, msgs = _csr(rows_d)
    tot = totals(off, msgs, sz)
    add("keys_bottom_digit", off, msgs, mp, np.zeros((2, 3)), sz, budget=[t // 2 for t in tot])

    # ---- sizes of 2^32 - 1: a row's total and a single histogram bin pass 2^32
    mp = line(6)
    sz = np.array([U32_MAX, U32_MAX, 5, U32_MAX, 0, U32_MAX], np.uint32)
    rows_h = [rng.integers(0, 6, size=n) for n in (50, 400, 900)]
    off, msgs = _csr(rows_h)
    tot = totals(off, msgs, sz)
    add("huge_sizes", off, msgs, mp, np.zeros((3, 3)), sz, budget=[tot[0] // 2, tot[1] // 2, tot[2] - 1])
    add("huge_sizes_w", off, msgs, mp, np.zeros((3, 3)), sz, w=10 * U32_MAX + 4)

    # ---- +inf keys: no position, m >= n_msgs (size 0, error bit 1), every message missing
    for name in ("missing_peer_positions", "missing_all_peer_positions", "missing_message_index", "missing_all_messages",
                 "keys_nan_position_700"):
        c = cc[name]
        add(name, c.offsets, c.msgs, c.msg_pos, c.peer_pos, _sizes(rng, len(c.msg_pos), zeros=0.1), w=2500)

    # ---- per-peer budgets mixing 0, small, exact fit and 2^64 - 1
    c = cc["budget_array"]
    sz = _sizes(rng, len(c.msg_pos), zeros=0.1)
    tot = totals(c.offsets, c.msgs, sz)
    add("budget_array", c.offsets, c.msgs, c.msg_pos, c.peer_pos, sz, w=5,
        budget=[0, 300, U64_MAX, U64_MAX, 0, 100, tot[6], tot[7], 7, tot[9] - 1, tot[10] + 1, 1 << 40])
    add("budget_all_zero", c.offsets, c.msgs, c.msg_pos, c.peer_pos, sz, w=9, budget=[0] * 12)
    add("budget_all_max", c.offsets, c.msgs, c.msg_pos, c.peer_pos, sz, w=0, budget=[U64_MAX] * 12)

    # ---- degenerate sizes
    for name in ("size_no_peers", "size_no_elements", "size_nothing"):
        c = cc[name]
        add(name, c.offsets, c.msgs, c.msg_pos, c.peer_pos, _sizes(rng, len(c.msg_pos)), w=1000)

    # ---- the hostile offsets of the count budget, with sizes
    for name in count.hostile_names():
        c = cc[name]
        add(name, c.offsets, c.msgs, c.msg_pos, c.peer_pos, _sizes(rng, len(c.msg_pos), zeros=0.1),
            w=40000 if name == "hostile_overlapping" else 2500, kind="hostile")
    return out


def exact_names():
    return sorted(n for n, c in cases().items() if c.kind == "exact")


def hostile_names():
    return sorted(n for n, c in cases().items() if c.kind == "hostile")


def budget_of(c):
    return [int(b) for b in c.budget] if c.budget is not None else [c.w] * c.n_peers


@functools.lru_cache(maxsize=None)
def want(name):
    """peer_budget_bytes_np of a case, computed once: (out_offsets, out_msgs, out_bytes, counters)."""
    c = cases()[name]
    oo, om, ob, cnt = interest.peer_budget_bytes_np(c.offsets, c.msgs, c.msg_pos, c.msg_size, c.peer_pos, w=c.w,
                                                    budget=c.budget)
    for a in (oo, om, ob):
        a.setflags(write=False)
    return oo, om, ob, cnt


def clamped_rows(c):
    n_in, off = len(c.msgs), c.offsets.astype(np.int64)
    a = np.minimum(off[:-1], n_in)
    return a, np.maximum(np.minimum(off[1:], n_in) - a, 0)


def well_formed(c, oo, om, ob, counters=None):
    """What include/wq_router.h promises whatever the offsets hold. oo: out_offsets[n_peers + 1], om: the
    kept elements out_msgs[:n_kept], ob: out_bytes[n_peers] (or None), counters: a mapping."""
    n_in = len(c.msgs)
    assert len(oo) == c.n_peers + 1 and int(oo[0]) == 0
    lens = np.diff(oo.astype(np.int64))
    assert (lens >= 0).all() and int(oo[-1]) == len(om) <= n_in
    a, clamped = clamped_rows(c)
    assert (lens <= clamped).all()
    size_of = lambda m: int(c.msg_size[m]) if m < len(c.msg_pos) else 0
    W = budget_of(c)
    for p in range(c.n_peers):
        kept = om[oo[p]:oo[p + 1]].tolist()
        it = iter(c.msgs[a[p]:a[p] + clamped[p]].tolist())
        assert all(any(m == x for x in it) for m in kept), p     # a subsequence of its input row
        row_bytes = sum(size_of(m) for m in kept)
        assert row_bytes <= W[p], p
        if ob is not None:
            assert int(ob[p]) == row_bytes, p
    if counters is not None:
        assert int(counters["n_kept"]) == int(oo[-1]) and int(counters["n_in"]) <= n_in
        assert int(counters["bytes_kept"]) == sum(size_of(m) for m in om.tolist()) <= int(counters["bytes_in"])
        off = c.offsets.astype(np.int64)
        descends = bool(((off[1:] < off[:-1]) | (off[1:] > n_in)).any())
        assert (int(counters["error"]) & 1) == int(descends)
        if c.kind == "exact":
            assert int(counters["n_in"]) == int(clamped.sum())
            assert int(counters["bytes_in"]) == sum(size_of(m) for p in range(c.n_peers)
                                                    for m in c.msgs[a[p]:a[p] + clamped[p]].tolist())


# ---- the independent restatement ------------------------------------------------------------

def key_bits(d2):
    return struct.unpack("<Q", struct.pack("<d", d2))[0]


def ordered(c, p):
    """Row p of an exact case: (its messages, [(key bits, position)] sorted, the sizes by position)."""
    off, n_in = c.offsets.tolist(), len(c.msgs)
    row = c.msgs[min(off[p], n_in):min(off[p + 1], n_in)].tolist()
    order = sorted((key_bits(d2), i) for d2, i in py_keys(c, p, row))
    sizes = [int(c.msg_size[m]) if m < len(c.msg_pos) else 0 for m in row]
    return row, order, sizes


def kept_positions(c, p, W, B=None):
    """The positions of row p with running bytes <= W (and rank < B), ascending."""
    row, order, sizes = ordered(c, p)
    keep, running = [], 0
    for rank, (_, i) in enumerate(order):
        running += sizes[i]
        if running <= W and (B is None or rank < B):
            keep.append(i)
    return row, sorted(keep), sizes


def restated(c, budgets=None, B=None):
    budgets = budget_of(c) if budgets is None else budgets
    oo, om, ob = [0], [], []
    for p in range(c.n_peers):
        row, keep, sizes = kept_positions(c, p, budgets[p], B)
        om += [row[i] for i in keep]
        oo.append(len(om))
        ob.append(sum(sizes[i] for i in keep))
    return np.array(oo, np.uint32), np.array(om, np.uint32), np.array(ob, np.uint64)


@pytest.mark.parametrize("name", exact_names())
def test_reference_matches_restatement(name):
    c = cases()[name]
    oo, om, ob, cnt = want(name)
    r_oo, r_om, r_ob = restated(c)
    assert oo.dtype == np.uint32 and om.dtype == np.uint32 and ob.dtype == np.uint64
    assert oo.tobytes() == r_oo.tobytes() and om.tobytes() == r_om.tobytes() and ob.tobytes() == r_ob.tobytes()
    assert cnt["bytes_kept"] == sum(int(v) for v in r_ob)
    a, clamped = clamped_rows(c)
    cut = sum(int(oo[p + 1]) - int(oo[p]) < int(clamped[p]) for p in range(c.n_peers))
    assert cnt["rows_cut"] == cut
    well_formed(c, oo, om, ob, cnt)


@pytest.mark.parametrize("name", hostile_names())
def test_reference_is_well_formed_on_hostile_offsets(name):
    c = cases()[name]
    oo, om, ob, cnt = want(name)
    well_formed(c, oo, om, ob, cnt)
    assert cnt["error"] & 1


PROPERTY_CASES = [n for n in exact_names() if not n.startswith("len_edges")] + ["len_edges_w3000"]


@pytest.mark.parametrize("name", PROPERTY_CASES)
def test_prefix_monotone_and_bounded(name):
    """The kept set is a prefix of the (key, position) order; it grows with W; a row's kept bytes are
    <= W_p and out_bytes sums to bytes_kept; a row under its total passes through unchanged."""
    c = cases()[name]
    rows = [ordered(c, p) for p in range(c.n_peers)]
    before = [0] * c.n_peers
    for W in sorted({0, 1, 150, 2999, 3000, 60000, U32_MAX, c.w, U64_MAX}):
        oo, om, ob, cnt = interest.peer_budget_bytes_np(c.offsets, c.msgs, c.msg_pos, c.msg_size, c.peer_pos, w=W)
        assert int(ob.astype(object).sum()) == cnt["bytes_kept"]
        for p, (row, order, sizes) in enumerate(rows):
            n = int(oo[p + 1]) - int(oo[p])
            prefix = sorted(i for _, i in order[:n])
            assert om[int(oo[p]):int(oo[p + 1])].tolist() == [row[i] for i in prefix], (p, W)
            assert int(ob[p]) == sum(sizes[i] for i in prefix) <= W
            assert n >= before[p]
            before[p] = n
            if sum(sizes) <= W:
                assert n == len(row)
            elif n < len(row):      # the next element in order does not fit
                assert int(ob[p]) + sizes[order[n][1]] > W
    assert om.tobytes() == c.msgs[:int(c.offsets[-1])].tobytes() and oo.tobytes() == c.offsets.tobytes()   # W = 2^64 - 1
    assert cnt["rows_cut"] == 0 and cnt["bytes_kept"] == cnt["bytes_in"]


COMPOSITION = [("len_edges_w3000", 64, 12000), ("len_edges_w3000", 257, 50000), ("mid_tile_w20000", 200, 50000),
               ("zero_sizes_at_cut", 100, 90000), ("ties_all_equal", 300, 60000), ("huge_sizes", 30, 20 * U32_MAX),
               ("missing_message_index", 17, 2500), ("budget_array", 40, 6000)]


@pytest.mark.parametrize("name,B,W", COMPOSITION)
def test_composition_with_the_count_budget(name, B, W):
    """The count budget first, the byte budget on its output: exactly "rank < B and running bytes <= W"."""
    c = cases()[name]
    o1, m1, _ = interest.peer_budget_np(c.offsets, c.msgs, c.msg_pos, c.peer_pos, k=B)
    oo, om, ob, cnt = interest.peer_budget_bytes_np(o1, m1, c.msg_pos, c.msg_size, c.peer_pos, w=W)
    r_oo, r_om, r_ob = restated(c, [W] * c.n_peers, B)
    assert oo.tobytes() == r_oo.tobytes() and om.tobytes() == r_om.tobytes() and ob.tobytes() == r_ob.tobytes()
    only_w = restated(c, [W] * c.n_peers)
    assert 0 < len(r_om) < len(m1) < len(c.msgs)             # the count cap cuts, the byte cap cuts further
    assert len(r_om) <= len(only_w[1])
    if (name, B) in (("len_edges_w3000", 64), ("zero_sizes_at_cut", 100), ("budget_array", 40)):
        assert len(r_om) < len(only_w[1])                    # and in some row the count cap is the tighter one


# ---- what the cases are there for ----------------------------------------------------------

def _analysis(name):
    """Per row of an exact case: dict(n, kept, W, total, order, sizes, thr) with thr the key bits of the
    first dropped element in order (None when the row is not cut)."""
    c = cases()[name]
    oo = want(name)[0]
    W = budget_of(c)
    rows = []
    for p in range(c.n_peers):
        row, order, sizes = ordered(c, p)
        kept = int(oo[p + 1]) - int(oo[p])
        rows.append(dict(n=len(row), kept=kept, W=W[p], total=sum(sizes), order=order, sizes=sizes,
                         thr=order[kept][0] if kept < len(row) else None, start=int(c.offsets[p])))
    return rows


def _all_rows():
    return [(name, r) for name in exact_names() for r in _analysis(name)]


def test_case_conditions():
    """Every condition the case list exists for is met by some case, from the definition alone."""
    rows = _all_rows()
    cut = [(n, r) for n, r in rows if r["thr"] is not None]
    long_cut = [(n, r) for n, r in cut if r["n"] > SHORT]
    short_cut = [(n, r) for n, r in cut if r["n"] <= SHORT]
    assert long_cut and short_cut
    # rows of 255, 256 and 257 elements are cut, among other rows
    assert {255, 256, 257} <= {r["n"] for _, r in cut}
    assert TILE == SHORT
    # a long cut row that starts mid-tile and spans a tile boundary and the block boundary at CHUNK
    assert any(r["start"] % TILE and r["start"] < CHUNK < r["start"] + r["n"] for _, r in long_cut)
    # two long cut rows inside one block of a histogram pass
    by_case = {}
    for n, r in long_cut:
        by_case.setdefault(n, []).append(r)
    assert any(a is not b and a["start"] // CHUNK == b["start"] // CHUNK == (a["start"] + a["n"] - 1) // CHUNK
               == (b["start"] + b["n"] - 1) // CHUNK for rs in by_case.values() for a in rs for b in rs)
    # W = total - 1, total, total + 1, on short and on long rows
    for pick in (lambda r: r["n"] <= SHORT, lambda r: r["n"] > SHORT):
        assert {-1, 0, 1} <= {r["W"] - r["total"] for _, r in rows if pick(r) and r["total"] > 0}
    # W = 0 with and without leading zero-size elements; W just below the nearest element's size
    zero_w = [r for _, r in cut if r["W"] == 0]
    assert any(r["kept"] > 0 for r in zero_w) and any(r["kept"] == 0 for r in zero_w)
    assert any(r["kept"] > 0 and r["n"] > SHORT for r in zero_w)
    assert any(r["kept"] == 0 and r["W"] == r["sizes"][r["order"][0][1]] - 1 and r["W"] > 0 and r["n"] > SHORT
               for _, r in cut)
    # zero-size elements before, at and after the cut of one long row
    def zero_around(r):
        k, o, s = r["kept"], r["order"], r["sizes"]
        return (any(s[i] == 0 for _, i in o[:k]) and any(s[i] == 0 and b == r["thr"] for b, i in o)
                and any(s[i] == 0 and b > r["thr"] for b, i in o[k:]))
    assert any(zero_around(r) for _, r in long_cut)
    # a whole top-digit bin of zero-size elements below the picked bin
    def zero_bin(r):
        top = lambda b: b >> (64 - DIGIT_BITS)
        lower = {top(b) for b, _ in r["order"] if top(b) < top(r["thr"])}
        return any(all(r["sizes"][i] == 0 for b, i in r["order"] if top(b) == d) for d in lower)
    assert any(zero_bin(r) for _, r in long_cut)
    # all keys equal; threshold ties of differing sizes, a strict non-empty subset of them kept
    assert any(len({b for b, _ in r["order"]}) == 1 for _, r in long_cut)
    def ties_split(r):
        ties = [(i, r["sizes"][i]) for b, i in r["order"] if b == r["thr"]]
        kept_ties = sum(1 for rank, (b, i) in enumerate(r["order"]) if b == r["thr"] and rank < r["kept"])
        return 0 < kept_ties < len(ties) and len({s for _, s in ties}) > 1
    assert any(ties_split(r) for _, r in long_cut) and any(ties_split(r) for _, r in short_cut)
    # sizes of 2^32 - 1: a row's total and one bin of the first pass exceed 2^32
    assert any(r["total"] > 1 << 32 and U32_MAX in r["sizes"] for _, r in long_cut)
    def big_bin(r):
        bins = {}
        for b, i in r["order"]:
            bins[b >> (64 - DIGIT_BITS)] = bins.get(b >> (64 - DIGIT_BITS), 0) + r["sizes"][i]
        return max(bins.values()) > 1 << 32
    assert any(big_bin(r) for _, r in long_cut)
    # keys that differ only in the last digit
    assert any(len({b for b, _ in r["order"]}) > 1 and len({b >> DIGIT_BITS for b, _ in r["order"]}) == 1
               for _, r in long_cut)
    # +inf keys kept and dropped; a missing message has size 0 and sets error bit 1
    assert any(r["thr"] == INF_BITS and r["order"][0][0] == INF_BITS and r["kept"] > 0 for _, r in long_cut)
    assert want("missing_message_index")[3]["error"] == 2 and want("missing_all_messages")[3]["error"] == 2
    assert want("missing_all_messages")[3]["bytes_in"] == 0 and want("missing_all_messages")[3]["rows_cut"] == 0
    assert want("missing_peer_positions")[3]["error"] == 0
    # per-peer budgets: 0, small, exact fit and 2^64 - 1 in one call
    b = _analysis("budget_array")
    assert any(r["W"] == 0 for r in b) and any(r["W"] == U64_MAX for r in b)
    assert any(r["W"] == r["total"] > 0 and r["n"] > SHORT for r in b) and any(0 < r["W"] < 1000 and r["thr"] for r in b)
    # the hostile offsets descend, wrap and pass n_in; the overlapping rows reach the n_in limit
    assert len(hostile_names()) == len(count.hostile_names()) >= 6
    assert want("hostile_overlapping")[3]["n_in"] == len(cases()["hostile_overlapping"].msgs)
    assert all(want(n)[3]["rows_cut"] > 0 for n in hostile_names() if want(n)[3]["n_in"])
    # small: a few thousand elements per case
    assert max(len(c.msgs) for c in cases().values()) < 14000


def test_frame_sizes():
    assert interest.frame_sizes(np.array([0, 130, 130, 5000], np.uint64)).tolist() == [130, 0, 4870]
    assert interest.frame_sizes(np.array([7], np.uint64)).dtype == np.uint32
    assert interest.frame_sizes(np.array([0, U32_MAX], np.uint64)).tolist() == [U32_MAX]
    with pytest.raises(ValueError):
        interest.frame_sizes(np.array([5, 5 + (1 << 32)], np.uint64))


def test_arguments():
    off, msgs = np.array([0, 3, 3, 5], np.uint32), np.array([0, 1, 2, 2, 0], np.uint32)
    mp = np.array([[3.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    sz = np.array([10, 20, 30], np.uint32)
    pp = np.zeros((3, 3))
    oo, om, ob, cnt = interest.peer_budget_bytes_np(off, msgs, mp, sz, pp, w=50)
    assert oo.tolist() == [0, 2, 2, 4] and om.tolist() == [1, 2, 2, 0] and ob.tolist() == [50, 0, 40]
    assert cnt == dict(n_in=5, n_kept=4, bytes_in=100, bytes_kept=90, rows_cut=1, error=0)
    oo, om, ob, cnt = interest.peer_budget_bytes_np(off, msgs, mp, sz, pp, budget=[19, 0, U64_MAX])
    assert oo.tolist() == [0, 0, 0, 2] and om.tolist() == [2, 0] and cnt["rows_cut"] == 1
    with pytest.raises(ValueError):
        interest.peer_budget_bytes_np(off, msgs, mp, sz, pp)
    with pytest.raises(ValueError):
        interest.peer_budget_bytes_np(off, msgs, mp, sz[:2], pp, w=1)
