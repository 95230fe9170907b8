"""The host definition of the send budgets (worldql_server_amd/interest.py peer_budget_np) against an
independent restatement with sorted() over (d2, position) tuples of Python floats. `cases()` is
shared with the C++ mirror (tests/test_peer_budget_cpp_mirror.py) and the GPU instance
(tests/test_gpu_peer_budget.py). No GPU needed.

A case is the argument list of one wq_peer_budget_device call: offsets[n_peers + 1], msgs[n_in],
msg_pos[n_msgs, 3], peer_pos[n_peer_pos, 3], k and the per-peer budget (or None), and its kind:
"exact" (ascending offsets) or "hostile" (offsets that descend, wrap or pass n_in: `well_formed`
states what include/wq_router.h promises then). The expected bytes of either kind are
peer_budget_np's (`want`)."""
import functools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from worldql_server_amd import interest

U32_MAX = 0xFFFFFFFF
# csrc/budget_ops.hpp / wq_budget.hip (the C++ mirror checks all of them against the shim's exports):
SHORT = 256        # kBudShort: rows up to this are ranked by counting, longer ones selected by radix
DIGIT_BITS = 8     # kBudDigitBits
TILE = 256         # kBudTile: a histogram pass counts a tile of this many ordinals of one row in LDS
CHUNK = 8 * TILE   # kBudTiles * kBudTile: ordinals per block of a histogram pass
INF_BITS = 0x7FF0000000000000


def _csr(rows):
    offsets = np.zeros(len(rows) + 1, dtype=np.uint32)
    if rows:
        np.cumsum([len(r) for r in rows], out=offsets[1:])
    msgs = np.concatenate([np.asarray(r, dtype=np.uint32) for r in rows]) if rows else np.zeros(0, np.uint32)
    return offsets, msgs.astype(np.uint32)


def _grid_world(rng, n_msgs, n_peers, side=4):
    """Positions on a small integer grid: many elements of a row have equal d2."""
    return (rng.integers(0, side, size=(n_msgs, 3)).astype(np.float64),
            rng.integers(0, side, size=(n_peers, 3)).astype(np.float64))


def _rows(rng, lengths, n_msgs):
    """Ascending message indices per row, as wq_peer_major_device writes them (repeats when the row
    is longer than the message count)."""
    return [np.sort(rng.integers(0, n_msgs, size=n)) if n > n_msgs else np.sort(rng.choice(n_msgs, size=n, replace=False))
            for n in lengths]


def _line_case(rng, xs, n, peers=1):
    """One row per peer of n elements drawn from messages at (x, 0, 0), x in xs, seen from the origin:
    d2 = x * x. Returns (offsets, msgs, msg_pos, peer_pos)."""
    xs = np.asarray(xs, dtype=np.float64)
    mpos = np.zeros((len(xs), 3))
    mpos[:, 0] = xs
    rows = [rng.integers(0, len(xs), size=n) for _ in range(peers)]
    return (*_csr(rows), mpos, np.zeros((peers, 3)))


# ---- FMA contraction: emulated exactly, numpy (which never contracts) is the arbiter --------------

def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def d2_contracted(dx, dy, dz):
    """What (dx*dx + dy*dy) + dz*dz gives when a compiler contracts it: fma(dz, dz, fma(dx, dx, dy*dy))."""
    return _fma(dz, dz, _fma(dx, dx, dy * dy))


def _fma_np(a, b, c):
    """fma(a, b, c) from error-free transformations (the search's filter; hits are confirmed exactly)."""
    def split(x):
        t = 134217729.0 * x
        hi = t - (t - x)
        return hi, x - hi
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


@functools.lru_cache(maxsize=None)
def fma_pair():
    """Two points (3,) seen from the origin: by numpy's d2 a is one ulp nearer than b; by the contracted
    d2 the two are equal, so b, which stands first in the row, wins. a has full-width coordinates and
    a contracted d2 one ulp above numpy's; b = (x, 0, 0) with x * x exactly numpy's d2 of a plus one
    ulp (nothing to contract there). Found by search, confirmed with exact rational arithmetic."""
    rng = np.random.default_rng(91)
    for _ in range(20):
        pts = 0.8 + rng.random((50000, 3)) * 0.3
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        plain = (x * x + y * y) + z * z
        fused = _fma_np(z, z, _fma_np(x, x, y * y))
        target = np.nextafter(plain, np.inf)
        for i in np.flatnonzero((fused == target) & (plain >= 2.0) & (target < 4.0)):
            r = np.sqrt(target[i])
            for bx in (np.nextafter(r, 0.0), r, np.nextafter(r, np.inf)):
                a, b = tuple(float(v) for v in pts[i]), (float(bx), 0.0, 0.0)
                if bx * bx == target[i] and d2_contracted(*a) == d2_contracted(*b) == float(target[i]):
                    return np.array(a), np.array(b)
    return None


@functools.lru_cache(maxsize=None)
def cases():
    """name -> SimpleNamespace(offsets, msgs, n_peers, msg_pos, peer_pos, k, budget, kind); built once,
    never modified (the arrays are read-only)."""
    rng = np.random.default_rng(44)
    out = {}

    def add(name, offsets, msgs, msg_pos, peer_pos, k=0, budget=None, kind="exact"):
        offsets, msgs = np.ascontiguousarray(offsets, np.uint32), np.ascontiguousarray(msgs, np.uint32)
        msg_pos = np.ascontiguousarray(msg_pos, np.float64).reshape(-1, 3)
        peer_pos = np.ascontiguousarray(peer_pos, np.float64).reshape(-1, 3)
        arrays = [offsets, msgs, msg_pos, peer_pos]
        if budget is not None:
            budget = np.ascontiguousarray(budget, np.uint32)
            assert len(budget) == len(offsets) - 1
            arrays.append(budget)
        for a in arrays:
            a.setflags(write=False)
        assert name not in out
        out[name] = SimpleNamespace(offsets=offsets, msgs=msgs, n_peers=len(offsets) - 1, msg_pos=msg_pos,
                                    peer_pos=peer_pos, k=int(k), budget=budget, kind=kind)

    # ---- budgets and row lengths: B - 1, B, B + 1 around every B, among other rows
    for B in (0, 1, 2, 32):
        lens = [n for n in (B - 1, B, B + 1) if n >= 0] + [0, 5, 70, B + 1, B]
        mp, pp = _grid_world(rng, 200, len(lens))
        add(f"len_around_{B}", *_csr(_rows(rng, lens, 200)), mp, pp, k=B)
    # 63 / 64 / 65, 255 / 256 / 257, the short / long threshold, the histogram's tile and chunk
    edge_lens = [63, 64, 65, 255, 256, 257, SHORT - 1, SHORT, SHORT + 1, SHORT + 2, 2 * SHORT + 1, CHUNK - 1, CHUNK,
                 CHUNK + 1, 2 * CHUNK + 37]
    mp, pp = _grid_world(rng, 5000, len(edge_lens), side=12)
    e_off, e_msgs = _csr(_rows(rng, edge_lens, 5000))
    for k in (7, 64, 255, 256, 257, 2000):
        add(f"len_edges_k{k}", e_off, e_msgs, mp, pp, k=k)
    # rows straddling a granule / tile boundary, the cut row first, in the middle, last
    for tag, big in (("short", 70), ("long", SHORT + 44)):
        for where, lens in (("first", [big, 10, 10]), ("middle", [10, big, 10]), ("last", [10, 10, big]),
                            ("all", [big, big, 3, big])):
            mp, pp = _grid_world(rng, 400, len(lens), side=6)
            add(f"straddle_{tag}_{where}", *_csr(_rows(rng, lens, 400)), mp, pp, k=20)

    # ---- equal keys: position alone decides
    for n, k in ((100, 50), (600, 300), (600, 1), (CHUNK + 100, CHUNK)):
        add(f"ties_all_equal_{n}_k{k}", *_line_case(rng, [3.0], n, peers=2), k=k)
    for n in (80, 800):
        # a quarter nearer, half equal (straddling the threshold at n / 2), a quarter farther
        off, msgs, mp, pp = _line_case(rng, [1.0, 2.0, 2.0, 3.0], n, peers=3)
        add(f"ties_half_{n}", off, msgs, mp, pp, k=n // 2)
    mp, pp = _grid_world(rng, 50, 4)
    add("ties_repeated_message", *_csr([[5, 5, 5, 7, 5], [], [7, 7, 7], [9, 5, 9, 5, 9, 5, 9]]), mp, pp, k=3)
    rep = np.sort(rng.integers(0, 20, size=700))   # every message about 35 times in one long row
    add("ties_repeated_message_long", *_csr([rep, rep[:300]]), mp, pp, k=123)

    # ---- key values
    x = next(v for v in 1.42 + np.arange(1000) * 2.0 ** -40
             if np.float64(np.nextafter(v, 2.0)) ** 2 == np.nextafter(np.float64(v) ** 2, 4.0))
    values = {
        "last_ulp": [x, np.nextafter(x, 2.0)],                               # d2 one ulp apart
        "top_digit": [2.0 ** (8 * j) for j in range(-5, 6)],                 # d2 = 2^(16 j): bits 56.. only
        "overflow": [1e200, 1.0, 1e150, 1e160, 2.0],                         # 1e200^2 and 1e160^2 are +inf
        "subnormal": [2.0 ** -520 * j for j in range(0, 9)],                 # d2 = j^2 2^-1040
        "zero": [0.0, 0.0, 2.0 ** -30, 1.0],
    }
    for name, xs in values.items():
        for n, k in ((40, 20), (40, 1), (700, 350), (700, 3)):
            add(f"keys_{name}_{n}_k{k}", *_line_case(rng, xs, n, peers=2), k=k)
    # differing in the bottom digit only: d2 = 1 + i^2 2^-52 from (1, i 2^-26, 0)
    mp = np.array([[1.0, i * 2.0 ** -26, 0.0] for i in range(16)])
    for n, k in ((40, 20), (700, 350)):
        add(f"keys_bottom_digit_{n}_k{k}", *_csr([rng.integers(0, 16, size=n) for _ in range(2)]), mp, np.zeros((2, 3)), k=k)
    # a NaN message position (and an infinite one): their elements sort last, by position
    mp, pp = _grid_world(rng, 30, 2)
    for i in range(3, 13):      # a third of the messages: NaN, +inf and -inf in every coordinate
        mp[i, i % 3] = (np.nan, np.inf, -np.inf)[i % 3 if i < 12 else 0]
    for n in (40, 700):      # k: all the finite keys of row 0 and half of its infinite ones
        rows = [rng.integers(0, 30, size=n) for _ in range(2)]
        fin = int(np.isfinite(interest.budget_keys_np(rows[0], mp, pp, 0)).sum())
        add(f"keys_nan_position_{n}", *_csr(rows), mp, pp, k=fin + (n - fin) // 2)
    # FMA contraction flips the boundary: a is kept by the definition, b (equal then, and first) by a contracted d2
    pair = fma_pair()
    if pair is not None:
        a, b = pair
        for n_far in (4, 600):
            mp = np.array([[0.5, 0, 0], [0.25, 0, 0], b, a] + [[2.0 + i, 0, 0] for i in range(n_far)])
            add(f"fma_boundary_{n_far + 4}", *_csr([np.arange(len(mp))]), mp, np.zeros((1, 3)), k=3)

    # ---- missing data
    mp, pp = _grid_world(rng, 300, 12, side=8)
    lens = [40, 300, 0, 41, 301, 5, 40, 300, 0, 41, 301, 5]
    off, msgs = _csr(_rows(rng, lens, 300))
    add("missing_peer_positions", off, msgs, mp, pp[:6], k=17)          # peers 6 .. 11 have none
    add("missing_all_peer_positions", off, msgs, mp, pp[:0], k=17)
    bad = msgs.copy()
    bad[rng.choice(len(bad), size=60, replace=False)] = rng.choice([300, 301, U32_MAX, U32_MAX - 1, 1 << 31], size=60)
    add("missing_message_index", off, bad, mp, pp, k=17)                # error bit 1
    add("missing_all_messages", off, msgs, mp[:0], pp, k=17)            # n_msgs == 0 with elements present

    # ---- per-peer budgets
    add("budget_array", off, msgs, mp, pp, k=5,
        budget=[0, 1, U32_MAX, U32_MAX, 0, 1, 39, 299, 7, 41, 300, 4])
    add("budget_all_zero", off, msgs, mp, pp, k=9, budget=np.zeros(12, np.uint32))
    add("budget_all_max", off, msgs, mp, pp, k=0, budget=np.full(12, U32_MAX, np.uint32))

    # ---- degenerate sizes
    add("size_no_peers", np.zeros(1, np.uint32), msgs[:100], mp, pp[:0], k=3)
    add("size_no_elements", np.zeros(1001, np.uint32), msgs[:0], mp, pp, k=3)
    add("size_nothing", np.zeros(1, np.uint32), msgs[:0], mp[:0], pp[:0], k=3)

    # ---- one long row among empty rows
    n_long = 200_000
    mp, _ = _grid_world(rng, 5000, 1, side=40)
    long_off = np.zeros(1002, np.uint32)
    long_off[501:] = n_long
    long_msgs = np.sort(rng.integers(0, 5000, size=n_long))
    pp = np.zeros((1001, 3)) + 17.0
    for k in (100_000, 7):
        add(f"long_row_k{k}", long_off, long_msgs, mp, pp, k=k)

    # ---- hostile offsets
    mp, pp = _grid_world(rng, 300, 12, side=8)
    add("hostile_descending", off[::-1], msgs, mp, pp, k=17, kind="hostile")
    one = off.copy()
    one[4] = 10
    add("hostile_one_descent", one, msgs, mp, pp, k=17, kind="hostile")
    add("hostile_past_n_in", off, msgs[:500], mp, pp, k=17, kind="hostile")
    add("hostile_all_ones", np.full(13, U32_MAX, np.uint32), msgs, mp, pp, k=17, kind="hostile")
    sums = np.cumsum(np.concatenate([[0], rng.integers(0, 1 << 31, size=12)]).astype(np.uint64))
    assert int(sums[-1]) > 1 << 32
    add("hostile_wrapped", (sums & np.uint64(U32_MAX)).astype(np.uint32), msgs, mp, pp, k=17, kind="hostile")
    add("hostile_overlapping", [0, 1300, 0, 1300, 0, 1300, 20, 10, 1369, 0, 5, 0, 700], msgs, mp, pp, k=280,
        kind="hostile")
    return out


def exact_names():
    return sorted(n for n, c in cases().items() if c.kind == "exact")


def hostile_names():
    return sorted(n for n, c in cases().items() if c.kind == "hostile")


def budget_of(c):
    return c.budget.astype(np.int64) if c.budget is not None else np.full(c.n_peers, c.k, np.int64)


@functools.lru_cache(maxsize=None)
def want(name):
    """peer_budget_np of a case, computed once: (out_offsets, out_msgs, counters)."""
    c = cases()[name]
    oo, om, cnt = interest.peer_budget_np(c.offsets, c.msgs, c.msg_pos, c.peer_pos, k=c.k, budget=c.budget)
    oo.setflags(write=False)
    om.setflags(write=False)
    return oo, om, cnt


def well_formed(c, oo, om, counters=None):
    """What include/wq_router.h promises whatever the offsets hold. oo: out_offsets[n_peers + 1],
    om: the kept elements out_msgs[:n_kept], counters: a mapping with n_in, n_kept, rows_cut, error."""
    n_in = len(c.msgs)
    assert len(oo) == c.n_peers + 1 and int(oo[0]) == 0
    lens = np.diff(oo.astype(np.int64))
    assert (lens >= 0).all() and int(oo[-1]) == len(om) <= n_in
    assert (lens <= budget_of(c)).all()
    off = c.offsets.astype(np.int64)
    a, b = np.minimum(off[:-1], n_in), np.minimum(off[1:], n_in)
    clamped = np.maximum(b - a, 0)
    assert (lens <= clamped).all()
    for p in np.flatnonzero(lens):                      # a kept row is a subsequence of its input row
        row, kept = c.msgs[a[p]:a[p] + clamped[p]].tolist(), om[oo[p]:oo[p + 1]].tolist()
        it = iter(row)
        assert all(any(m == x for x in it) for m in kept), int(p)
    if counters is not None:
        assert int(counters["n_kept"]) == int(oo[-1]) and int(counters["n_in"]) <= n_in
        descends = bool(((off[1:] < off[:-1]) | (off[1:] > n_in)).any())
        assert (int(counters["error"]) & 1) == int(descends)
        assert (int(counters["error"]) >> 1) == int(bool(clamped.sum()) and bool((_walked(c) >= len(c.msg_pos)).any()))
        if c.kind == "exact":
            assert int(counters["n_in"]) == int(clamped.sum())
            assert int(counters["rows_cut"]) == int((clamped > budget_of(c)).sum())


def _walked(c):
    """The message indices of the elements the call walks (peer_budget_np's rows)."""
    n_in, off = len(c.msgs), c.offsets.astype(np.int64)
    parts, walked = [], 0
    for p in range(c.n_peers):
        a = min(off[p], n_in)
        n = min(max(min(off[p + 1], n_in) - a, 0), n_in - walked)
        walked += n
        parts.append(c.msgs[a:a + n])
    return np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)


# ---- the independent restatement ------------------------------------------------------------

def py_keys(c, p, row):
    """(d2, position) tuples of a row in Python floats, +inf for NaN and for missing positions."""
    mp, pp = c.msg_pos.tolist(), c.peer_pos.tolist()
    keys = []
    for i, m in enumerate(row):
        d2 = float("inf")
        if m < len(mp) and p < len(pp):
            dx, dy, dz = mp[m][0] - pp[p][0], mp[m][1] - pp[p][1], mp[m][2] - pp[p][2]
            d2 = (dx * dx + dy * dy) + dz * dz
            if d2 != d2:
                d2 = float("inf")
        keys.append((d2, i))
    return keys


def restated(c, budgets=None):
    """Per row: sorted() over (d2, position), the first B, back in input order."""
    off, msgs, n_in = c.offsets.tolist(), c.msgs.tolist(), len(c.msgs)
    budgets = budget_of(c).tolist() if budgets is None else budgets
    oo, om = [0], []
    for p in range(c.n_peers):
        row = msgs[min(off[p], n_in):min(off[p + 1], n_in)]
        first = sorted(py_keys(c, p, row))[:budgets[p]]
        om += [row[i] for i in sorted(i for _, i in first)]
        oo.append(len(om))
    return np.array(oo, np.uint32), np.array(om, np.uint32)


@pytest.mark.parametrize("name", exact_names())
def test_reference_matches_restatement(name):
    c = cases()[name]
    oo, om, cnt = want(name)
    r_oo, r_om = restated(c)
    assert oo.dtype == np.uint32 and om.dtype == np.uint32
    assert oo.tobytes() == r_oo.tobytes() and om.tobytes() == r_om.tobytes()
    well_formed(c, oo, om, cnt)


@pytest.mark.parametrize("name", hostile_names())
def test_reference_is_well_formed_on_hostile_offsets(name):
    c = cases()[name]
    oo, om, cnt = want(name)
    well_formed(c, oo, om, cnt)
    assert cnt["error"] & 1


@pytest.mark.parametrize("name", exact_names())
def test_pass_through(name):
    """B >= the longest row reproduces the input bytes."""
    c = cases()[name]
    longest = int(np.diff(c.offsets.astype(np.int64)).max()) if c.n_peers else 0
    for k in (longest, longest + 1, U32_MAX):
        oo, om, cnt = interest.peer_budget_np(c.offsets, c.msgs, c.msg_pos, c.peer_pos, k=k)
        assert oo.tobytes() == c.offsets.tobytes() and om.tobytes() == c.msgs[:int(c.offsets[-1])].tobytes()
        assert cnt["rows_cut"] == 0


def _kept_positions(c, k):
    """Per row the kept positions at budget k for everyone (from the reference: the kept elements are
    matched back to their positions through the total order)."""
    oo, om, _ = interest.peer_budget_np(c.offsets, c.msgs, c.msg_pos, c.peer_pos, k=k)
    sets = []
    for p in range(c.n_peers):
        row = c.msgs[int(c.offsets[p]):int(c.offsets[p + 1])]
        d2 = interest.budget_keys_np(row, c.msg_pos, c.peer_pos, p)
        order = np.lexsort((np.arange(len(row)), d2))
        n = int(oo[p + 1]) - int(oo[p])
        kept = np.sort(order[:n])
        assert row[kept].tobytes() == om[int(oo[p]):int(oo[p + 1])].tobytes()
        sets.append((kept, d2))
    return sets


@pytest.mark.parametrize("name", [n for n in exact_names() if not n.startswith("long_row")])
def test_monotone_and_nearest(name):
    """The kept set at budget B is a subset of the kept set at B + 1, and in every cut row the largest
    kept (d2, position) is below the smallest dropped one."""
    c = cases()[name]
    for B in sorted({0, 1, 2, 31, c.k, SHORT - 1, SHORT}):
        lo, hi = _kept_positions(c, B), _kept_positions(c, B + 1)
        for (kl, d2), (kh, _) in zip(lo, hi):
            assert set(kl.tolist()) <= set(kh.tolist())
            if 0 < len(kl) < len(d2):
                dropped = np.setdiff1d(np.arange(len(d2)), kl)
                worst = max((d2[i], i) for i in kl.tolist())
                best = min((d2[i], i) for i in dropped.tolist())
                assert worst < best


def _bits(c, p, row):
    return interest.budget_keys_np(row, c.msg_pos, c.peer_pos, p).view(np.uint64)


def test_case_conditions():
    """What the rows are there for, from the reference alone."""
    c = cases()
    # keys: the values differ where the name says
    ulp = _bits(c["keys_last_ulp_40_k20"], 0, [0, 1])
    assert int(ulp[1]) - int(ulp[0]) == 1
    top = _bits(c["keys_top_digit_40_k20"], 0, np.arange(11))
    assert len(set(top.tolist())) == 11 and len({int(b) & ((1 << (64 - DIGIT_BITS)) - 1) for b in top}) == 1
    bot = _bits(c["keys_bottom_digit_40_k20"], 0, np.arange(16))
    assert len(set(bot.tolist())) == 16 and len({int(b) >> DIGIT_BITS for b in bot}) == 1
    ovf = _bits(c["keys_overflow_40_k20"], 0, np.arange(5))
    assert int(ovf[0]) == INF_BITS and int(ovf[3]) == INF_BITS and int(ovf[2]) < INF_BITS
    sub = interest.budget_keys_np(np.arange(9), c["keys_subnormal_40_k20"].msg_pos, np.zeros((1, 3)), 0)
    assert sub[0] == 0 and (sub[1:] > 0).all() and (sub < np.finfo(np.float64).tiny).all() and len(set(sub)) == 9
    nan = _bits(c["keys_nan_position_40"], 0, [3, 7, 11])
    assert (nan == INF_BITS).all()
    for name in ("keys_nan_position_40", "keys_nan_position_700"):
        oo, om, _ = want(name)     # some +inf elements are kept and some dropped: position decides among them
        cc = cases()[name]
        row = cc.msgs[:int(cc.offsets[1])]
        inf = _bits(cc, 0, row) == INF_BITS
        kept_inf = int(oo[1]) - int((~inf).sum())
        assert 0 < kept_inf < int(inf.sum()), name
    # ties: the threshold key is shared by kept and dropped elements
    for name in ("ties_all_equal_600_k300", "ties_half_80", "ties_half_800", "ties_repeated_message_long"):
        cc = cases()[name]
        oo, om, cnt = want(name)
        assert cnt["rows_cut"] >= 1 and 0 < cnt["n_kept"] < cnt["n_in"]
    assert want("ties_repeated_message")[2]["rows_cut"] == 2 and want("ties_repeated_message")[2]["n_kept"] == 9
    # both kernels' paths see cut rows: short ones and long ones, in one case even
    lens = np.diff(c["len_edges_k64"].offsets.astype(np.int64))
    assert (lens <= SHORT).any() and (lens > SHORT).any() and SHORT in lens and SHORT + 1 in lens
    assert CHUNK in lens and CHUNK + 1 in lens and TILE == SHORT
    # missing data
    assert want("missing_message_index")[2]["error"] == 2 and want("missing_all_messages")[2]["error"] == 2
    assert want("missing_peer_positions")[2]["error"] == 0
    cc = c["missing_all_messages"]     # every key +inf: the first B of every row
    oo, om, _ = want("missing_all_messages")
    for p in range(cc.n_peers):
        a = int(cc.offsets[p])
        assert om[int(oo[p]):int(oo[p + 1])].tobytes() == cc.msgs[a:a + int(oo[p + 1]) - int(oo[p])].tobytes()
    # budgets
    oo = want("budget_array")[0]
    assert np.diff(oo.astype(np.int64)).tolist() == [0, 1, 0, 41, 0, 1, 39, 299, 0, 41, 300, 4]
    assert want("budget_all_zero")[2]["n_kept"] == 0 and want("budget_all_max")[2]["rows_cut"] == 0
    # sizes
    for name in ("size_no_peers", "size_no_elements", "size_nothing"):
        assert not want(name)[0].any() and len(want(name)[1]) == 0
    assert want("long_row_k100000")[2]["n_kept"] == 100_000 and want("long_row_k7")[2]["n_kept"] == 7
    # hostile: overlapping rows reach the n_in limit
    assert want("hostile_overlapping")[2]["n_in"] == len(c["hostile_overlapping"].msgs)


def test_an_fma_boundary_case_exists():
    """At least one case whose boundary decision a contracted d2 flips: numpy keeps a, FMA keeps b."""
    names = [n for n in cases() if n.startswith("fma_boundary_")]
    assert len(names) == 2
    for name in names:
        c = cases()[name]
        a, b = c.msg_pos[3], c.msg_pos[2]
        plain = lambda v: (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        assert plain(a) < plain(b) and d2_contracted(*a.tolist()) == d2_contracted(*b.tolist())
        om = want(name)[1].tolist()
        assert om == [0, 1, 3]          # a contracted key would give [0, 1, 2]


def test_arguments():
    off, msgs = np.array([0, 3, 3, 5], np.uint32), np.array([0, 1, 2, 2, 0], np.uint32)
    mp = np.array([[3.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    pp = np.zeros((3, 3))
    oo, om, cnt = interest.peer_budget_np(off, msgs, mp, pp, k=2)
    assert oo.tolist() == [0, 2, 2, 4] and om.tolist() == [1, 2, 2, 0]
    assert cnt == dict(n_in=5, n_kept=4, rows_cut=1, error=0)
    oo, om, cnt = interest.peer_budget_np(off, msgs, mp, pp, budget=[1, 9, 1])
    assert oo.tolist() == [0, 1, 1, 2] and om.tolist() == [1, 2] and cnt["rows_cut"] == 2
    with pytest.raises(ValueError):
        interest.peer_budget_np(off, msgs, mp, pp)
