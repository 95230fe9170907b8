"""The host reference of the interest diff (worldql_server_amd/interest.py csr_diff_np) against a
brute force of Python sets per row. `cases()` is shared with the C++ mirror
(tests/test_csr_diff_cpp_mirror.py) and the GPU instance (tests/test_gpu_csr_diff.py). No GPU needed."""
import functools

import numpy as np
import pytest

from worldql_server_amd import interest

U32_MAX = 0xFFFFFFFF
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257)


def csr(rows):
    """A CSR from a list of rows (each an iterable of distinct peer ids; stored ascending)."""
    rows = [np.array(sorted(r), dtype=np.uint32) for r in rows]
    offsets = np.zeros(len(rows) + 1, dtype=np.uint32)
    if rows:
        np.cumsum([len(r) for r in rows], out=offsets[1:])
    peers = np.concatenate(rows) if rows else np.zeros(0, np.uint32)
    return offsets, peers.astype(np.uint32)


def rows_of(offsets, peers):
    return [peers[int(offsets[m]):int(offsets[m + 1])] for m in range(len(offsets) - 1)]


def _random_rows(rng, n_rows, id_range):
    old, new = [], []
    for _ in range(n_rows):
        lo, ln = rng.choice(LENGTHS, 2)
        k = int(max(lo, ln) * 1.5) + 2
        pool = np.unique(rng.integers(0, id_range, size=3 * k))  # overlapping draws from one pool
        assert len(pool) >= max(lo, ln)
        old.append(rng.choice(pool, size=int(lo), replace=False))
        new.append(rng.choice(pool, size=int(ln), replace=False))
    return old, new


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (old_offsets, old_peers, new_offsets, new_peers); built once, never modified."""
    rng = np.random.default_rng(41)
    out = {}
    a = list(range(10, 20))
    out["small_mix"] = (
        # empty/empty, empty/full, full/empty, identical, disjoint, interleaved, the extreme ids
        [[], [], a, a, [1, 3, 5], [0, 2, 4, 6, 8], [0, U32_MAX], [U32_MAX], [0], []],
        [[], a, [], a, [2, 4, 6], [1, 2, 3, 4, 5], [U32_MAX], [0, U32_MAX], [0, 1, U32_MAX], []])
    long_old = rng.choice(1 << 20, size=5000, replace=False)
    long_new = np.concatenate([long_old[:3000], (1 << 20) + rng.choice(1 << 20, size=2000, replace=False)])
    out["one_long_row"] = ([[], [], long_old, [], []], [[], [], long_new, [], [7]])
    out["random_2000"] = _random_rows(rng, 2000, 1 << 16)
    for n in (0, 1, 255, 256, 257, 513):  # rows straddling tile and block edges
        out[f"rows_{n}"] = _random_rows(np.random.default_rng(100 + n), n, 1 << 12)
    # long rows and skew: 5,000 peers against 4,999 shifted by one (interleaved, with a run in
    # common) among 300 empty rows; then 64 rows of 257 peers
    base = np.arange(0, 10000, 2)
    shifted = np.concatenate([base[1:2500], base[2500:] + 1])
    out["skew_5000"] = ([[]] * 150 + [base] + [[]] * 150, [[]] * 150 + [shifted] + [[]] * 150)
    o257, n257 = [], []
    for _ in range(64):
        pool = rng.choice(1 << 14, size=400, replace=False)
        o257.append(pool[:257])
        n257.append(pool[100:357])
    out["rows_of_257"] = (o257, n257)
    built = {}
    for name, (old, new) in out.items():
        arrs = csr(old) + csr(new)
        for x in arrs:
            x.setflags(write=False)
        built[name] = arrs
    return built


def descending_pair(offsets, peers):
    """A copy of the CSR with offsets[m + 1] = offsets[m] - 3 for one row m in the middle: row m is
    then empty and row m + 1 starts three elements inside row m - 1. The peers of rows m - 1 .. m + 1
    are rewritten as one ascending run, so every clamped row is still ascending and distinct."""
    lens = np.diff(offsets.astype(np.int64))
    m = next(i for i in range(len(lens) // 2, len(lens) - 1) if lens[i - 1] >= 3 and lens[i] >= 1 and lens[i + 1] >= 1)
    off, p = offsets.copy(), peers.copy()
    a, b = int(off[m - 1]), int(off[m + 2])
    p[a:b] = 5 * np.arange(b - a, dtype=np.uint32) + 1
    off[m + 1] = off[m] - 3
    return off, p


def brute(oo, op, no, npr):
    ent, left = [], []
    for o, n in zip(rows_of(oo, op), rows_of(no, npr)):
        so, sn = set(o.tolist()), set(n.tolist())
        ent.append(sn - so)
        left.append(so - sn)
    return csr(ent), csr(left)


@pytest.mark.parametrize("name", sorted(cases()))
def test_matches_sets_per_row(name):
    oo, op, no, npr = cases()[name]
    eo, ep, lo, lp = interest.csr_diff_np(oo, op, no, npr)
    (w_eo, w_ep), (w_lo, w_lp) = brute(oo, op, no, npr)
    for got, want in ((eo, w_eo), (ep, w_ep), (lo, w_lo), (lp, w_lp)):
        assert got.dtype == np.uint32 and got.tobytes() == want.tobytes()
    # (old ∪ entered) \ left == new, row by row
    for o, n, e, l in zip(rows_of(oo, op), rows_of(no, npr), rows_of(eo, ep), rows_of(lo, lp)):
        assert (set(o.tolist()) | set(e.tolist())) - set(l.tolist()) == set(n.tolist())
        assert (np.diff(e.astype(np.int64)) > 0).all() and (np.diff(l.astype(np.int64)) > 0).all()


def test_cases_cover_the_edges():
    c = cases()
    oo, op, no, npr = c["small_mix"]
    assert 0 in op and U32_MAX in op and 0 in npr and U32_MAX in npr
    oo, op, no, npr = c["one_long_row"]
    assert 5000 in np.diff(oo.astype(np.int64)) and 5000 in np.diff(no.astype(np.int64))
    oo, op, no, npr = c["random_2000"]
    assert len(oo) == 2001 and set(np.diff(oo.astype(np.int64)).tolist()) == set(LENGTHS)
    eo, ep, lo, lp = interest.csr_diff_np(*c["skew_5000"])
    assert len(ep) == 2500 and len(lp) == 2501   # interleaved half, common half


def test_clamp_is_the_identity_on_a_csr_and_cuts_what_is_outside():
    oo, op, no, npr = cases()["rows_257"]
    o, p, cut = interest.clamp_csr_np(no, npr)
    assert not cut and o.tobytes() == no.tobytes() and p.tobytes() == npr.tobytes()
    # a truncated tick: capacity below offsets[n_rows]
    cap = int(no[-1]) // 2
    o, p, cut = interest.clamp_csr_np(no, npr[:cap], cap)
    assert cut and int(o[-1]) == cap and p.tobytes() == npr[:cap].tobytes()
    assert (o == np.minimum(no, cap)).all()
    # one descending pair: that row is empty, the next one starts where its own offset says
    off = np.array([0, 5, 9, 7, 12], np.uint32)
    pe = np.arange(12, dtype=np.uint32)
    o, p, cut = interest.clamp_csr_np(off, pe)
    assert cut and o.tolist() == [0, 5, 9, 9, 14]
    assert p.tolist() == list(range(0, 9)) + list(range(7, 12))


def test_rejects_offsets_that_do_not_ascend():
    with pytest.raises(ValueError):
        interest.csr_diff_np([0, 2, 1], [1, 2], [0, 1, 2], [1, 2])
