"""The host definition of the per-peer send lists (worldql_server_amd/interest.py peer_major_np)
against a brute force of Python dicts. `cases()` is shared with the C++ mirror
(tests/test_peer_major_cpp_mirror.py) and the GPU instance (tests/test_gpu_peers.py). No GPU needed.

A case is the argument list of one wq_peer_major_device call: offsets[n_msgs + 1], peers[n_pairs]
(n_pairs = len(peers): a cut tick's offsets reach past it, a padded buffer's end before it),
n_peers, the connected bitmap (exactly ceil(n_peers / 32) words, or None) and its kind: "exact"
(ascending offsets: the result is peer_major_np's, byte for byte) or "hostile" (only the
well-formedness clauses of include/wq_router.h hold; `well_formed` states them)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from worldql_server_amd import interest

U32_MAX = 0xFFFFFFFF
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257)
SWEEP_N_PEERS = (0, 1, 2, 3, 31, 32, 33, 255, 256, 257, 65535, 65536, 65537, 1 << 20)
SWEEP_ID_RANGE = 70000
EDGE_N_PEERS = 100
EDGE_PEERS = (0, 31, 32, 63, 64, EDGE_N_PEERS - 1)


def _csr(rows):
    """A CSR from a list of rows, the peers of a row kept in the order given."""
    offsets = np.zeros(len(rows) + 1, dtype=np.uint32)
    if rows:
        np.cumsum([len(r) for r in rows], out=offsets[1:])
    peers = np.concatenate([np.asarray(r, dtype=np.uint32) for r in rows]) if rows else np.zeros(0, np.uint32)
    return offsets, peers.astype(np.uint32)


def _random_rows(rng, n_rows, id_range, lengths=LENGTHS):
    return [np.sort(rng.integers(0, id_range, size=int(rng.choice(lengths)))) for _ in range(n_rows)]


def _bitmap(rng, n_peers, frac=0.7):
    """Exactly ceil(n_peers / 32) words; the bits past n_peers in the last word are random too."""
    n_words = (n_peers + 31) // 32
    bits = rng.random(n_words * 32) < frac
    return np.packbits(bits, bitorder="little").view(np.uint32) if n_words else np.zeros(0, np.uint32)


def _only(n_peers, peer, connected):
    """The bitmap with `peer` alone connected (or alone disconnected)."""
    words = np.zeros((n_peers + 31) // 32, np.uint32) if connected else np.full((n_peers + 31) // 32, U32_MAX, np.uint32)
    words[peer >> 5] ^= np.uint32(1 << (peer & 31))
    return words


def sweep_csr():
    """The CSR of the n_peers sweep, the cut and the padded rows: 300 rows with lengths from LENGTHS,
    ids drawn below 70,000. The ids n - 1 and n of every swept n_peers are planted one per row (the
    draw cannot give 2^20, and need not give the others), so each radix width sees its largest peer
    and its sentinel's twin."""
    rng = np.random.default_rng(77)
    rows = _random_rows(rng, 300, SWEEP_ID_RANGE)
    plant = sorted({n + d for n in SWEEP_N_PEERS for d in (-1, 0) if n + d >= 0})
    at = [m for m in range(300) if len(rows[m]) >= 2]
    for m, v in zip(at, plant):
        rows[m] = np.sort(np.concatenate([rows[m][:-1], [v]]))
    return _csr(rows)


def wrapped_offsets(n_rows=2000):
    """Offsets as a tick past the 2^32-pair limit leaves them: cumulative sums taken mod 2^32. The
    first 60 rows are short (their offsets stay below the 5000 pairs the case passes), the rest
    are up to 8M pairs long, so the sums wrap about twice."""
    rng = np.random.default_rng(78)
    lens = np.concatenate([rng.choice(LENGTHS[:6], size=60), rng.integers(0, 1 << 23, size=n_rows - 60)]).astype(np.uint64)
    sums = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
    assert int(sums[-1]) > 1 << 32 and 1000 < int(sums[60]) < 5000
    off = (sums & np.uint64(U32_MAX)).astype(np.uint32)
    assert (np.diff(off.astype(np.int64)) < 0).any()
    return off


@functools.lru_cache(maxsize=None)
def cases():
    """name -> SimpleNamespace(offsets, peers, n_msgs, n_peers, connected, kind); built once, never
    modified (the arrays are read-only)."""
    rng = np.random.default_rng(43)
    out = {}

    def add(name, offsets, peers, n_peers, connected=None, kind="exact"):
        offsets, peers = np.ascontiguousarray(offsets, np.uint32), np.ascontiguousarray(peers, np.uint32)
        if connected is not None:
            connected = np.ascontiguousarray(connected, np.uint32)
            assert len(connected) == (n_peers + 31) // 32
            connected.setflags(write=False)
        offsets.setflags(write=False)
        peers.setflags(write=False)
        assert name not in out
        out[name] = SimpleNamespace(offsets=offsets, peers=peers, n_msgs=len(offsets) - 1, n_peers=int(n_peers),
                                    connected=connected, kind=kind)

    # ---- the n_peers sweep: every radix width at a power of two, with and without a bitmap
    s_off, s_peers = sweep_csr()
    P = int(s_off[-1])
    assert len(s_peers) == P and 15000 < P < 45000
    for n in SWEEP_N_PEERS:
        add(f"sweep_{n}", s_off, s_peers, n)
        add(f"sweep_{n}_bitmap", s_off, s_peers, n, _bitmap(rng, n))

    # ---- bitmap word edges: one peer alone connected, then alone disconnected
    e_off, e_peers = _csr(_random_rows(rng, 60, EDGE_N_PEERS + 10, (0, 1, 2, 63, 64, 65)))
    assert set(EDGE_PEERS) <= set(e_peers.tolist())
    for p in EDGE_PEERS:
        add(f"edge_only_{p}_on", e_off, e_peers, EDGE_N_PEERS, _only(EDGE_N_PEERS, p, True))
        add(f"edge_only_{p}_off", e_off, e_peers, EDGE_N_PEERS, _only(EDGE_N_PEERS, p, False))

    # ---- rows
    some = lambda k: _random_rows(rng, k, 3000, (1, 2, 63, 65))
    add("rows_empty_runs", *_csr([[]] * 300 + some(7) + [[]] * 300 + some(5) + [[]] * 300), 3000, _bitmap(rng, 3000))
    for n in (0, 1, 255, 256, 257, 513):
        add(f"rows_{n}", *_csr(_random_rows(np.random.default_rng(200 + n), n, 1 << 12, (0, 1, 2, 3, 63, 64, 65))),
            (1 << 12) - 5, _bitmap(rng, (1 << 12) - 5))
    short = _random_rows(rng, 500, 70000, (0, 1, 2, 3))
    add("rows_hot_70000", *_csr(short[:250] + [np.arange(70000)] + short[250:]), 69000, _bitmap(rng, 69000))
    add("rows_repeated_peer", *_csr([[5, 5, 5, 7, 5], [], [7, 7], [5], [9, 5, 9, 5, 9], [40, 40, 40]]), 40,
        _only(40, 7, False))
    add("rows_extreme_ids", *_csr([[0, 1], [U32_MAX, U32_MAX - 1, 3], [U32_MAX], [2, U32_MAX - 1]]), 1 << 20,
        _bitmap(rng, 1 << 20, 0.9) | np.uint32(0xF))

    # ---- sizes: peer_offsets is written in full, all zeros
    add("size_no_pairs", np.zeros(11, np.uint32), np.zeros(0, np.uint32), 1000)
    add("size_both_zero", np.zeros(1, np.uint32), np.zeros(0, np.uint32), 1000)
    add("size_no_peers", e_off, e_peers, 0)

    # ---- padded: the buffer is 1000 words longer than offsets[M]; the words behind it are valid,
    # connected peer ids, and belong to nobody. The two all-valid cases are the calls that leave
    # plausible keys in the handle's scratch before it (tests/test_gpu_peers.py).
    pad_conn = _bitmap(rng, 65536)
    valid = np.flatnonzero(np.unpackbits(pad_conn.view(np.uint8), bitorder="little")).astype(np.uint32)
    add("padded_1000", s_off, np.concatenate([s_peers, rng.choice(valid, size=1000)]), 65536, pad_conn)
    for name, n in (("all_valid_larger", P + 5000), ("all_valid_smaller", P // 2)):
        add(name, [0, n // 3, n // 3, n], rng.choice(valid, size=n), 65536, pad_conn)
    # no rows at all over 1000 valid, connected ids, with the same n_peers and bitmap as the calls
    # above: keys they left behind would sort in as sends
    add("size_no_msgs_1000_pairs", np.zeros(1, np.uint32), rng.choice(valid, size=1000), 65536, pad_conn)

    # ---- cut: the tick's buffer ended before offsets[M]
    m_mid = next(m for m in range(150, 300) if int(s_off[m + 1]) - int(s_off[m]) >= 255)
    cuts = {"0": 0, "1": 1, "row_start": int(s_off[150]), "mid_row": int(s_off[m_mid]) + 100, "last": P - 1}
    assert int(s_off[150]) > 1 and all(c < P for c in cuts.values())
    cut_conn = _bitmap(rng, 65536)
    for name, c in cuts.items():
        add(f"cut_{name}", s_off, s_peers[:c], 65536, cut_conn)

    # ---- hostile offsets: unspecified but well formed
    add("hostile_wrapped", wrapped_offsets(), rng.integers(0, 70000, size=5000), 65536, cut_conn, "hostile")
    add("hostile_descending", s_off[::-1], s_peers, 65536, cut_conn, "hostile")
    add("hostile_all_ones", np.full(301, U32_MAX, np.uint32), s_peers[:5000], 65536, cut_conn, "hostile")
    return out


def exact_names():
    return sorted(n for n, c in cases().items() if c.kind == "exact")


def hostile_names():
    return sorted(n for n, c in cases().items() if c.kind == "hostile")


@functools.lru_cache(maxsize=None)
def want(name):
    """peer_major_np of an exact case, computed once."""
    c = cases()[name]
    po, rows = interest.peer_major_np(c.offsets, c.peers, c.n_peers, c.connected)
    po.setflags(write=False)
    rows.setflags(write=False)
    return po, rows


def well_formed(c, po, msgs):
    """What include/wq_router.h promises whatever the offsets hold. po: peer_offsets[n_peers + 1],
    msgs: msgs_out[n_pairs]."""
    n_pairs = len(c.peers)
    assert len(po) == c.n_peers + 1 and len(msgs) == n_pairs
    assert int(po[0]) == 0 and (np.diff(po.astype(np.int64)) >= 0).all()
    kept = int(po[-1])
    assert kept <= n_pairs
    assert (msgs[:kept] < c.n_msgs).all()
    assert (msgs[kept:] < max(c.n_msgs, 1)).all()   # behind the kept ones: a row index, or 0 with no rows


def brute(c):
    """Per peer the rows that hold it, by dicts and Python ints: (peer_offsets, rows)."""
    off, peers, cap = c.offsets.tolist(), c.peers.tolist(), len(c.peers)
    words = c.connected.tolist() if c.connected is not None else None
    lists = {}
    for m in range(c.n_msgs):
        for j in range(min(off[m], cap), min(off[m + 1], cap)):
            p = peers[j]
            if p < c.n_peers and (words is None or (words[p // 32] >> (p % 32)) & 1):
                lists.setdefault(p, []).append(m)
    po, rows = [0] * (c.n_peers + 1), []
    for p in sorted(lists):
        po[p + 1] = len(lists[p])
        rows += lists[p]
    return np.cumsum(po, dtype=np.int64).astype(np.uint32), np.array(rows, dtype=np.uint32)


@pytest.mark.parametrize("name", exact_names())
def test_reference_matches_brute_force(name):
    c = cases()[name]
    po, rows = want(name)
    b_po, b_rows = brute(c)
    assert po.dtype == np.uint32 and rows.dtype == np.uint32
    assert po.tobytes() == b_po.tobytes() and rows.tobytes() == b_rows.tobytes()
    well_formed(c, po, np.concatenate([rows, np.zeros(len(c.peers) - len(rows), np.uint32)]))


def test_sweep_conditions():
    """The sweep sees a kept and a dropped pair at every n_peers >= 255, and at the powers of two the
    largest peer and the sentinel's twin are both in the input (from the reference alone)."""
    off, peers = sweep_csr()
    P = int(off[-1])
    ids = set(peers.tolist())
    assert max(ids) == 1 << 20 and sorted(ids)[-3] < SWEEP_ID_RANGE
    for n in SWEEP_N_PEERS:
        for name in (f"sweep_{n}", f"sweep_{n}_bitmap"):
            kept = int(want(name)[0][-1])
            assert kept <= P
            if n >= 255:
                assert 0 < kept < P, name
            if n == 0:
                assert kept == 0
        if n & (n - 1) == 0 and n:
            assert n - 1 in ids and n in ids, n
        # the bitmap drops more than the id bound alone
        assert n < 31 or int(want(f"sweep_{n}_bitmap")[0][-1]) < int(want(f"sweep_{n}")[0][-1])


def test_case_conditions():
    """What the other rows are there for, from the reference alone."""
    c = cases()
    for p in EDGE_PEERS:
        on, off_ = want(f"edge_only_{p}_on"), want(f"edge_only_{p}_off")
        n_p = int((c["edge_only_0_on"].peers == p).sum())
        assert n_p > 0 and int(on[0][-1]) == n_p
        assert int(off_[0][-1]) == int((c["edge_only_0_on"].peers < EDGE_N_PEERS).sum()) - n_p
    for name in ("size_no_pairs", "size_no_msgs_1000_pairs", "size_both_zero", "size_no_peers"):
        assert not want(name)[0].any() and len(want(name)[1]) == 0
    # the padding contributes nothing: the padded result is the unpadded one
    pad = c["padded_1000"]
    plain = interest.peer_major_np(pad.offsets, pad.peers[:int(pad.offsets[-1])], pad.n_peers, pad.connected)
    assert len(pad.peers) == int(pad.offsets[-1]) + 1000
    assert want("padded_1000")[0].tobytes() == plain[0].tobytes() and want("padded_1000")[1].tobytes() == plain[1].tobytes()
    for name in ("all_valid_larger", "all_valid_smaller"):   # every pair kept: the keys they leave are plausible
        assert int(want(name)[0][-1]) == len(c[name].peers)
    assert len(c["all_valid_larger"].peers) > len(pad.peers) > len(c["all_valid_smaller"].peers)
    # a repeated peer keeps its repeats; the extreme ids are dropped
    po, rows = want("rows_repeated_peer")
    assert rows[int(po[5]):int(po[6])].tolist() == [0, 0, 0, 0, 3, 4, 4] and int(po[8]) == int(po[7])
    assert int(want("rows_extreme_ids")[0][-1]) == 4
    hot = c["rows_hot_70000"]
    assert int(np.diff(hot.offsets.astype(np.int64)).max()) == 70000 and hot.n_msgs == 501
    for name in (n for n in c if n.startswith("cut_")):
        assert len(c[name].peers) < int(c[name].offsets[-1])
    assert 0 < int(want("cut_mid_row")[0][-1]) < int(want("cut_last")[0][-1])


def test_existing_callers_and_arguments():
    """The three-argument form is unchanged: peers longer than offsets[M] are not read, ids >= n_peers
    are dropped; capacity cuts the rows; offsets that descend are refused."""
    off, peers = np.array([0, 2, 2, 5], np.uint32), np.array([3, 1, 9, 1, 3, 77, 78], np.uint32)
    po, rows = interest.peer_major_np(off, peers, 4)
    assert po.tolist() == [0, 0, 2, 2, 4] and rows.tolist() == [0, 2, 0, 2]
    po, rows = interest.peer_major_np(off, peers, 4, capacity=4)
    assert po.tolist() == [0, 0, 2, 2, 3] and rows.tolist() == [0, 2, 0]
    po, rows = interest.peer_major_np(off, peers, 4, connected=np.array([0b0010], np.uint32))
    assert po.tolist() == [0, 0, 2, 2, 2] and rows.tolist() == [0, 2]
    with pytest.raises(ValueError):
        interest.peer_major_np(off[::-1], peers, 4)
    with pytest.raises(ValueError):
        interest.peer_major_np(off, peers, 4, capacity=8)
