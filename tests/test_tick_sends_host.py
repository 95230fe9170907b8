"""The host definition of the tick sends (worldql_server_amd/interest.py tick_sends_np) against a
per-element restatement in Python ints. `cases()` is shared with the C++ mirror
(tests/test_tick_sends_cpp_mirror.py) and the GPU instance (tests/test_gpu_tick_sends.py). No GPU needed.

A case is the argument list of one wq_tick_sends_device call: the regions (abi.SEND_REGION_DTYPE), the
offsets and peers they point into, the two src arrays, n_peers, n_frames, the connected bitmap (exactly
ceil(n_peers / 32) words, or None) and its kind: "exact" (ascending offsets: the result is
tick_sends_np's, byte for byte) or "hostile" (only the well-formedness clauses of include/wq_router.h
hold; `well_formed` states them). `invalid_cases()` are the calls the C ABI refuses."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from worldql_server_amd import abi, interest

U32_MAX = 0xFFFFFFFF
UNIT, NO_SRC = abi.SEND_UNIT_ROWS, abi.SEND_NO_SRC
FILL = 1          # what lies in a region's elements behind its pairs: a valid peer id, so covering it shows


class Layout:
    """Regions laid into shared offsets / peers / src arrays, as IngestTick.process leaves them."""

    def __init__(self):
        self.off, self.peers, self.src, self.regions = [], [], ([], []), []

    def pad(self, off=0, peers=0, src=(0, 0)):
        """Junk between regions: the next one starts wherever this ends."""
        self.off += [U32_MAX - 3] * off
        self.peers += [FILL] * peers
        for k in (0, 1):
            self.src[k].extend([7] * src[k])
        return self

    def _src(self, frames, sel):
        if frames is None:
            return NO_SRC
        at = len(self.src[sel])
        self.src[sel].extend(int(f) for f in frames)
        return at

    def csr(self, rows, frames=None, sel=0, base=0, capacity=None, offsets=None):
        """A routed region: region-local offsets, the pairs cut or padded to `capacity`."""
        flat = [int(p) for r in rows for p in r]
        o = offsets if offsets is not None else np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
        cap = len(flat) if capacity is None else capacity
        g = abi.send_region(off_at=len(self.off), peers_at=len(self.peers), n_rows=len(o) - 1, capacity=cap,
                            src_at=self._src(frames, sel), frame_base=base, src_sel=sel)
        self.off += [int(x) for x in o]
        self.peers += (flat + [FILL] * max(cap - len(flat), 0))[:cap]
        self.regions.append(g)
        return self

    def unit(self, peers, frames=None, sel=0, base=0, n_rows=None, capacity=None):
        """A unit-row region: row r is element r."""
        cap = len(peers) if capacity is None else capacity
        g = abi.send_region(off_at=UNIT, peers_at=len(self.peers), n_rows=len(peers) if n_rows is None else n_rows,
                            capacity=cap, src_at=self._src(frames, sel), frame_base=base, src_sel=sel)
        self.peers += ([int(p) for p in peers] + [FILL] * max(cap - len(peers), 0))[:cap]
        self.regions.append(g)
        return self

    def case(self, n_peers, n_frames, connected=None, kind="exact"):
        ro = lambda a, dt=np.uint32: _readonly(np.array(a, dtype=dt))
        if connected is not None:
            connected = ro(connected)
            assert len(connected) == (n_peers + 31) // 32
        reg = ro(self.regions, abi.SEND_REGION_DTYPE) if self.regions else ro(np.zeros(0, abi.SEND_REGION_DTYPE), abi.SEND_REGION_DTYPE)
        return SimpleNamespace(regions=reg, offsets=ro(self.off), peers=ro(self.peers), srcs=(ro(self.src[0]), ro(self.src[1])),
                               n_peers=int(n_peers), n_frames=int(n_frames), connected=connected, kind=kind, n_pairs=len(self.peers),
                               n_elems=int(reg["capacity"].astype(np.int64).sum()))


def _readonly(a):
    a.setflags(write=False)
    return a


def _bitmap(rng, n_peers, frac=0.5):
    """Exactly ceil(n_peers / 32) words; the bits past n_peers in the last word are random too."""
    n_words = (n_peers + 31) // 32
    bits = rng.random(n_words * 32) < frac
    return np.packbits(bits, bitorder="little").view(np.uint32) if n_words else np.zeros(0, np.uint32)


def _random_rows(rng, n_rows, id_range, lengths):
    return [np.sort(rng.integers(0, id_range, size=int(rng.choice(lengths)))).tolist() for _ in range(n_rows)]


def mixed_layout(seed=5, big_peer=(1 << 20) + 2, big_frame=4999):
    """A tick of 400 frames as process() leaves it: 40 read runs, each with a local region, a global
    region or both, whose rows interleave by frame; regions begin at multiples of four and are padded to
    rows * 12 pairs; row lengths 0 .. 65; peers below 310 (a few fall outside n_peers = 300). Two unit-row
    regions behind them carry one peer and one frame that only the wide key holds."""
    rng = np.random.default_rng(seed)
    L = Layout()
    frame = 0
    for run in range(40):
        n = int(rng.integers(1, 14))
        kinds = rng.integers(0, 2, size=n) if run % 3 else np.full(n, run % 2)
        frames = np.arange(frame, frame + n)
        frame += n + int(rng.integers(0, 3))          # the frames between the runs were table ops
        for sel in (0, 1):
            f = frames[kinds == sel]
            if len(f):
                rows = _random_rows(rng, len(f), 310, (0, 1, 2, 3, 5, 12, 65) if run == 7 else (0, 1, 2, 3, 5, 12))
                L.csr(rows, f, sel=sel, capacity=max(len(f) * 12, sum(map(len, rows))))
                L.pad(off=-len(L.off) % 4, peers=-len(L.peers) % 4)
    assert frame <= 400
    L.unit([3, big_peer, 299], frames=[big_frame, 17, 399], sel=1)
    L.unit([0, 5, 6], base=big_frame - 1)              # frames big_frame - 1, big_frame and the one behind it
    return L


@functools.lru_cache(maxsize=None)
def cases():
    """name -> SimpleNamespace(regions, offsets, peers, srcs, n_peers, n_frames, connected, kind, n_elems);
    built once, never modified (the arrays are read-only)."""
    rng = np.random.default_rng(91)
    out = {}
    rows5 = [[2, 9], [], [9, 4, 9], [0], [7, 9, 30]]

    out["no_regions"] = Layout().pad(off=3, peers=5).case(40, 10)
    out["no_peers"] = Layout().csr(rows5).case(0, 5)
    out["no_frames"] = Layout().csr(rows5).case(40, 0)
    out["no_elems"] = Layout().csr([[], []], capacity=0).unit([], n_rows=4).case(40, 5)
    out["identity"] = Layout().csr(_random_rows(rng, 300, 3000, (0, 1, 2, 63, 64, 65, 257))).case(2990, 300, _bitmap(rng, 2990, 0.7))
    # one read run: the local rows are frames 1, 3, 5, the global rows frames 2, 4; peer 9 is in all of them
    out["interleaved"] = Layout().csr([[9, 12], [3, 9], [9]], [1, 3, 5], sel=0).csr([[9], [8, 9, 11]], [2, 4], sel=1).case(40, 6)
    # two runs: the second region starts at an odd element, an odd offset index and an odd src entry
    out["two_runs_odd"] = (Layout().csr([[1, 2], [2]], [0, 1], sel=0).pad(off=0, peers=0, src=(1, 0))
                           .csr([[2, 5, 6], [], [1, 2]], [4, 5, 7], sel=0).pad(off=1, peers=2, src=(0, 3))
                           .csr([[6], [2, 6]], [3, 6], sel=1).case(8, 8))
    assert out["two_runs_odd"].regions["peers_at"][1] % 2 == 1 and out["two_runs_odd"].regions["off_at"][1] % 2 == 1
    # cut: the route call's buffer ended in the middle of row 2, and before row 0's end
    out["cut_mid_row"] = Layout().csr(rows5, [3, 4, 5, 6, 7], capacity=4).csr([[5, 6], [7]], [1, 2], sel=1).case(40, 8)
    out["cut_first_row"] = Layout().csr([[4, 5, 6], [7, 8]], [0, 1], capacity=1).pad(peers=3).csr([[5]], [2]).case(40, 3)
    out["cut_to_zero"] = Layout().csr(rows5, [3, 4, 5, 6, 7], capacity=0).csr([[5]], [2]).case(40, 8)
    # padded: capacity far beyond the pairs; the padding holds a valid, connected peer id
    out["padded"] = Layout().csr(rows5, [0, 1, 2, 3, 4], capacity=700).csr([[1], [1, 2]], [5, 6], sel=1, capacity=300).case(40, 7)
    # unit rows with a frame_base behind the 5 received frames: heartbeat echoes, say
    out["unit_frame_base"] = Layout().csr(rows5, [0, 1, 2, 3, 4]).unit([9, 0, 9], base=5).case(40, 8)
    out["unit_with_src"] = Layout().unit([4, 4, 6], frames=[2, 0, 1], sel=1, base=10).unit([4, 6], n_rows=9, capacity=2).case(8, 13)
    out["unit_fewer_rows"] = Layout().unit([4, 5, 6, 7], n_rows=2).case(8, 4)
    out["repeated_peer"] = Layout().csr([[5, 5, 5, 7, 5], [], [7, 7], [5]], [3, 2, 1, 0]).case(40, 4)
    out["same_frame_twice"] = Layout().csr([[1, 2], [2]], [3, 3]).csr([[2, 3]], [3], sel=1).unit([2], base=3).case(8, 4)
    out["src_out_of_range"] = Layout().csr(rows5, [0, 2, 9, U32_MAX, 8]).case(40, 9)
    out["frame_sum_past_u32"] = Layout().csr([[1], [2]], [5, U32_MAX], base=U32_MAX).unit([3], base=2).case(8, 3)
    out["src_descending"] = Layout().csr(rows5, [4, 3, 2, 1, 0]).case(40, 5)
    conn = np.zeros(2, np.uint32)
    conn[0], conn[1] = 0x55555555, 0xFFFFFF55   # bits past n_peers = 40 set: ids 40 .. 63 stay dropped
    out["connected_half"] = Layout().csr([list(range(64))] * 2, [1, 0]).case(40, 2, conn)
    out["peers_out_of_range"] = Layout().csr([[39, 40, 41, U32_MAX], [U32_MAX - 1, 0]], [0, 1]).case(40, 2)
    out["empty_regions_between"] = (Layout().csr([], capacity=0).csr([[1]], [0]).csr([[], []], [1, 1], capacity=0)
                                    .unit([], n_rows=0).csr([[2, 1]], [1]).csr([], capacity=0).case(8, 2))
    # ---- the key widths
    L = mixed_layout()
    def bitmap(n_peers):     # peers 0 .. 7 and the largest two connected, the rest drawn
        words = _bitmap(rng, n_peers, 0.8)
        words[0] |= 0xFF
        words[-1] |= 0xFFFFFFFF
        return words

    out["mixed_32bit"] = L.case(300, 400, bitmap(300))                       # 9 + 9 bits
    out["mixed_64bit"] = L.case((1 << 20) + 3, 5000, bitmap((1 << 20) + 3))  # 21 + 13 = 34 bits
    edge = lambda: Layout().csr([[65534, 0, 65535], [65534, 65536]], [65535, 0]).unit([65534, 1], base=65534, n_rows=3, capacity=3)
    out["exactly_32_bits"] = edge().case(65535, 65536)      # 16 + 16
    out["exactly_33_bits"] = edge().case(65536, 65536)      # 17 + 16
    out["frames_2_pow_32"] = Layout().csr([[1, 0]], [U32_MAX - 1]).unit([1], base=U32_MAX).unit([1], base=0).case(2, U32_MAX)
    # ---- hostile offsets: unspecified but well formed
    s_rows = _random_rows(rng, 60, 300, (0, 1, 2, 3, 5, 12))
    n = sum(map(len, s_rows))
    asc = np.concatenate([[0], np.cumsum([len(r) for r in s_rows])])
    out["offsets_all_ones"] = Layout().csr([[1, 2]], [0]).csr(s_rows, np.arange(60), offsets=[U32_MAX] * 61, capacity=n).case(300, 62)
    for name, o in (("hostile_descending", asc[::-1].tolist()),
                    ("hostile_junk", rng.integers(0, 2 * n, size=61).tolist()),
                    ("hostile_one_pair", asc[:20].tolist() + [3] + asc[21:].tolist())):
        out[name] = Layout().csr([[1, 2]], [0]).csr(s_rows, np.arange(60), offsets=o, capacity=n).csr([[3]], [61], sel=1).case(
            300, 62, kind="hostile")
    return out


def exact_names():
    return sorted(n for n, c in cases().items() if c.kind == "exact")


def hostile_names():
    return sorted(n for n, c in cases().items() if c.kind == "hostile")


def _with(c, **kw):
    return SimpleNamespace(**{**vars(c), **kw})


def _regions(c, k, **fields):
    reg = c.regions.copy()
    for f, v in fields.items():
        reg[f][k] = v
    return reg


@functools.lru_cache(maxsize=None)
def invalid_cases():
    """name -> a case the C ABI refuses with WQ_E_INVALID (tick_sends_np: ValueError)."""
    c = cases()["two_runs_odd"]
    n_off, n_p, n_l = len(c.offsets), len(c.peers), len(c.srcs[0])
    assert int(np.argmax(c.regions["off_at"])) == 2 and int(np.argmax(c.regions["peers_at"])) == 2   # nothing lies behind region 2
    return {
        "n_peers_all_ones": _with(c, n_peers=U32_MAX),
        "n_elems_too_small": _with(c, n_elems=c.n_elems - 1),
        "n_elems_too_large": _with(c, n_elems=c.n_elems + 1),
        "pad_set": _with(c, regions=_regions(c, 1, pad_=1)),
        "src_sel_2": _with(c, regions=_regions(c, 2, src_sel=2)),
        "offsets_one_short": _with(c, offsets=c.offsets[:n_off - 1]),
        "off_at_near_2_pow_32": _with(c, regions=_regions(c, 0, off_at=U32_MAX - 1)),
        "peers_one_short": _with(c, peers=c.peers[:n_p - 1], n_pairs=n_p - 1),
        "peers_at_near_2_pow_32": _with(c, regions=_regions(c, 0, peers_at=U32_MAX)),
        "src_one_short": _with(c, srcs=(c.srcs[0][:n_l - 1], c.srcs[1])),
        "src_at_near_2_pow_32": _with(c, regions=_regions(c, 2, src_at=U32_MAX - 1)),
        "src_array_missing": _with(c, srcs=(c.srcs[0], None)),
        # every region lies inside the n_pairs the call claims; nothing is launched, so nothing reads them
        "capacities_past_u32": _with(c, regions=np.array([abi.send_region(n_rows=1, capacity=1 << 31)] * 2, abi.SEND_REGION_DTYPE),
                                     n_pairs=1 << 31, n_elems=1 << 32),
    }


@functools.lru_cache(maxsize=None)
def want(name):
    """tick_sends_np of an exact case, computed once: (peer_offsets, frames, counters)."""
    c = cases()[name]
    po, frames, cnt = interest.tick_sends_np(c.regions, c.offsets, c.peers, c.srcs, c.n_peers, c.n_frames, c.connected)
    return _readonly(po), _readonly(frames), cnt


def well_formed(c, po, frames, counters=None):
    """What include/wq_router.h promises whatever the offsets hold. po: peer_offsets[n_peers + 1], frames:
    frames_out[n_elems]."""
    assert len(po) == c.n_peers + 1 and len(frames) == c.n_elems
    assert int(po[0]) == 0 and (np.diff(po.astype(np.int64)) >= 0).all()
    kept = int(po[-1])
    assert kept <= c.n_elems
    assert (frames[:kept] < c.n_frames).all()
    assert not frames[kept:].any()                       # behind the kept ones: zeros
    for p in np.flatnonzero(np.diff(po.astype(np.int64)) > 1)[:2000]:
        assert (np.diff(frames[int(po[p]):int(po[p + 1])].astype(np.int64)) >= 0).all(), ("a list descends", p)
    if counters is not None:
        assert counters["n_regions"] == len(c.regions) and counters["n_elems"] == c.n_elems
        assert counters["n_kept"] == kept
        assert counters["n_covered"] == kept + counters["n_drop_peer"] + counters["n_drop_frame"] <= c.n_elems
        assert bool(counters["error"] & abi.SENDS_ERROR_FRAME) == bool(counters["n_drop_frame"])


def brute(c):
    """Element by element in Python ints: (peer_offsets, frames, counters)."""
    off, peers = c.offsets.tolist(), c.peers.tolist()
    src = [s.tolist() if s is not None else [] for s in c.srcs]
    words = c.connected.tolist() if c.connected is not None else None
    sends, cnt = [], dict(n_regions=len(c.regions), n_elems=0, n_covered=0, n_kept=0, n_drop_peer=0, n_drop_frame=0, error=0)
    for g in c.regions.tolist():
        off_at, peers_at, n_rows, cap, src_at, base, sel, _ = g
        cnt["n_elems"] += cap
        if off_at != UNIT and any(off[off_at + r + 1] > cap for r in range(n_rows)):
            cnt["error"] |= abi.SENDS_ERROR_ROWS
        for e in range(cap):
            if off_at == UNIT:
                row = e if e < n_rows else None
            else:
                row = next((r for r in range(n_rows) if min(off[off_at + r], cap) <= e < min(off[off_at + r + 1], cap)), None)
            if row is None:
                continue
            cnt["n_covered"] += 1
            frame = base + (row if src_at == NO_SRC else src[sel][src_at + row])
            p = peers[peers_at + e]
            if frame >= c.n_frames:
                cnt["n_drop_frame"] += 1
                cnt["error"] |= abi.SENDS_ERROR_FRAME
            elif p >= c.n_peers or (words is not None and not (words[p // 32] >> (p % 32)) & 1):
                cnt["n_drop_peer"] += 1
            else:
                sends.append((p, frame, len(sends)))
    sends.sort()
    cnt["n_kept"] = len(sends)
    po = np.searchsorted(np.array([s[0] for s in sends], np.int64), np.arange(c.n_peers + 1), side="left")
    return po.astype(np.uint32), np.array([s[1] for s in sends], dtype=np.uint32), cnt


def check_against_brute(c, got):
    po, frames, cnt = got
    b_po, b_frames, b_cnt = brute(c)
    assert po.dtype == np.uint32 and frames.dtype == np.uint32
    assert po.tobytes() == b_po.tobytes() and frames.tobytes() == b_frames.tobytes()
    assert cnt == b_cnt
    well_formed(c, po, np.concatenate([frames, np.zeros(c.n_elems - len(frames), np.uint32)]), cnt)


@pytest.mark.parametrize("name", exact_names())
def test_definition_matches_the_restatement(name):
    check_against_brute(cases()[name], want(name))


def random_layout(seed):
    rng = np.random.default_rng(1000 + seed)
    n_peers, n_frames = int(rng.choice([1, 2, 7, 33, 64])), int(rng.choice([1, 2, 5, 9, 40]))
    L = Layout()
    for _ in range(int(rng.integers(0, 6))):
        n = int(rng.integers(0, 7))
        sel = int(rng.integers(0, 2))
        frames = rng.integers(0, n_frames + 2, size=n).tolist() if rng.random() < 0.8 else None
        base = int(rng.integers(0, 3)) if rng.random() < 0.3 else 0
        if rng.random() < 0.25:
            L.unit(rng.integers(0, n_peers + 3, size=n).tolist(), frames, sel, base,
                   n_rows=n if frames is not None or rng.random() < 0.5 else n + 2, capacity=int(rng.integers(0, n + 3)))
        else:
            rows = _random_rows(rng, n, n_peers + 3, (0, 0, 1, 2, 3, 4))
            pairs = sum(map(len, rows))
            L.csr(rows, frames, sel, base, capacity=int(rng.choice([pairs, pairs, int(rng.integers(0, pairs + 1)), pairs + 5])))
        L.pad(off=int(rng.integers(0, 3)), peers=int(rng.integers(0, 3)), src=(int(rng.integers(0, 2)), int(rng.integers(0, 2))))
    return L.case(n_peers, n_frames, _bitmap(rng, n_peers, 0.7) if rng.random() < 0.5 else None)


def test_200_random_small_layouts():
    kept = cut = dropped = 0
    for seed in range(200):
        c = random_layout(seed)
        got = interest.tick_sends_np(c.regions, c.offsets, c.peers, c.srcs, c.n_peers, c.n_frames, c.connected)
        check_against_brute(c, got)
        kept += got[2]["n_kept"]
        cut += bool(got[2]["error"] & abi.SENDS_ERROR_ROWS)
        dropped += got[2]["n_drop_frame"] > 0 and got[2]["n_drop_peer"] > 0
    assert kept > 500 and cut > 20 and dropped > 20


def test_case_conditions():
    """What the named cases are there for, from the definition alone."""
    c = cases()
    for name in ("no_regions", "no_peers", "no_frames", "no_elems"):
        assert not want(name)[0].any() and len(want(name)[1]) == 0
    assert want("no_frames")[2]["n_drop_frame"] == 9 and want("no_peers")[2]["n_drop_peer"] == 9
    # one identity region is the transpose of that CSR
    i = c["identity"]
    po, rows = interest.peer_major_np(i.offsets, i.peers, i.n_peers, i.connected)
    assert want("identity")[0].tobytes() == po.tobytes() and want("identity")[1].tobytes() == rows.tobytes()
    assert 0 < len(rows) < len(i.peers)
    po, f, _ = want("interleaved")
    assert f[int(po[9]):int(po[10])].tolist() == [1, 2, 3, 4, 5]
    po, f, _ = want("two_runs_odd")
    assert f[int(po[2]):int(po[3])].tolist() == [0, 1, 4, 6, 7] and f[int(po[6]):int(po[7])].tolist() == [3, 4, 6]
    for name in ("cut_mid_row", "cut_first_row", "cut_to_zero"):
        assert want(name)[2]["error"] == abi.SENDS_ERROR_ROWS and want(name)[2]["n_kept"] > 0
    assert want("cut_mid_row")[2]["n_covered"] == 4 + 3
    pad = want("padded")
    assert pad[2]["n_elems"] == 1000 and pad[2]["n_covered"] == 9 + 3 and pad[2]["error"] == 0
    po, f, _ = want("unit_frame_base")
    assert f[int(po[9]):int(po[10])].tolist() == [0, 2, 2, 4, 5, 7] and f[int(po[0]):int(po[1])].tolist() == [3, 6]
    po, f, _ = want("repeated_peer")
    assert f[int(po[5]):int(po[6])].tolist() == [0, 3, 3, 3, 3] and f[int(po[7]):int(po[8])].tolist() == [1, 1, 3]
    po, f, cnt = want("same_frame_twice")
    assert f[int(po[2]):int(po[3])].tolist() == [3, 3, 3, 3] and cnt["error"] == 0
    assert want("src_out_of_range")[2]["n_drop_frame"] == 4 and want("src_out_of_range")[2]["error"] == abi.SENDS_ERROR_FRAME
    assert want("frame_sum_past_u32")[2]["n_drop_frame"] == 2 and want("frame_sum_past_u32")[1].tolist() == [2]
    assert want("connected_half")[2]["n_kept"] == 2 * 20 and want("connected_half")[2]["n_drop_peer"] == 2 * 44
    assert want("peers_out_of_range")[2]["n_kept"] == 2
    # the key widths: 18, 34, 32 and 33 bits; the wide key keeps what the narrow one's bounds drop
    bits = lambda n: max(c[n].n_peers.bit_length(), 1) + max(c[n].n_frames - 1, 0).bit_length()
    assert [bits(n) for n in ("mixed_32bit", "mixed_64bit", "exactly_32_bits", "exactly_33_bits", "frames_2_pow_32")] == \
        [18, 34, 32, 33, 34]
    m32, m64 = want("mixed_32bit"), want("mixed_64bit")
    assert m32[2]["n_drop_frame"] == 4 and m64[2]["n_drop_frame"] == 1 and m64[2]["n_kept"] > 500
    assert int(m64[0][(1 << 20) + 3]) - int(m64[0][(1 << 20) + 2]) == 1 and 4999 in m64[1] and 4998 in m64[1]
    both = sum(1 for a, b in zip(c["mixed_32bit"].regions[:-1], c["mixed_32bit"].regions[1:])
               if a["src_sel"] == 0 and b["src_sel"] == 1 and a["off_at"] != UNIT and b["off_at"] != UNIT)
    assert both > 10                                       # runs with a local and a global region
    po, f, _ = want("exactly_32_bits")
    assert f[int(po[65534]):int(po[65535])].tolist() == [0, 65534, 65535] and int(po[65535]) == 5
    po, f, _ = want("exactly_33_bits")
    assert f[int(po[65535]):int(po[65536])].tolist() == [65535] and int(po[65536]) == 6
    assert want("frames_2_pow_32")[1].tolist() == [U32_MAX - 1, 0, U32_MAX - 1] and want("frames_2_pow_32")[2]["n_drop_frame"] == 1


def test_hostile_cases_are_what_they_say():
    for name in hostile_names():
        c = cases()[name]
        o = c.offsets[int(c.regions["off_at"][1]):][:61].astype(np.int64)
        assert (np.diff(o) < 0).any(), name
        with pytest.raises(ValueError):
            interest.tick_sends_np(c.regions, c.offsets, c.peers, c.srcs, c.n_peers, c.n_frames, c.connected)


@pytest.mark.parametrize("name", sorted(invalid_cases()))
def test_invalid_calls_raise(name):
    c = invalid_cases()[name]
    with pytest.raises(ValueError):
        interest.tick_sends_np(c.regions, c.offsets, c.peers, c.srcs, c.n_peers, c.n_frames, c.connected, n_elems=c.n_elems)
    # the case it was made from is a valid call
    ok = cases()["two_runs_odd"]
    interest.tick_sends_np(ok.regions, ok.offsets, ok.peers, ok.srcs, ok.n_peers, ok.n_frames, ok.connected, n_elems=ok.n_elems)


def test_legal_edges_do_not_raise():
    """A unit-row region with a src, regions with n_rows == 0 or capacity == 0 (their off_at and src_at
    point anywhere), src arrays left out when no region names them."""
    r = np.array([abi.send_region(off_at=12345, peers_at=0, n_rows=0, capacity=2, src_at=999, src_sel=1),
                  abi.send_region(off_at=0, peers_at=2, n_rows=1, capacity=0)], abi.SEND_REGION_DTYPE)
    po, f, cnt = interest.tick_sends_np(r, [0, 1], [1, 1], None, 4, 4)
    assert not po.any() and cnt["n_covered"] == 0 and cnt["error"] == abi.SENDS_ERROR_ROWS


# ---- the stream of the end-to-end test, on the oracle --------------------------------------------------

def oracle_tick_regions(o, disp, per_row=320):
    """The caller's side of a dispatched tick with the C oracle as the table, leaving what
    IngestTick.process leaves: every read run's route results laid into shared offsets / peers, each region
    padded to rows * per_row pairs and begun at a multiple of four. Returns (regions, offsets, peers, the
    read runs with a region of both kinds)."""
    L, both = Layout(), 0
    runs = disp["runs"]
    for a, b in zip(runs[:-1], runs[1:]):
        if a["kind"] == abi.RUN_TABLE:
            o.apply_ops(disp["ops"][a["op_begin"]:b["op_begin"]])
            continue
        both += b["l_begin"] > a["l_begin"] and b["g_begin"] > a["g_begin"]
        for sel, (lo, hi) in enumerate(((int(a["l_begin"]), int(b["l_begin"])), (int(a["g_begin"]), int(b["g_begin"])))):
            if hi <= lo:
                continue
            s = slice(lo, hi)
            if sel == 0:
                offs, peers, _ = o.route(disp["l_pos"][s], disp["l_world"][s], disp["l_sender"][s], disp["l_repl"][s])
            else:
                offs, peers = o.route_global(disp["g_world"][s], disp["g_sender"][s], disp["g_repl"][s])
            assert int(offs[-1]) <= (hi - lo) * per_row
            L.off += [int(x) for x in offs]
            g = abi.send_region(off_at=len(L.off) - len(offs), peers_at=len(L.peers), n_rows=hi - lo, capacity=(hi - lo) * per_row,
                                src_at=lo, src_sel=sel)
            L.peers += peers[:int(offs[-1])].tolist() + [FILL] * ((hi - lo) * per_row - int(offs[-1]))
            L.regions.append(g)
            L.pad(off=-len(L.off) % 4, peers=-len(L.peers) % 4)
    return np.array(L.regions, abi.SEND_REGION_DTYPE).reshape(-1), np.array(L.off, np.uint32), np.array(L.peers, np.uint32), int(both)


def test_the_end_to_end_stream_is_not_trivial():
    """The 6,000-event stream of the GPU's end-to-end test in ticks of 97 and 400 frames, with the oracle as
    the table and the definition as the sends: inverted, the per-peer lists are the sequential reference's
    recipients event by event; read runs with both a local and a global region, and peers whose list draws
    on two regions of one tick, each occur more than 100 times."""
    import uuid

    from oracle import oracle as orc
    from worldql_server_amd import ingest

    from test_ingest_dispatch_host import N_PEERS, all_worlds, check_events, stream, ticks_of, wire
    from tests.seq_reference import SequentialReference
    events = stream(6000, seed=33)
    worlds, peers = all_worlds(), [uuid.UUID(int=k + 1) for k in range(N_PEERS)]
    ref, o = SequentialReference(16), orc.COracle(16)
    nonempty = both_kinds = multi_region_peers = 0
    for chunk in ticks_of(events, (97, 400)):
        data, offsets = wire(chunk)
        dec = ingest.decode_frames_np(data, offsets, worlds, peers)
        disp = ingest.dispatch_np(dec)
        reg, off, prs, both = oracle_tick_regions(o, disp)
        both_kinds += both
        po, frames, cnt = interest.tick_sends_np(reg, off, prs, (disp["l_src"], disp["g_src"]), N_PEERS, len(chunk))
        assert cnt["error"] == 0 and cnt["n_drop_peer"] == 0 and cnt["n_drop_frame"] == 0
        region_of = np.full(len(chunk), -1, np.int64)
        for k, g in enumerate(reg):
            src = disp["l_src"] if g["src_sel"] == 0 else disp["g_src"]
            region_of[src[int(g["src_at"]):int(g["src_at"]) + int(g["n_rows"])]] = k
        res = [[] for _ in chunk]
        po = po.astype(np.int64)
        for p in np.flatnonzero(np.diff(po)):
            mine = frames[po[p]:po[p + 1]]
            assert (np.diff(mine.astype(np.int64)) > 0).all()
            multi_region_peers += len(set(region_of[mine].tolist())) >= 2
            for f in mine.tolist():
                res[f].append(int(p))
        nonempty += check_events(chunk, dec, disp, res, ref, lambda ids: [f"peer-{q}" for q in ids])
    assert nonempty > 500 and both_kinds > 100 and multi_region_peers > 100
