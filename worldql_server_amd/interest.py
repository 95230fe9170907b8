"""Interest changes between two ticks: who entered and who left each row (include/wq_router.h,
wq_csr_diff*; kernels: csrc/wq_csr_diff.hip).

`csr_diff_np` is the host reference and the byte-identical definition of the GPU output;
`clamp_csr_np` is the definition of how the kernels read offsets that do not describe a CSR;
`InterestTracker` is the convenience a server that replicates entities uses: route a tick, get the
observers that entered and left every entity's interest set since the previous tick.

`peer_major_np` is the definition of the per-peer send lists (wq_peer_major_device) and
`peer_budget_np` the definition of the send budgets that follow them (wq_peer_budget_device,
csrc/wq_budget.hip): of every peer's list the min(budget, len) messages nearest to the peer.
`peer_budget_bytes_np` is the definition of the byte budgets (wq_peer_budget_bytes_device): of every
peer's list the nearest messages whose sizes sum to at most the peer's bytes.
`peer_pack_np` is the definition of the send buffers (wq_peer_pack_device, csrc/wq_pack.hip): every
peer's frames in one contiguous byte run, in list order.
`peer_rotate_np` is the definition of the fair share (wq_peer_rotate_device, csrc/wq_rotate.hip): the
budget's output plus, per peer, the cut elements that follow the peer's cursor in cyclic order.
`tick_sends_np` is the definition of the tick sends (wq_tick_sends_device, csrc/wq_sends.hip): one
per-peer list of received frames, ascending, from all the CSR regions a tick's read runs left.
"""
from __future__ import annotations

import numpy as np

from . import abi


def _row_keys(offsets: np.ndarray, peers: np.ndarray):
    """(row << 32 | peer) of every element of a CSR: ascending, because rows are and peers within a
    row are."""
    M = len(offsets) - 1
    counts = np.diff(offsets.astype(np.int64))
    if (counts < 0).any() or (M >= 0 and len(offsets) and int(offsets[0]) != 0):
        raise ValueError("offsets must ascend from 0 (clamp_csr_np makes them)")
    rows = np.repeat(np.arange(M, dtype=np.uint64), counts)
    return rows, (rows << np.uint64(32)) | peers[: int(offsets[-1])].astype(np.uint64)


def _missing(keys: np.ndarray, other: np.ndarray) -> np.ndarray:
    """keys[i] not in other (both ascending and distinct)."""
    if len(other) == 0:
        return np.ones(len(keys), bool)
    at = np.searchsorted(other, keys)
    return other[np.minimum(at, len(other) - 1)] != keys


def _side(rows, keys, other_keys, peers, M):
    keep = _missing(keys, other_keys)
    out_peers = np.ascontiguousarray(peers[: len(keys)][keep], dtype=np.uint32)
    offsets = np.zeros(M + 1, dtype=np.uint32)
    np.cumsum(np.bincount(rows[keep].astype(np.int64), minlength=M)[:M], out=offsets[1:])
    return offsets, out_peers


def csr_diff_np(old_offsets, old_peers, new_offsets, new_peers):
    """(ent_offsets, ent_peers, left_offsets, left_peers) of two CSRs over the same rows, peers
    ascending and distinct within a row: row m of entered = new_m \\ old_m, of left = old_m \\ new_m,
    both ascending. All four arrays are uint32."""
    oo = np.ascontiguousarray(old_offsets, dtype=np.uint32)
    no = np.ascontiguousarray(new_offsets, dtype=np.uint32)
    op = np.ascontiguousarray(old_peers, dtype=np.uint32)
    npr = np.ascontiguousarray(new_peers, dtype=np.uint32)
    if len(oo) != len(no) or len(oo) < 1:
        raise ValueError("both CSRs need offsets[n_rows + 1] over the same rows")
    M = len(oo) - 1
    ro, ko = _row_keys(oo, op)
    rn, kn = _row_keys(no, npr)
    eo, ep = _side(rn, kn, ko, npr, M)
    lo, lp = _side(ro, ko, kn, op, M)
    return eo, ep, lo, lp


def diff_limit(capacity: int) -> int:
    """csr_diff_ops.hpp diff_limit: the elements a side's clamped rows are walked up to."""
    return min((2 * capacity + 63) & ~63, 0xFFFFFFC0)


def clamp_csr_np(offsets, peers, capacity: int | None = None):
    """How wq_csr_diff* reads a CSR whose offsets may not describe one (csr_diff_ops.hpp): row m is
    the part of [offsets[m], offsets[m + 1]) inside [0, capacity), empty when offsets[m + 1] <
    offsets[m]; the rows are walked up to diff_limit(capacity) elements in total. Returns (offsets,
    peers, cut): a valid CSR holding those rows, and whether any row was cut (error bit 0)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint32).astype(np.int64)
    peers = np.ascontiguousarray(peers, dtype=np.uint32)
    cap = len(peers) if capacity is None else int(capacity)
    a = np.minimum(off[:-1], cap)
    b = np.maximum(a, np.minimum(off[1:], cap))
    cut = bool(((off[1:] < off[:-1]) | (off[1:] > cap)).any())
    pre = np.concatenate([[0], np.cumsum(b - a)])
    pre = np.minimum(pre, diff_limit(cap))
    n = np.diff(pre)
    idx = np.repeat(a - pre[:-1], n) + np.arange(int(pre[-1]), dtype=np.int64)
    return pre.astype(np.uint32), np.ascontiguousarray(peers[idx], dtype=np.uint32), cut


def peer_major_np(offsets, peers, n_peers: int, connected=None, capacity: int | None = None):
    """The transpose of a CSR: (peer_offsets[n_peers + 1], rows) — per peer the rows that hold it,
    ascending; the definition of what wq_peer_major_device writes for ascending offsets.

    Row m is the part of [offsets[m], offsets[m + 1]) inside [0, capacity) (capacity: the element
    count of `peers`, the default — a cut tick's offsets reach past it, a padded buffer's end before
    it; elements no row covers belong to nobody). A pair is kept when its peer is below n_peers and,
    with `connected` (u32 words, bit p % 32 of word p // 32), its bit is set. The kept pairs are
    sorted stably by peer: a peer's rows ascend, and a peer repeated within a row keeps its repeats.
    `offsets` of length 0 or 1 is a CSR without rows."""
    off = np.ascontiguousarray(offsets, dtype=np.uint32).astype(np.int64)
    peers = np.ascontiguousarray(peers, dtype=np.uint32)
    cap = len(peers) if capacity is None else int(capacity)
    if cap > len(peers):
        raise ValueError("capacity is the element count of peers: it cannot exceed len(peers)")
    n_peers = int(n_peers)
    M = max(len(off) - 1, 0)
    if M and (np.diff(off) < 0).any():
        raise ValueError("offsets must ascend (for others the kernel's result is unspecified)")
    a = np.minimum(off[:M], cap)
    b = np.minimum(off[1:M + 1], cap)
    n = b - a
    total = int(n.sum())
    rows = np.repeat(np.arange(M, dtype=np.uint32), n)
    idx = np.repeat(a - (np.cumsum(n) - n), n) + np.arange(total, dtype=np.int64)
    p = peers[idx]
    keep = p < n_peers
    if connected is not None:
        keep &= _connected_bits(p, keep, connected)
    p, rows = p[keep], rows[keep]
    order = np.argsort(p, kind="stable")
    po = np.zeros(n_peers + 1, dtype=np.uint32)
    np.cumsum(np.bincount(p.astype(np.int64), minlength=n_peers)[:n_peers], out=po[1:])
    return po, np.ascontiguousarray(rows[order], dtype=np.uint32)


def _connected_bits(p, keep, connected):
    """Of the peers p (kept so far where `keep`), which have their bit set in the bitmap's u32 words."""
    words = np.ascontiguousarray(connected, dtype=np.uint32)
    q = np.where(keep, p, 0).astype(np.int64)
    if keep.any() and int(q.max()) >> 5 >= len(words):
        raise ValueError("connected needs ceil(n_peers / 32) words")
    if not len(words):
        return np.zeros(len(p), bool)
    return ((words[q >> 5] >> (q & 31).astype(np.uint32)) & np.uint32(1)) == 1


def tick_sends_check(regions, n_offsets: int, n_pairs: int, n_src, n_peers: int, n_elems: int | None = None) -> int:
    """The checks wq_tick_sends_device refuses a call by (WQ_E_INVALID), as ValueError; returns the sum
    of the capacities."""
    if int(n_peers) >= 0xFFFFFFFF or int(n_peers) < 0:
        raise ValueError("n_peers must be < 2^32 - 1")
    total = 0
    for g in regions:
        n_rows, cap = int(g["n_rows"]), int(g["capacity"])
        if int(g["pad_"]) or int(g["src_sel"]) > 1:
            raise ValueError("a region with pad_ != 0 or src_sel > 1")
        if n_rows and int(g["off_at"]) != abi.SEND_UNIT_ROWS and int(g["off_at"]) + n_rows + 1 > n_offsets:
            raise ValueError("a region reaches outside the offsets")
        if int(g["peers_at"]) + cap > n_pairs:
            raise ValueError("a region reaches outside the peers")
        if n_rows and int(g["src_at"]) != abi.SEND_NO_SRC and int(g["src_at"]) + n_rows > n_src[int(g["src_sel"])]:
            raise ValueError("a region reaches outside its src array")
        total += cap
        if total > 0xFFFFFFFF:
            raise ValueError("the capacities sum to more than 2^32 - 1")
    if n_elems is not None and int(n_elems) != total:
        raise ValueError("n_elems is not the sum of the regions' capacities")
    return total


def tick_sends_np(regions, offsets, peers, srcs, n_peers: int, n_frames: int, connected=None, n_elems: int | None = None):
    """One per-peer frame list from all of a tick's regions: (peer_offsets[n_peers + 1], frames,
    counters) — the definition of what wq_tick_sends_device writes for ascending offsets.

    regions: abi.SEND_REGION_DTYPE rows. The element space is the regions' [0, capacity) laid end to end.
    Inside a region the rows are peer_major_np's with capacity = the region's, on its own n_rows + 1
    offsets from off_at (abi.SEND_UNIT_ROWS: row r is element r, r < min(n_rows, capacity)); the element
    of row r has the frame frame_base + (srcs[src_sel][src_at + r], or r with abi.SEND_NO_SRC) and the
    peer peers[peers_at + element]. A covered element is dropped when its frame is >= n_frames
    (n_drop_frame, error bit 1), else when its peer is >= n_peers or not in `connected` (n_drop_peer). The
    kept ones are sorted stably by (peer, frame). A row that ends past its region's capacity sets error
    bit 0. srcs: (l_src, g_src), either may be None. Raises ValueError where the C call returns
    WQ_E_INVALID, and for offsets that descend (the kernel's result is then unspecified)."""
    reg = np.ascontiguousarray(regions, dtype=abi.SEND_REGION_DTYPE).reshape(-1)
    off = np.ascontiguousarray(offsets if offsets is not None else [], dtype=np.uint32).astype(np.int64)
    peers = np.ascontiguousarray(peers if peers is not None else [], dtype=np.uint32)
    src = [np.ascontiguousarray(s if s is not None else [], dtype=np.uint32).astype(np.int64) for s in (tuple(srcs or ()) + (None, None))[:2]]
    n_peers, n_frames = int(n_peers), int(n_frames)
    total = tick_sends_check(reg, len(off), len(peers), [len(s) for s in src], n_peers, n_elems)
    error, n_covered = 0, 0
    ps, fs = [np.zeros(0, np.uint32)], [np.zeros(0, np.int64)]
    for g in reg:
        M, cap, base = int(g["n_rows"]), int(g["capacity"]), int(g["frame_base"])
        if int(g["off_at"]) == abi.SEND_UNIT_ROWS:
            rows = np.arange(min(M, cap), dtype=np.int64)
            idx = rows
        else:
            o = off[int(g["off_at"]):int(g["off_at"]) + M + 1] if M else np.zeros(1, np.int64)
            if (np.diff(o) < 0).any():
                raise ValueError("offsets must ascend (for others the kernel's result is unspecified)")
            if (o[1:] > cap).any():
                error |= abi.SENDS_ERROR_ROWS
            a, b = np.minimum(o[:M], cap), np.minimum(o[1:M + 1], cap)
            n = b - a
            rows = np.repeat(np.arange(M, dtype=np.int64), n)
            idx = np.repeat(a - (np.cumsum(n) - n), n) + np.arange(int(n.sum()), dtype=np.int64)
        n_covered += len(rows)
        ps.append(peers[int(g["peers_at"]) + idx])
        fs.append(base + (rows if int(g["src_at"]) == abi.SEND_NO_SRC else src[int(g["src_sel"])][int(g["src_at"]) + rows]))
    p, f = np.concatenate(ps), np.concatenate(fs)
    in_range = f < n_frames
    if not in_range.all():
        error |= abi.SENDS_ERROR_FRAME
    keep = in_range & (p < n_peers)
    if connected is not None:
        keep &= _connected_bits(p, keep, connected)
    n_kept = int(keep.sum())
    p, f = p[keep], f[keep]
    order = np.lexsort((f, p))
    po = np.zeros(n_peers + 1, dtype=np.uint32)
    np.cumsum(np.bincount(p.astype(np.int64), minlength=n_peers)[:n_peers], out=po[1:])
    n_drop_frame = int((~in_range).sum())
    counters = dict(n_regions=len(reg), n_elems=total, n_covered=n_covered, n_kept=n_kept,
                    n_drop_peer=n_covered - n_kept - n_drop_frame, n_drop_frame=n_drop_frame, error=error)
    return po, np.ascontiguousarray(f[order], dtype=np.uint32), counters


def budget_keys_np(msgs, msg_pos, peer_pos, p: int):
    """The keys of row p's elements `msgs` (message indices): the radius filter's f64 squared distance
    (dx*dx + dy*dy) + dz*dz, left to right; +inf for NaN, for a message index >= len(msg_pos) and for a
    peer without a position."""
    msgs = np.asarray(msgs, dtype=np.int64)
    d2 = np.full(len(msgs), np.inf, dtype=np.float64)
    if p >= len(peer_pos) or not len(msgs):
        return d2
    ok = msgs < len(msg_pos)
    with np.errstate(over="ignore", invalid="ignore"):
        d = msg_pos[msgs[ok]] - peer_pos[p][None, :]
        v = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    d2[ok] = np.where(np.isnan(v), np.inf, v)
    return d2


def peer_budget_np(peer_offsets, msgs, msg_pos, peer_pos, k=None, budget=None):
    """Send budgets, the definition of what wq_peer_budget_device writes: of every row of the
    peer-major CSR (peer_offsets[n_peers + 1], msgs[n_in]) the min(B_p, len_p) elements nearest to
    the peer, in input order. Returns (out_offsets[n_peers + 1], out_msgs[n_kept], counters) with
    counters a dict of n_in, n_kept, rows_cut, error.

    Row p is the part of [peer_offsets[p], peer_offsets[p + 1]) inside [0, n_in), empty when the
    offsets descend; the rows are walked up to n_in elements in total (only offsets that descend get
    there: the row that passes n_in is cut, the ones behind it are empty; error bit 0). B_p is
    budget[p], or k for everyone. Elements order by (d2, position in the row), d2 from
    budget_keys_np. error bit 1: a message index >= len(msg_pos). Row by row, for clarity."""
    off = np.ascontiguousarray(peer_offsets, dtype=np.uint32).astype(np.int64)
    msgs = np.ascontiguousarray(msgs, dtype=np.uint32)
    msg_pos = np.ascontiguousarray(msg_pos, dtype=np.float64).reshape(-1, 3)
    peer_pos = np.ascontiguousarray(peer_pos, dtype=np.float64).reshape(-1, 3)
    n_in, n_peers = len(msgs), max(len(off) - 1, 0)
    if budget is None and k is None:
        raise ValueError("give k or a per-peer budget")
    out_off = np.zeros(n_peers + 1, dtype=np.uint32)
    out, walked, rows_cut, error = [], 0, 0, 0
    for p in range(n_peers):
        a, b = min(off[p], n_in), min(off[p + 1], n_in)
        b = max(a, b)
        if off[p] > off[p + 1] or off[p + 1] > n_in:
            error |= 1
        n = min(b - a, n_in - walked)
        if n != b - a:
            error |= 1
        walked += n
        row = msgs[a:a + n]
        B = int(budget[p]) if budget is not None else int(k)
        if (row.astype(np.int64) >= len(msg_pos)).any():
            error |= 2
        if n > B:
            rows_cut += 1
            d2 = budget_keys_np(row, msg_pos, peer_pos, p)
            order = np.lexsort((np.arange(n), d2))      # by d2, then position
            row = row[np.sort(order[:B])]               # the B nearest, back in input order
        out.append(row)
        out_off[p + 1] = out_off[p] + len(row)
    out_msgs = np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)
    return out_off, out_msgs, dict(n_in=walked, n_kept=int(out_off[-1]), rows_cut=rows_cut, error=error)


def frame_sizes(offsets):
    """The u32 size of every frame from wq_serialize_messages' u64 offsets[n + 1], the msg_size array of
    the byte budgets. Raises on a frame of 2^32 bytes or more (the codec's own limit is 2 GiB)."""
    sizes = np.diff(np.ascontiguousarray(offsets, dtype=np.uint64))
    if len(sizes) and int(sizes.max()) >= 1 << 32:
        raise ValueError("a frame of 2^32 bytes or more has no u32 size")
    return sizes.astype(np.uint32)


def peer_budget_bytes_np(peer_offsets, msgs, msg_pos, msg_size, peer_pos, w=None, budget=None):
    """Byte budgets, the definition of what wq_peer_budget_bytes_device writes: an element of row p is
    kept iff the sizes of all elements of row p at or before it in the (d2, position) order, its own
    included, sum to at most W_p (budget[p], or w for everyone), so each row keeps a prefix of that
    order; the kept elements stay in input order. Returns (out_offsets[n_peers + 1], out_msgs[n_kept],
    out_bytes[n_peers] u64, counters) with counters a dict of n_in, n_kept, bytes_in, bytes_kept,
    rows_cut, error.

    Rows, keys and the error bits are peer_budget_np's. The size of an element with message m is
    msg_size[m], and 0 when m >= len(msg_pos). The sums are Python ints. Row by row, for clarity."""
    off = np.ascontiguousarray(peer_offsets, dtype=np.uint32).astype(np.int64)
    msgs = np.ascontiguousarray(msgs, dtype=np.uint32)
    msg_pos = np.ascontiguousarray(msg_pos, dtype=np.float64).reshape(-1, 3)
    msg_size = np.ascontiguousarray(msg_size, dtype=np.uint32)
    peer_pos = np.ascontiguousarray(peer_pos, dtype=np.float64).reshape(-1, 3)
    n_in, n_peers, n_msgs = len(msgs), max(len(off) - 1, 0), len(msg_pos)
    if budget is None and w is None:
        raise ValueError("give w or a per-peer byte budget")
    if len(msg_size) < n_msgs:
        raise ValueError("msg_size needs an entry per message")
    out_off = np.zeros(n_peers + 1, dtype=np.uint32)
    out_bytes = np.zeros(n_peers, dtype=np.uint64)
    out, walked, rows_cut, error, bytes_in = [], 0, 0, 0, 0
    for p in range(n_peers):
        a, b = min(off[p], n_in), min(off[p + 1], n_in)
        b = max(a, b)
        if off[p] > off[p + 1] or off[p + 1] > n_in:
            error |= 1
        n = min(b - a, n_in - walked)
        if n != b - a:
            error |= 1
        walked += n
        row = msgs[a:a + n]
        W = int(budget[p]) if budget is not None else int(w)
        if (row.astype(np.int64) >= n_msgs).any():
            error |= 2
        sizes = [int(msg_size[m]) if m < n_msgs else 0 for m in row.tolist()]
        bytes_in += sum(sizes)
        d2 = budget_keys_np(row, msg_pos, peer_pos, p)
        order = np.lexsort((np.arange(n), d2)).tolist()    # by d2, then position
        kept, running = [], 0
        for i in order:
            running += sizes[i]
            if running > W:
                break                                       # everything behind it has a larger sum
            kept.append(i)
        if len(kept) < n:
            rows_cut += 1
        kept.sort()                                         # back in input order
        out.append(row[kept] if kept else row[:0])
        out_off[p + 1] = out_off[p] + len(kept)
        out_bytes[p] = sum(sizes[i] for i in kept)
    out_msgs = np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)
    return out_off, out_msgs, out_bytes, dict(n_in=walked, n_kept=int(out_off[-1]), bytes_in=bytes_in,
                                              bytes_kept=int(sum(int(v) for v in out_bytes)), rows_cut=rows_cut,
                                              error=error)


def _walk_rows(offsets, n):
    """The budgets' rows of a CSR over an array of n elements: per row (start, length) after the clamp
    to [0, n) and the walk of at most n elements in total; (rows, walked, error bit 0)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint32).astype(np.int64)
    rows, walked, error = [], 0, 0
    for p in range(max(len(off) - 1, 0)):
        a, b = min(off[p], n), min(off[p + 1], n)
        b = max(a, b)
        if off[p] > off[p + 1] or off[p + 1] > n:
            error |= 1
        ln = min(b - a, n - walked)
        if ln != b - a:
            error |= 1
        walked += ln
        rows.append((int(a), int(ln)))
    return rows, walked, error


def peer_rotate_np(peer_offsets, msgs, kept_offsets, kept_msgs, cursor, r=None, extra=None, msg_size=None,
                   v=None, extra_bytes=None):
    """The fair share, the definition of what wq_peer_rotate_device writes. The full peer-major CSR
    (peer_offsets[n_peers + 1], msgs[n_in]) and a kept CSR over the same peers (either budget's output
    on it); cursor[n_peers] u32, a message index per peer, read and written IN PLACE. Returns
    (out_offsets[n_peers + 1], out_msgs[n_out], out_bytes[n_peers] u64 or None without sizes, counters)
    with counters a dict of n_in, n_kept_in, n_chosen, n_out, bytes_chosen, bytes_out, rows_rotated,
    rows_behind, error.

    Rows of both CSRs are peer_budget_np's (error bit 0). For rows that ascend: a value that occurs cf
    times in full row p and ck times in kept row p has its first min(cf, ck) occurrences kept, the others
    cut; a kept element without a partner is ignored (error bit 2). The cut elements are numbered
    q = 0, 1, ... from the first index whose message index is greater than cursor[p] to the row's end,
    then from the row's start. Chosen is the longest prefix of that order with q < R_p (extra[p], or r)
    and, with msg_size, a running size sum <= V_p (extra_bytes[p], or v); q = 0 is always chosen when
    R_p >= 1. The size of message m is msg_size[m], and 0 when m >= len(msg_size) (error bit 1). Output
    row p: the kept and the chosen elements in the full row's order; cursor[p]: the message index of the
    chosen element with the largest q, unchanged when there is none. The sums are Python ints. Row by
    row, for clarity."""
    import bisect
    from collections import Counter
    msgs = np.ascontiguousarray(msgs, dtype=np.uint32)
    kept_msgs = np.ascontiguousarray(kept_msgs, dtype=np.uint32)
    n_in, n_kin = len(msgs), len(kept_msgs)
    rows, walked, error = _walk_rows(peer_offsets, n_in)
    krows, _, kerror = _walk_rows(kept_offsets, n_kin)
    error |= kerror
    n_peers = len(rows)
    if len(krows) != n_peers or len(cursor) < n_peers:
        raise ValueError("the kept CSR and the cursors cover the full CSR's peers")
    if cursor.dtype != np.uint32:
        raise ValueError("cursor is a u32 array, written in place")
    if extra is None and r is None:
        raise ValueError("give r or a per-peer share")
    sizes_on = msg_size is not None
    if sizes_on:
        msg_size = np.ascontiguousarray(msg_size, dtype=np.uint32)
        if extra_bytes is None and v is None:
            raise ValueError("with msg_size give v or a per-peer byte share")
    n_msgs = len(msg_size) if sizes_on else 0
    out_off = np.zeros(n_peers + 1, dtype=np.uint32)
    out_bytes = np.zeros(n_peers, dtype=np.uint64) if sizes_on else None
    out, matched, n_chosen, bytes_chosen, bytes_out, rows_rotated, rows_behind = [], 0, 0, 0, 0, 0, 0
    for p in range(n_peers):
        (a, n), (ka, kn) = rows[p], krows[p]
        row = msgs[a:a + n].tolist()
        have = Counter(kept_msgs[ka:ka + kn].tolist())
        size = [0] * n
        if sizes_on:
            if any(m >= n_msgs for m in row):
                error |= 2
            size = [int(msg_size[m]) if m < n_msgs else 0 for m in row]
        seen, is_cut = Counter(), []
        for m in row:
            is_cut.append(seen[m] >= have[m])
            seen[m] += 1
        n_match = n - sum(is_cut)
        matched += n_match
        if n_match != kn:
            error |= 4
        pos = bisect.bisect_right(row, int(cursor[p]))
        order = [i for i in range(pos, n) if is_cut[i]] + [i for i in range(pos) if is_cut[i]]
        R = int(extra[p]) if extra is not None else int(r)
        V = (int(extra_bytes[p]) if extra_bytes is not None else int(v)) if sizes_on else 0
        chosen, running = [], 0
        for q, i in enumerate(order):
            if q >= R:
                break
            running += size[i]
            if sizes_on and q > 0 and running > V:
                break
            chosen.append(i)
        if chosen:
            cursor[p] = row[chosen[-1]]
            rows_rotated += 1
        if len(chosen) < len(order):
            rows_behind += 1
        n_chosen += len(chosen)
        bytes_chosen += sum(size[i] for i in chosen)
        picked = set(chosen)
        keep = [i for i in range(n) if not is_cut[i] or i in picked]
        out.append(np.array([row[i] for i in keep], dtype=np.uint32))
        out_off[p + 1] = out_off[p] + len(keep)
        row_bytes = sum(size[i] for i in keep)
        bytes_out += row_bytes
        if sizes_on:
            out_bytes[p] = row_bytes
    out_msgs = np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)
    return out_off, out_msgs, out_bytes, dict(
        n_in=walked, n_kept_in=matched, n_chosen=n_chosen, n_out=int(out_off[-1]), bytes_chosen=bytes_chosen,
        bytes_out=bytes_out, rows_rotated=rows_rotated, rows_behind=rows_behind, error=error)


def peer_pack_np(peer_offsets, msgs, frames, frame_offsets, len_prefix=False, capacity=None):
    """Send buffers, the definition of what wq_peer_pack_device writes: for every row of the peer-major
    CSR (peer_offsets[n_peers + 1], msgs[n_in]) the records of its elements, in list order, in one byte
    run. Returns (out_bytes u8[bytes_written], peer_bytes u64[n_peers + 1], elem_bytes u64[walked],
    counters) with counters a dict of n_in, n_complete, bytes_need, bytes_written, overflow, error.

    Rows and error bit 0 are peer_budget_np's: row p is the part of [peer_offsets[p],
    peer_offsets[p + 1]) inside [0, n_in), and the rows are walked up to n_in elements in total. The
    frame of an element with message m is frames[fo[m]:fo[m + 1]], fo = frame_offsets[n_msgs + 1]; it is
    empty when m >= n_msgs (error bit 1) and when fo[m] > fo[m + 1], fo[m + 1] > len(frames) or the
    frame spans 2^32 bytes or more (error bit 2). A record is the frame, behind its size as a
    little-endian u32 with len_prefix. elem_bytes[q] is where the record of the q-th walked element
    starts and peer_bytes[p] where row p's first record does; peer_bytes[n_peers] = bytes_need. Only
    the first `capacity` bytes are written (None: all of them); n_complete counts the records that lie
    wholly below it. Row by row, for clarity."""
    off = np.ascontiguousarray(peer_offsets, dtype=np.uint32).astype(np.int64)
    msgs = np.ascontiguousarray(msgs, dtype=np.uint32)
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    fo = [int(v) for v in np.ascontiguousarray(frame_offsets, dtype=np.uint64)]
    n_in, n_peers, n_msgs, n_frame_bytes = len(msgs), max(len(off) - 1, 0), max(len(fo) - 1, 0), len(frames)
    peer_bytes = np.zeros(n_peers + 1, dtype=np.uint64)
    records, elem_bytes, walked, error, at = [], [], 0, 0, 0
    for p in range(n_peers):
        a, b = min(off[p], n_in), min(off[p + 1], n_in)
        b = max(a, b)
        if off[p] > off[p + 1] or off[p + 1] > n_in:
            error |= 1
        n = min(b - a, n_in - walked)
        if n != b - a:
            error |= 1
        walked += n
        peer_bytes[p] = at
        for m in msgs[a:a + n].tolist():
            frame = b""
            if m >= n_msgs:
                error |= 2
            elif fo[m] > fo[m + 1] or fo[m + 1] > n_frame_bytes or fo[m + 1] - fo[m] >= 1 << 32:
                error |= 4
            else:
                frame = frames[fo[m]:fo[m + 1]].tobytes()
            record = (len(frame).to_bytes(4, "little") if len_prefix else b"") + frame
            elem_bytes.append(at)
            records.append(record)
            at += len(record)
    peer_bytes[n_peers] = at
    cap = at if capacity is None else int(capacity)
    written = min(at, cap)
    out = np.frombuffer(b"".join(records)[:written], dtype=np.uint8).copy()
    n_complete = sum(1 for e, r in zip(elem_bytes, records) if e + len(r) <= cap)
    return out, peer_bytes, np.array(elem_bytes, dtype=np.uint64), dict(
        n_in=walked, n_complete=n_complete, bytes_need=at, bytes_written=written, overflow=int(at > cap), error=error)


class InterestTracker:
    """Routes ticks of `n_rows` entities (row m of every tick = entity m) and keeps the previous
    tick's CSR on the device, so every `route` also returns who entered and who left each row.

    It owns two CSR buffer sets and the two output sets (torch tensors on the router's device, int32
    holding the u32 bits); a tick is routed into the set that is not the previous one, diffed against
    the previous one, and the two swap — no CSR is copied. Once per tick it reads the route's and the
    diff's counters and waits for the device to do so: a convenience, not the asynchronous path
    (that is Router.route_device + Router.csr_diff_device). A buffer that overflows is grown and the
    step redone."""

    def __init__(self, router, n_rows: int, capacity: int, with_left: bool = True):
        import torch
        self.torch = torch
        self.router = router
        self.n_rows = int(n_rows)
        self.with_left = bool(with_left)
        self.dev = torch.device("cuda", router.device)
        cap = max(int(capacity), 1)
        i32 = dict(dtype=torch.int32, device=self.dev)
        # [offsets, peers, pairs held]; `prev` starts as the empty CSR: the first tick enters everything
        self.prev = [torch.zeros(self.n_rows + 1, **i32), torch.empty(cap, **i32), 0]
        self.cur = [torch.zeros(self.n_rows + 1, **i32), torch.empty(cap, **i32), 0]
        self.ent = [torch.zeros(self.n_rows + 1, **i32), torch.empty(cap, **i32), 0]
        self.left = [torch.zeros(self.n_rows + 1, **i32), torch.empty(cap, **i32), 0] if with_left else None
        self.route_cnt = torch.zeros(24, dtype=torch.uint8, device=self.dev)
        self.diff_cnt = torch.zeros(24, dtype=torch.uint8, device=self.dev)
        self.pack_cnt = torch.zeros(40, dtype=torch.uint8, device=self.dev)
        self.pack_buf = None  # peer_pack's send buffer, grow-only
        self.frame_cnt = torch.zeros(40, dtype=torch.uint8, device=self.dev)
        self.frame_buf = None  # build_frames' frame bytes, grow-only
        self.cursor = None     # peer_rotate's u32 cursor per observer (a message index), on the device
        torch.cuda.synchronize(self.dev)
        self.ticks = 0

    def _grow(self, buf, need: int):
        if need > buf[1].numel():
            buf[1] = self.torch.empty(need + need // 4, dtype=self.torch.int32, device=self.dev)

    def _read(self, t, dtype):
        # the handle has a stream of its own: wait for the whole device, then read
        self.torch.cuda.synchronize(self.dev)
        return t.cpu().numpy().view(dtype)[0]

    def route(self, pos_ptr: int, world_ptr: int, sender_ptr: int, repl_ptr: int):
        """One tick of n_rows messages on device pointers. Returns (ent_offsets, ent_peers,
        left_offsets, left_peers, n_entered, n_left); the tensors are views of the tracker's buffers,
        valid until the next call; the left ones are None and n_left 0 with with_left=False."""
        r, M, cur = self.router, self.n_rows, self.cur
        while True:
            r.route_device(pos_ptr, world_ptr, sender_ptr, repl_ptr, M, cur[0].data_ptr(), cur[1].data_ptr(), None,
                           cur[1].numel(), self.route_cnt.data_ptr())
            c = self._read(self.route_cnt, abi.COUNTERS_DTYPE)
            if c["error"]:
                r.check_health()
                raise RuntimeError(f"route error bits {int(c['error']):#x}")
            cur[2] = int(c["n_pairs"]) if M else 0
            if not c["overflow"]:
                break
            r.route_health()  # the retried tick's overflow is handled here: clear the sticky word
            self._grow(cur, cur[2])
        prev, ent, left = self.prev, self.ent, self.left
        while True:
            r.csr_diff_device(M, prev[0].data_ptr(), prev[1].data_ptr(), prev[1].numel(), cur[0].data_ptr(),
                              cur[1].data_ptr(), cur[1].numel(), ent[0].data_ptr(), ent[1].data_ptr(),
                              ent[1].numel(), left[0].data_ptr() if left else None,
                              left[1].data_ptr() if left else None, left[1].numel() if left else 0,
                              self.diff_cnt.data_ptr())
            d = self._read(self.diff_cnt, abi.DIFF_COUNTERS_DTYPE)
            if d["error"]:
                raise RuntimeError("the diff read a CSR whose offsets do not ascend within its capacity")
            ent[2] = int(d["n_entered"])
            if left:
                left[2] = int(d["n_left"])
            if not d["overflow"]:
                break
            self._grow(ent, ent[2])
            if left:
                self._grow(left, left[2])
        self.prev, self.cur = cur, prev
        self.ticks += 1
        return (ent[0], ent[1][: ent[2]], left[0] if left else None, left[1][: left[2]] if left else None,
                ent[2], left[2] if left else 0)

    def current(self):
        """(offsets, peers[:P]) of the latest tick's CSR (device tensors, valid until the next call)."""
        return self.prev[0], self.prev[1][: self.prev[2]]

    def peer_major(self, which: str, connected_ptr: int | None, n_peers: int):
        """Per observer the entities that entered ("entered") or left ("left") its view in the latest
        tick: (peer_offsets[n_peers + 1], rows[kept]) through wq_peer_major_device."""
        torch = self.torch
        if which not in ("entered", "left") or (which == "left" and not self.left):
            raise ValueError("which is 'entered' or 'left' (the latter only with with_left=True)")
        src = self.ent if which == "entered" else self.left
        po = torch.empty(n_peers + 1, dtype=torch.int32, device=self.dev)
        rows = torch.empty(max(src[2], 1), dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        self.router.peer_major_device(src[0].data_ptr(), src[1].data_ptr() if src[2] else None, self.n_rows, src[2],
                                      connected_ptr, n_peers, po.data_ptr(), rows.data_ptr() if src[2] else None)
        torch.cuda.synchronize(self.dev)
        kept = int(po[n_peers].item()) & 0xFFFFFFFF
        return po, rows[:kept]

    def peer_budget(self, peer_offsets, rows, msg_pos_ptr: int, k: int | None = None, budget_ptr: int | None = None,
                    peer_pos_ptr: int | None = None, n_peer_pos: int = 0):
        """Chains after peer_major: of every observer's list (peer_offsets, rows — the tensors peer_major
        returned) the min(budget, len) entities nearest to it, in input order, through
        wq_peer_budget_device: (out_offsets[n_peers + 1], out_rows[kept]). msg_pos_ptr: the tick's
        n_rows x 3 f64 positions on the device; the observers' positions are the router's
        set_peer_positions unless peer_pos_ptr / n_peer_pos give others; budget_ptr: u32 per observer,
        else k for everyone."""
        torch = self.torch
        if k is None and budget_ptr is None:
            raise ValueError("give k or budget_ptr")
        n_peers, n_in = peer_offsets.numel() - 1, rows.numel()
        oo = torch.empty(n_peers + 1, dtype=torch.int32, device=self.dev)
        om = torch.empty(max(n_in, 1), dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        self.router.peer_budget_device(peer_offsets.data_ptr(), rows.data_ptr() if n_in else None, n_peers, n_in,
                                       msg_pos_ptr, self.n_rows, peer_pos_ptr, n_peer_pos, k or 0, budget_ptr,
                                       oo.data_ptr(), om.data_ptr() if n_in else None, None)
        torch.cuda.synchronize(self.dev)
        kept = int(oo[n_peers].item()) & 0xFFFFFFFF
        return oo, om[:kept]

    def peer_budget_bytes(self, peer_offsets, rows, msg_pos_ptr: int, msg_size_ptr: int, w: int | None = None,
                          budget_bytes_ptr: int | None = None, peer_pos_ptr: int | None = None, n_peer_pos: int = 0):
        """Chains after peer_major or peer_budget: of every observer's list the nearest entities whose
        sizes (msg_size_ptr: u32 per entity on the device, see frame_sizes) sum to at most its byte
        budget (budget_bytes_ptr: u64 per observer, else w for everyone), in input order, through
        wq_peer_budget_bytes_device: (out_offsets[n_peers + 1], out_rows[kept], out_bytes[n_peers]), the
        last an int64 tensor of every observer's kept bytes. Positions as in peer_budget."""
        torch = self.torch
        if w is None and budget_bytes_ptr is None:
            raise ValueError("give w or budget_bytes_ptr")
        n_peers, n_in = peer_offsets.numel() - 1, rows.numel()
        oo = torch.empty(n_peers + 1, dtype=torch.int32, device=self.dev)
        om = torch.empty(max(n_in, 1), dtype=torch.int32, device=self.dev)
        ob = torch.empty(max(n_peers, 1), dtype=torch.int64, device=self.dev)
        torch.cuda.synchronize(self.dev)
        self.router.peer_budget_bytes_device(peer_offsets.data_ptr(), rows.data_ptr() if n_in else None, n_peers, n_in,
                                             msg_pos_ptr, msg_size_ptr, self.n_rows, peer_pos_ptr, n_peer_pos, w or 0,
                                             budget_bytes_ptr, oo.data_ptr(), om.data_ptr() if n_in else None,
                                             ob.data_ptr(), None)
        torch.cuda.synchronize(self.dev)
        kept = int(oo[n_peers].item()) & 0xFFFFFFFF
        return oo, om[:kept], ob[:n_peers]

    def peer_rotate(self, peer_offsets, rows, kept_offsets, kept_rows, r: int | None = None,
                    extra_ptr: int | None = None, msg_size_ptr: int | None = None, v: int | None = None,
                    extra_bytes_ptr: int | None = None):
        """Chains after peer_budget / peer_budget_bytes: the budget's output (kept_offsets, kept_rows) of
        the lists (peer_offsets, rows) plus, per observer, the cut entities that follow its cursor in
        cyclic order of entity index, at most r of them (extra_ptr: u32 per observer) and, with
        msg_size_ptr, at most v bytes (extra_bytes_ptr: u64 per observer), through
        wq_peer_rotate_device: (out_offsets[n_peers + 1], out_rows[n_out], out_bytes[n_peers] or None
        without sizes). The tracker owns the cursors (self.cursor, one u32 per observer on the device,
        0xFFFFFFFF for an observer not seen before) and they move with every call, so an entity that
        stays in an observer's list and stays cut arrives within ceil(cut / r) ticks. The call is
        enqueued and nothing is read back: out_rows is the whole buffer (n_in elements), of which
        out_offsets[n_peers] are valid, and feeds peer_pack with n_in = rows.numel() unchanged."""
        torch = self.torch
        if r is None and extra_ptr is None:
            raise ValueError("give r or extra_ptr")
        if msg_size_ptr is not None and v is None and extra_bytes_ptr is None:
            raise ValueError("with msg_size_ptr give v or extra_bytes_ptr")
        n_peers, n_in, n_kin = peer_offsets.numel() - 1, rows.numel(), kept_rows.numel()
        if kept_offsets.numel() != n_peers + 1:
            raise ValueError("the kept lists cover the same observers")
        have = 0 if self.cursor is None else self.cursor.numel()
        if have < n_peers:
            grown = torch.full((n_peers,), -1, dtype=torch.int32, device=self.dev)
            if have:
                grown[:have] = self.cursor
            self.cursor = grown
        oo = torch.empty(n_peers + 1, dtype=torch.int32, device=self.dev)
        om = torch.empty(max(n_in, 1), dtype=torch.int32, device=self.dev)
        ob = torch.empty(max(n_peers, 1), dtype=torch.int64, device=self.dev) if msg_size_ptr is not None else None
        torch.cuda.synchronize(self.dev)   # torch's stream filled the cursors; the call runs on the handle's
        self.router.peer_rotate_device(peer_offsets.data_ptr(), rows.data_ptr() if n_in else None, n_peers, n_in,
                                       kept_offsets.data_ptr(), kept_rows.data_ptr() if n_kin else None, n_kin,
                                       msg_size_ptr, self.n_rows if msg_size_ptr is not None else 0, r or 0, extra_ptr,
                                       v or 0, extra_bytes_ptr, self.cursor.data_ptr() if n_peers else None,
                                       oo.data_ptr(), om.data_ptr() if n_in else None,
                                       ob.data_ptr() if ob is not None else None, None)
        return oo, om[:n_in], (ob[:n_peers] if ob is not None else None)

    def build_frames(self, src: "abi.FramesSrc"):
        """The tick's frames built on the device through wq_frames_build_device, for entity updates
        whose fields are already there (src: abi.FramesSrc of device pointers over the n_rows entities,
        worlds as ids into the router's set_worlds table): (frames[bytes_need] uint8,
        frame_offsets[n_rows + 1] int64, frame_size[n_rows] int32 holding the u32 bits). They are what
        peer_budget_bytes takes as msg_size_ptr and peer_pack as frames_ptr / frame_offsets_ptr /
        n_frame_bytes (frames.numel()), so a tick goes from positions to packed runs without the host
        building or uploading a frame. `frames` is a view of the tracker's grow-only buffer, valid until
        the next call; a buffer that is too small is grown to bytes_need and the call made once more.
        Error bits (a world id outside the table, a payload range out of bounds, a frame above 2^30
        bytes) raise."""
        torch = self.torch
        n = self.n_rows
        if self.frame_buf is None:
            self.frame_buf = torch.empty(1 << 20, dtype=torch.uint8, device=self.dev)
        fo = torch.empty(n + 1, dtype=torch.int64, device=self.dev)
        fs = torch.empty(max(n, 1), dtype=torch.int32, device=self.dev)
        for _ in range(2):
            torch.cuda.synchronize(self.dev)
            self.router.build_frames_device(src, n, self.frame_buf.data_ptr(), self.frame_buf.numel(), fo.data_ptr(),
                                            fs.data_ptr(), self.frame_cnt.data_ptr())
            c = self._read(self.frame_cnt, abi.FRAMES_COUNTERS_DTYPE)
            if not c["overflow"]:
                break
            need = int(c["bytes_need"])
            self.frame_buf = torch.empty(need + need // 4, dtype=torch.uint8, device=self.dev)
        if c["error"]:
            raise RuntimeError(f"build_frames error bits {int(c['error']):#x}")
        return self.frame_buf[: int(c["bytes_written"])], fo, fs[:n]

    def peer_pack(self, peer_offsets, rows, frames_ptr: int, frame_offsets_ptr: int, n_frame_bytes: int,
                  len_prefix: bool = False):
        """Chains after peer_major or either budget: every observer's frames in one contiguous byte run,
        in list order, through wq_peer_pack_device: (out[bytes_need] uint8, peer_bytes[n_peers + 1],
        elem_bytes[n_in]), the last two int64 tensors; observer p's run is out[peer_bytes[p]:
        peer_bytes[p + 1]] and the record of list element q starts at elem_bytes[q]. frames_ptr /
        frame_offsets_ptr: the tick's frames on the device as wq_serialize_messages leaves them (u8 bytes,
        u64 offsets[n_rows + 1]), uploaded once per tick or built on the device by build_frames. `out` is
        a view of the tracker's grow-only buffer, valid until the next call; a buffer that is too small
        is grown to bytes_need and the call made once more."""
        torch = self.torch
        n_peers, n_in = peer_offsets.numel() - 1, rows.numel()
        if self.pack_buf is None:
            self.pack_buf = torch.empty(1 << 20, dtype=torch.uint8, device=self.dev)
        pb = torch.empty(n_peers + 1, dtype=torch.int64, device=self.dev)
        eb = torch.empty(max(n_in, 1), dtype=torch.int64, device=self.dev)
        flags = abi.PACK_LEN_PREFIX if len_prefix else 0
        for _ in range(2):
            torch.cuda.synchronize(self.dev)
            self.router.peer_pack_device(peer_offsets.data_ptr(), rows.data_ptr() if n_in else None, n_peers, n_in,
                                         frames_ptr, frame_offsets_ptr, self.n_rows, n_frame_bytes, flags,
                                         self.pack_buf.data_ptr(), self.pack_buf.numel(), pb.data_ptr(),
                                         eb.data_ptr() if n_in else None, self.pack_cnt.data_ptr())
            c = self._read(self.pack_cnt, abi.PACK_COUNTERS_DTYPE)
            if not c["overflow"]:
                break
            need = int(c["bytes_need"])
            self.pack_buf = torch.empty(need + need // 4, dtype=torch.uint8, device=self.dev)
        if c["error"]:
            raise RuntimeError(f"peer_pack error bits {int(c['error']):#x}")
        return self.pack_buf[: int(c["bytes_written"])], pb, eb[: int(c["n_in"])]
