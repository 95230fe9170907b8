"""Interest changes between two ticks on the GPU (wq_csr_diff*, csrc/wq_csr_diff.hip): who entered
and who left each row.

Bars: all four output arrays and both counters are byte-identical to the host reference
(worldql_server_amd/interest.py csr_diff_np), twice in a row; nothing is written at or past a
capacity; offsets that do not describe a CSR are read as interest.clamp_csr_np reads them.
"""
import ctypes

import numpy as np
import pytest

from worldql_server_amd import abi, interest, synth_ext

from test_csr_diff_host import cases, descending_pair, rows_of

pytestmark = pytest.mark.gpu

CANARY = 0x5EEDC0DE
GUARD = 1024  # canary words on either side of an exactly sized device array


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def wants():
    """csr_diff_np of every shared case, computed once."""
    return {name: interest.csr_diff_np(*c) for name, c in cases().items()}


class Dev:
    """A u32 device array of exactly n words between two canary guards."""

    def __init__(self, data=None, n=None, fill=CANARY):
        import torch
        n = len(data) if data is not None else n
        host = np.full(n + 2 * GUARD, CANARY, np.uint32)
        host[GUARD:GUARD + n] = data if data is not None else fill
        self.n = n
        self.t = torch.from_numpy(host.view(np.int32)).to("cuda:0")
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def read(self):
        """(the array, are both guards intact)"""
        import torch
        torch.cuda.synchronize()
        h = self.t.cpu().numpy().view(np.uint32)
        ok = bool((h[:GUARD] == CANARY).all() and (h[GUARD + self.n:] == CANARY).all())
        return h[GUARD:GUARD + self.n], ok


def device_diff(r, oo, op, no, npr, ent_cap=None, left=True, left_cap=None, old_cap=None, new_cap=None):
    """wq_csr_diff_device on exactly sized guarded arrays. Returns (ent_off, ent_peers buffer,
    left_off, left_peers buffer, counters, the Dev objects)."""
    import torch
    M = len(oo) - 1
    d_oo, d_op, d_no, d_np = Dev(oo), Dev(op), Dev(no), Dev(npr)
    ce = len(npr) if ent_cap is None else ent_cap
    cl = len(op) if left_cap is None else left_cap
    d_eo, d_ep, d_lo, d_lp = Dev(n=M + 1), Dev(n=ce), Dev(n=M + 1), Dev(n=cl)
    cnt = torch.zeros(24, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    r.csr_diff_device(M, d_oo.ptr, d_op.ptr if len(op) else None, len(op) if old_cap is None else old_cap,
                      d_no.ptr, d_np.ptr if len(npr) else None, len(npr) if new_cap is None else new_cap,
                      d_eo.ptr, d_ep.ptr if ce else None, ce,
                      d_lo.ptr if left else None, (d_lp.ptr if cl else None) if left else None, cl if left else 0,
                      cnt.data_ptr())
    torch.cuda.synchronize()
    c = cnt.cpu().numpy().view(abi.DIFF_COUNTERS_DTYPE)[0]
    outs = []
    for d in (d_eo, d_ep, d_lo, d_lp, d_oo, d_op, d_no, d_np):
        a, ok = d.read()
        assert ok, "a guard word next to a device array was overwritten"
        outs.append(a)
    return outs[0], outs[1], outs[2], outs[3], c


def _bytes_equal(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.uint32 and g.tobytes() == w.tobytes()


@pytest.mark.parametrize("name", sorted(cases()))
def test_exact_on_the_host_cases(router, wants, name):
    oo, op, no, npr = cases()[name]
    want = wants[name]
    first = router.csr_diff(oo, op, no, npr)
    _bytes_equal(first[:4], want)
    assert first[4:] == (len(want[1]), len(want[3]))
    second = router.csr_diff(oo, op, no, npr)
    _bytes_equal(second[:4], first[:4])
    assert second[4:] == first[4:]


def test_long_rows_and_skew_device_form(router, wants):
    """One row of 5,000 peers against 4,999 shifted by one among 300 empty rows, then 64 rows of 257:
    rows far longer than a wave's 64 ordinals, through the asynchronous form."""
    for name, n_ent in (("skew_5000", 2500), ("rows_of_257", 64 * 100)):
        oo, op, no, npr = cases()[name]
        w_eo, w_ep, w_lo, w_lp = wants[name]
        assert len(w_ep) == n_ent
        eo, ep, lo, lp, c = device_diff(router, oo, op, no, npr)
        assert (int(c["n_entered"]), int(c["n_left"]), int(c["overflow"]), int(c["error"])) == (len(w_ep), len(w_lp), 0, 0)
        _bytes_equal((eo, ep[:len(w_ep)], lo, lp[:len(w_lp)]), (w_eo, w_ep, w_lo, w_lp))
        assert (ep[len(w_ep):] == CANARY).all() and (lp[len(w_lp):] == CANARY).all()


def test_left_side_off(router, wants):
    oo, op, no, npr = cases()["random_2000"]
    w_eo, w_ep, _, _ = wants["random_2000"]
    eo, ep, lo, lp, c = device_diff(router, oo, op, no, npr, left=False)
    assert (int(c["n_entered"]), int(c["n_left"]), int(c["overflow"]), int(c["error"])) == (len(w_ep), 0, 0, 0)
    _bytes_equal((eo, ep[:len(w_ep)]), (w_eo, w_ep))
    assert (lo == CANARY).all() and (lp == CANARY).all()   # the left buffers were not passed: untouched
    got = router.csr_diff(oo, op, no, npr, with_left=False)
    _bytes_equal(got[:2], (w_eo, w_ep))
    assert got[2] is None and got[3] is None and got[4:] == (len(w_ep), 0)


def test_capacity(router, wants):
    from worldql_server_amd.router import WQError
    oo, op, no, npr = cases()["random_2000"]
    w_eo, w_ep, w_lo, w_lp = wants["random_2000"]
    E, L = len(w_ep), len(w_lp)
    for cap in (E - 1, 0):
        # Dev(n=cap) is exactly `cap` words: the guard behind it is the canary after `capacity`
        eo, ep, lo, lp, c = device_diff(router, oo, op, no, npr, ent_cap=cap)
        assert int(c["n_entered"]) == E and int(c["n_left"]) == L
        assert int(c["overflow"]) == abi.DIFF_OVERFLOW_ENTERED and int(c["error"]) == 0
        _bytes_equal((eo, ep, lo, lp[:L]), (w_eo, w_ep[:cap], w_lo, w_lp))
        with pytest.raises(WQError) as e:
            router.csr_diff(oo, op, no, npr, ent_capacity=cap)
        assert e.value.code == abi.WQ_E_CAPACITY and e.value.sizes == (E, L)
        _bytes_equal(e.value.offsets, (w_eo, w_lo))
    eo, ep, lo, lp, c = device_diff(router, oo, op, no, npr, left_cap=L - 1)
    assert int(c["overflow"]) == abi.DIFF_OVERFLOW_LEFT and int(c["n_left"]) == L
    _bytes_equal((eo, ep[:E], lo, lp), (w_eo, w_ep, w_lo, w_lp[:L - 1]))


def test_clamping(router):
    """Offsets that reach past the array or descend: a correct run on the clamped rows (the arrays are
    exactly `capacity` words between canary guards; device_diff checks the guards)."""
    oo, op, no, npr = cases()["rows_513"]
    # a truncated tick: new_capacity below new_offsets[n_rows]
    cap = int(no[-1]) * 2 // 3
    c_no, c_np, cut = interest.clamp_csr_np(no, npr[:cap], cap)
    assert cut
    want = interest.csr_diff_np(oo, op, c_no, c_np)
    eo, ep, lo, lp, c = device_diff(router, oo, op, no, npr[:cap].copy())
    assert int(c["error"]) == abi.DIFF_ERROR_ROWS and int(c["overflow"]) == 0
    assert (int(c["n_entered"]), int(c["n_left"])) == (len(want[1]), len(want[3]))
    _bytes_equal((eo, ep[:len(want[1])], lo, lp[:len(want[3])]), want)
    # one row with offsets[m + 1] < offsets[m], on the old side
    bad, bad_p = descending_pair(oo, op)
    c_oo, c_op, cut = interest.clamp_csr_np(bad, bad_p)
    assert cut
    want = interest.csr_diff_np(c_oo, c_op, no, npr)
    eo, ep, lo, lp, c = device_diff(router, bad, bad_p, no, npr, left_cap=len(bad_p) + 3)
    assert int(c["error"]) == abi.DIFF_ERROR_ROWS and int(c["overflow"]) == 0
    assert (int(c["n_entered"]), int(c["n_left"])) == (len(want[1]), len(want[3]))
    _bytes_equal((eo, ep[:len(want[1])], lo, lp[:len(want[3])]), want)
    # the next call on the handle starts from a clean error word
    eo, ep, lo, lp, c = device_diff(router, oo, op, no, npr)
    assert int(c["error"]) == 0


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint32).copy()


def _check_tick(prev, cur, out, n_peers, tracker):
    """One tracker tick against csr_diff_np of the two route outputs; returns (E, L)."""
    eo, ep, lo, lp, ne, nl = out
    want = interest.csr_diff_np(prev[0], prev[1], cur[0], cur[1])
    _bytes_equal((_host(eo), _host(ep), _host(lo), _host(lp)), want)
    assert (ne, nl) == (len(want[1]), len(want[3]))
    for o, n, e, l in zip(rows_of(*prev), rows_of(*cur), rows_of(want[0], want[1]), rows_of(want[2], want[3])):
        assert (set(o.tolist()) | set(e.tolist())) - set(l.tolist()) == set(n.tolist())
    po, rows = tracker.peer_major("entered", None, n_peers)
    w_po, w_rows = interest.peer_major_np(want[0], want[1], n_peers)
    _bytes_equal((_host(po), _host(rows)), (w_po, w_rows))
    # the same with a connected bitmap: about a third of the observers are dropped
    n_seen = n_peers - 3
    conn = np.packbits(np.random.default_rng(ne).random(((n_seen + 31) // 32) * 32) < 0.66,
                       bitorder="little").view(np.uint32)
    d_conn = _dev(conn)
    po, rows = tracker.peer_major("entered", d_conn.data_ptr(), n_seen)
    w_po, w_rows = interest.peer_major_np(want[0], want[1], n_seen, conn)
    assert ne == 0 or 0 < len(w_rows) < ne
    _bytes_equal((_host(po), _host(rows)), (w_po, w_rows))
    return ne, nl


@pytest.mark.parametrize("kind", ["single", "replicate"])
def test_c5_ticks_through_the_tracker(kind):
    from worldql_server_amd.router import Router
    c5 = synth_ext.config_c5(scale=0.01)
    n = c5.n
    r = Router(16, 0) if kind == "single" else Router.multi(16, (0, 0), mode="replicate")
    r.set_radius(c5.radius)
    world = np.zeros(n, np.uint32)
    tracker = interest.InterestTracker(r, n, n)   # P is about 1.9 n: the first tick grows every buffer
    prev = (np.zeros(n + 1, np.uint32), np.zeros(0, np.uint32))
    for tick in range(4):
        r.follow_peers(world, c5.pos)
        r.set_peer_positions(c5.pos)
        pos, w, s, rp = c5.messages()
        d = [_dev(x) for x in (pos, w, s, rp)]
        out = tracker.route(*(x.data_ptr() for x in d))
        cur = tuple(_host(t) for t in tracker.current())
        ref = r.route(pos, w, s, rp, capacity=256 * n)      # the tick itself, through the host form
        _bytes_equal(cur, ref[:2])
        ne, nl = _check_tick(prev, cur, out, n, tracker)
        if tick == 0:
            assert ne == len(cur[1]) > 0 and nl == 0        # the first tick enters everything
        else:
            assert ne > 0 and nl > 0                        # entities moved: not a vacuous diff
        prev = cur
        c5.step()
    r.route_health()
    r.close()


def test_c4_tick_pair_except_self():
    from worldql_server_amd.router import Router
    c4 = synth_ext.config_c4(scale=0.01, worlds=range(4))
    n = c4.n_peers
    r = Router(16, 0)
    r.follow_peers(c4.world, c4.pos)
    tracker = interest.InterestTracker(r, n, 64 * n)
    prev = (np.zeros(n + 1, np.uint32), np.zeros(0, np.uint32))
    for tick in range(2):
        _, pos, w, s, rp = c4.step(move_frac=0.05)
        assert (rp == abi.REPL_EXCEPT_SELF).all()
        r.follow_peers(c4.world, c4.pos)
        d = [_dev(x) for x in (pos, w, s, rp)]
        out = tracker.route(*(x.data_ptr() for x in d))
        cur = tuple(_host(t) for t in tracker.current())
        ne, nl = _check_tick(prev, cur, out, n, tracker)
        assert ne > 0 and (tick == 0 or nl > 0)
        prev = cur
    assert r.route_health() == (0, 0)
    r.close()


def test_errors(router):
    from worldql_server_amd.router import WQError, load_library
    lib = load_library()
    oo, op, no, npr = cases()["rows_257"]
    M = len(oo) - 1
    d = {k: Dev(v) for k, v in (("oo", oo), ("op", op), ("no", no), ("np", npr))}
    d_eo, d_ep, d_lo, d_lp = Dev(n=M + 1), Dev(n=len(npr)), Dev(n=M + 1), Dev(n=len(op))

    def call(**kw):
        a = dict(n_rows=M, old_offsets_ptr=d["oo"].ptr, old_peers_ptr=d["op"].ptr, old_capacity=len(op),
                 new_offsets_ptr=d["no"].ptr, new_peers_ptr=d["np"].ptr, new_capacity=len(npr),
                 ent_offsets_ptr=d_eo.ptr, ent_peers_ptr=d_ep.ptr, ent_capacity=len(npr),
                 left_offsets_ptr=d_lo.ptr, left_peers_ptr=d_lp.ptr, left_capacity=len(op))
        a.update(kw)
        router.csr_diff_device(**a)

    bad = [dict(old_offsets_ptr=None), dict(new_offsets_ptr=None), dict(ent_offsets_ptr=None),
           dict(old_peers_ptr=None), dict(new_peers_ptr=None), dict(ent_peers_ptr=None),
           dict(left_peers_ptr=None),                               # a size without its array
           dict(left_offsets_ptr=None),                             # half a left side: peers without offsets
           dict(left_offsets_ptr=None, left_peers_ptr=None),        # ... or a capacity without either
           dict(n_rows=2 ** 32 - 1024)]
    for kw in bad:
        with pytest.raises(WQError) as e:
            call(**kw)
        assert e.value.code == abi.WQ_E_INVALID, kw
    args = [M, d["oo"].ptr, d["op"].ptr, len(op), d["no"].ptr, d["np"].ptr, len(npr), d_eo.ptr, d_ep.ptr, len(npr),
            d_lo.ptr, d_lp.ptr, len(op), None]
    assert lib.wq_csr_diff_device(None, *args) == abi.WQ_E_INVALID     # a null handle
    ne, nl = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.wq_csr_diff(None, *args[:-1], ctypes.byref(ne), ctypes.byref(nl)) == abi.WQ_E_INVALID
    # nothing was launched: every output still holds its canary
    for o in (d_eo, d_ep, d_lo, d_lp):
        a, ok = o.read()
        assert ok and (a == CANARY).all()
    call(left_offsets_ptr=None, left_peers_ptr=None, left_capacity=0)  # the valid way to leave it out
    call()
    a, ok = d_eo.read()
    assert ok and a[0] == 0
