"""GPU parity for the send budgets (include/wq_router.h wq_peer_budget_device, csrc/wq_budget.hip): of
every peer's send list the min(B, len) messages nearest to the peer, in input order.

Bars, all bit-exact against worldql_server_amd/interest.py peer_budget_np (the shared case list of
tests/test_peer_budget_host.py, where the definition itself is checked against a restatement):
  - d_out_offsets[0 .. n_peers], d_out_msgs[0 .. n_kept) and the counters are the definition's bytes,
    for ascending offsets and for hostile ones (the header's rule for overlapping rows);
  - every device array is sized exactly, with FRONT guard words before it and SLACK behind it, all
    holding a canary: the words before and behind d_out_offsets[0 .. n_peers], before d_out_msgs and
    behind d_out_msgs[n_kept) (the rest of the array included), and around (and inside) every input
    are as they were;
  - every case runs twice on one handle, and the largest after the smallest, so stale scratch shows;
  - the f64 expression is not contracted on the GPU: the fma_boundary cases and the last-ulp cases
    compare equal to numpy, which never contracts."""
import ctypes

import numpy as np
import pytest

from worldql_server_amd import abi, interest, synth_ext

from test_peer_budget_host import cases, exact_names, hostile_names, want, well_formed

pytestmark = pytest.mark.gpu

CANARY = 0xA5A5A5A5   # no message index of any case, above every n_in
SLACK = 1024          # guard words behind every device array
FRONT = 1024          # guard words before it (4 KB: the array keeps the allocation's alignment)


class Guarded:
    """A device array of the bytes of `data` (or n u32 canaries) with FRONT guard words before it and
    SLACK behind it; ptr is the array's first byte."""

    def __init__(self, data=None, n=None, device="cuda:0"):
        import torch
        body = np.ascontiguousarray(data).view(np.uint8).reshape(-1) if data is not None else \
            np.full(n, CANARY, np.uint32).view(np.uint8)
        assert len(body) % 4 == 0
        self.n_bytes = len(body)
        guard = lambda words: np.full(words, CANARY, np.uint32).view(np.uint8)
        self.host = np.concatenate([guard(FRONT), body, guard(SLACK)])
        self.t = torch.from_numpy(self.host.copy()).to(device)
        self.ptr = self.t.data_ptr() + 4 * FRONT
        assert self.ptr % 8 == 0

    def read(self, dtype=np.uint32):
        """The array and the guard words behind it."""
        return self.t.cpu().numpy()[4 * FRONT:].view(dtype)

    def front_intact(self):
        return bool((self.t[:4 * FRONT].cpu().numpy().view(np.uint32) == CANARY).all())

    def unchanged(self):
        return self.t.cpu().numpy().tobytes() == self.host.tobytes()


class Call:
    """One case on the device: guarded inputs and outputs, and the checks after a call."""

    def __init__(self, c, device="cuda:0", handle_positions=False):
        self.c, self.n_in = c, len(c.msgs)
        self.handle_positions = handle_positions
        g = lambda a: Guarded(a, device=device)
        self.off, self.msgs, self.mpos, self.ppos = g(c.offsets), g(c.msgs), g(c.msg_pos), g(c.peer_pos)
        self.budget = g(c.budget) if c.budget is not None else None
        self.oo = Guarded(n=c.n_peers + 1, device=device)
        self.om = Guarded(n=self.n_in, device=device)
        self.cnt = Guarded(n=6, device=device)

    def launch(self, r):
        """Enqueues the call; nothing is waited for."""
        c = self.c
        explicit = not self.handle_positions
        r.peer_budget_device(self.off.ptr, self.msgs.ptr if self.n_in else None, c.n_peers, self.n_in,
                             self.mpos.ptr if len(c.msg_pos) else None, len(c.msg_pos),
                             self.ppos.ptr if explicit else None,     # non-NULL with n_peer_pos 0: nobody has a position
                             len(c.peer_pos) if explicit else 0, c.k,
                             self.budget.ptr if self.budget is not None else None, self.oo.ptr,
                             self.om.ptr if self.n_in else None, self.cnt.ptr)

    def outputs(self):
        """(out_offsets, out_msgs[:n_kept], counters) after the canary checks on every array."""
        import torch
        torch.cuda.synchronize()
        c = self.c
        oo, om = self.oo.read(), self.om.read()
        cnt = self.cnt.read(np.uint8)[:24].view(abi.BUDGET_COUNTERS_DTYPE)[0]
        counters = {k: int(cnt[k]) for k in abi.BUDGET_COUNTERS_DTYPE.names}
        assert (oo[c.n_peers + 1:] == CANARY).all(), "written behind d_out_offsets[n_peers]"
        assert counters["n_kept"] <= self.n_in
        assert (om[counters["n_kept"]:] == CANARY).all(), "written behind d_out_msgs[n_kept)"
        assert (self.cnt.read()[6:] == CANARY).all(), "written behind the counters"
        for a, what in ((self.oo, "d_out_offsets"), (self.om, "d_out_msgs"), (self.cnt, "the counters")):
            assert a.front_intact(), "written before " + what
        for a in (self.off, self.msgs, self.mpos, self.ppos, self.budget):
            assert a is None or a.unchanged(), "an input was written"
        return oo[:c.n_peers + 1], om[:counters["n_kept"]], counters

    def run(self, r):
        import torch
        torch.cuda.synchronize()
        self.launch(r)
        return self.outputs()


def check(name, oo, om, counters):
    w_oo, w_om, w_cnt = want(name)
    assert counters == w_cnt, name
    assert oo.tobytes() == w_oo.tobytes(), (name, "offsets")
    assert om.tobytes() == w_om.tobytes(), (name, "messages")
    well_formed(cases()[name], oo, om, counters)


def run_case(r, name, device="cuda:0"):
    check(name, *Call(cases()[name], device).run(r))


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    yield r
    r.close()


# ---- the shared cases ---------------------------------------------------------------------

@pytest.mark.parametrize("name", exact_names())
def test_exact_on_the_shared_cases(router, name):
    """Twice on one handle (the second call sees the first one's scratch)."""
    run_case(router, name)
    run_case(router, name)


@pytest.mark.parametrize("name", hostile_names())
def test_hostile_offsets(router, name):
    """Descending, wrapped and overlapping offsets: in bounds, the same bytes twice, error bit 0, and
    the definition's result for the rows the header describes."""
    c = cases()[name]
    first = Call(c).run(router)
    well_formed(c, *first)
    assert first[2]["error"] & abi.BUDGET_ERROR_ROWS
    again = Call(c).run(router)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2] == again[2]
    check(name, *first)


def test_stale_scratch_largest_after_smallest():
    """A fresh handle: the smallest cases, the largest one, and the small ones again."""
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    for name in ("size_nothing", "ties_repeated_message", "long_row_k100000", "ties_repeated_message",
                 "len_edges_k64", "long_row_k7", "size_no_elements", "keys_top_digit_700_k350"):
        run_case(r, name)
    r.close()


def test_steady_state_allocates_nothing(router):
    """After one call has grown the scratch, the very next call of the same size and a smaller one
    leave the device's free memory as it was. The handle has no allocation counter, so this reads
    hipMemGetInfo, which other processes on the device move too. The scratch only ever grows, so a
    call that allocated can only lower the figure: a lower figure fails at once, and the pair is
    measured again only when the figure went up, which another process alone can do."""
    import torch
    call, small = Call(cases()["long_row_k100000"]), Call(cases()["len_edges_k64"])
    call.run(router)
    for _ in range(5):
        free = torch.cuda.mem_get_info()[0]
        check("long_row_k100000", *call.run(router))
        small.run(router)
        after = torch.cuda.mem_get_info()[0]
        assert after >= free, ("a steady-state call allocated", free - after)
        if after == free:
            return
    pytest.fail("the device's free memory kept rising: no quiet pair in five")


# ---- the pipeline ---------------------------------------------------------------------------

def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _pipeline(r, pos, world, sender, repl, n_peers, capacity, k):
    """tick -> peer_major -> peer_budget with the handle's positions, nothing read in between.
    Returns the downloaded (offsets, peers, peer_offsets, rows, out_offsets, out_msgs, counters)."""
    import torch
    M = len(world)
    d_in = [_dev(x) for x in (pos, world, sender, repl)]
    i32 = dict(dtype=torch.int32, device="cuda:0")
    canary = int(np.uint32(CANARY).view(np.int32))
    offs, peers = torch.empty(M + 1, **i32), torch.full((capacity + SLACK,), canary, **i32)
    po, rows = torch.empty(n_peers + 1, **i32), torch.full((capacity + SLACK,), canary, **i32)
    oo = torch.full((FRONT + n_peers + 1 + SLACK,), canary, **i32)
    om = torch.full((FRONT + capacity + SLACK,), canary, **i32)
    cnt = torch.zeros(24, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    r.route_device(*(x.data_ptr() for x in d_in), M, offs.data_ptr(), peers.data_ptr(), None, capacity)
    r.peer_major_device(offs.data_ptr(), peers.data_ptr(), M, capacity, None, n_peers, po.data_ptr(), rows.data_ptr())
    r.peer_budget_device(po.data_ptr(), rows.data_ptr(), n_peers, capacity, d_in[0].data_ptr(), M, None, 0, k, None,
                         oo.data_ptr() + 4 * FRONT, om.data_ptr() + 4 * FRONT, cnt.data_ptr())
    torch.cuda.synchronize()
    c = cnt.cpu().numpy().view(abi.BUDGET_COUNTERS_DTYPE)[0]
    counters = {f: int(c[f]) for f in abi.BUDGET_COUNTERS_DTYPE.names}
    oo, om = _u32(oo), _u32(om)
    assert (oo[:FRONT] == CANARY).all() and (om[:FRONT] == CANARY).all()
    oo, om = oo[FRONT:], om[FRONT:]
    assert (oo[n_peers + 1:] == CANARY).all() and (om[counters["n_kept"]:] == CANARY).all()
    assert (_u32(rows)[capacity:] == CANARY).all() and (_u32(peers)[capacity:] == CANARY).all()
    return _u32(offs), _u32(peers)[:capacity], _u32(po), _u32(rows)[:capacity], oo[:n_peers + 1], \
        om[:counters["n_kept"]], counters


def _check_pipeline(res, pos, peer_pos, k, radius=None):
    offs, peers, po, rows, oo, om, counters = res
    kept_in = int(po[-1])
    w_oo, w_om, w_cnt = interest.peer_budget_np(po, rows, pos, peer_pos, k=k)
    assert w_cnt["n_in"] == kept_in and w_cnt["rows_cut"] > 0 and w_cnt["n_kept"] < kept_in   # budgets bite
    assert counters == w_cnt
    assert oo.tobytes() == w_oo.tobytes() and om.tobytes() == w_om.tobytes()
    lens = np.diff(po.astype(np.int64))
    for p in np.flatnonzero(lens > k)[:200]:        # every cut row's kept keys are <= its dropped ones
        row = rows[po[p]:po[p + 1]]
        d2 = interest.budget_keys_np(row, pos, peer_pos, int(p))
        kept = interest.budget_keys_np(om[oo[p]:oo[p + 1]], pos, peer_pos, int(p))
        assert len(kept) == k and kept.max() <= np.sort(d2)[k:].min()
        if radius is not None:
            assert (kept <= radius * radius).all()
    if radius is not None:                          # every kept pair satisfies the radius predicate
        p_of = np.repeat(np.arange(len(oo) - 1), np.diff(oo.astype(np.int64)))
        d = pos[om] - peer_pos[p_of]
        assert (((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= radius * radius).all()


def test_c5_tick_peer_major_budget():
    """About 20k moving entities with the radius filter on: tick, transpose, budget on one stream."""
    from worldql_server_amd.router import Router
    c5 = synth_ext.config_c5(scale=0.02)
    n = c5.n
    r = Router(16, 0)
    r.apply_ops(c5.initial_ops())
    r.set_radius(c5.radius)
    r.set_peer_positions(c5.pos)
    pos, world, sender, repl = c5.messages()
    res = _pipeline(r, pos, world, sender, repl, n, 16 * n, k=1)
    assert int(res[0][-1]) <= 16 * n
    _check_pipeline(res, pos, c5.pos, 1, radius=c5.radius)
    r.route_health()
    r.close()


def test_c3_tick_peer_major_budget():
    """About 50k messages around hotspots, 5k peers: rows from 0 to thousands of messages, K = 32."""
    from worldql_server_amd.router import Router
    scale = 0.005
    w = synth_ext.config_c3(scale=scale)
    peer_pos = synth_ext.hotspot_positions(3, 1, w.n_peers, 4096.0 * scale ** (1.0 / 3.0), 256,
                                           128.0 * scale ** (1.0 / 3.0))
    r = Router(16, 0)
    r.apply_ops(w.ops)
    r.set_peer_positions(peer_pos)
    P = len(r.route(w.pos, w.world, w.sender, w.repl)[1])
    res = _pipeline(r, w.pos, w.world, w.sender, w.repl, w.n_peers, P, k=32)
    assert int(np.diff(res[2].astype(np.int64)).max()) > 256          # long rows: the radix select runs
    _check_pipeline(res, w.pos, peer_pos, 32)
    r.route_health()
    r.close()


def test_cut_tick_through_peer_major_into_budget():
    """A tick into a buffer that ends inside a hot-cube message (capacity below P), transposed and
    budgeted with n_in = capacity: in bounds, and the definition's result on the transposed rows."""
    import test_gpu_truncation as tr
    w = tr.workload()
    r = tr.mk_router(w)
    r.set_peer_positions(w.peer_pos)
    P = len(r.route(w.pos, w.world, w.sender, w.repl)[1])
    cap = P // 2
    res = _pipeline(r, w.pos, w.world, w.sender, w.repl, w.n_peers, cap, k=5)
    assert int(res[0][-1]) > cap                                        # the tick was cut
    _check_pipeline(res, w.pos, w.peer_pos, 5)
    assert r.route_health()[1] == 1                                     # the tick's sticky overflow, read here
    r.close()


# ---- arguments ------------------------------------------------------------------------------

def test_invalid_arguments():
    from worldql_server_amd.router import Router, WQError, load_library
    c = cases()["len_edges_k64"]
    call = Call(c)
    r = Router(16, 0)

    def invalid(**kw):
        a = dict(peer_offsets_ptr=call.off.ptr, msgs_ptr=call.msgs.ptr, n_peers=c.n_peers, n_in=call.n_in,
                 msg_pos_ptr=call.mpos.ptr, n_msgs=len(c.msg_pos), peer_pos_ptr=call.ppos.ptr,
                 n_peer_pos=len(c.peer_pos), k=c.k, budget_ptr=None, out_offsets_ptr=call.oo.ptr,
                 out_msgs_ptr=call.om.ptr, counters_ptr=call.cnt.ptr)
        a.update(kw)
        with pytest.raises(WQError) as e:
            r.peer_budget_device(**a)
        assert e.value.code == abi.WQ_E_INVALID

    invalid(peer_pos_ptr=None, n_peer_pos=0)            # the handle has no positions
    invalid(peer_pos_ptr=None)                          # half given: a count without an array
    invalid(msgs_ptr=None)
    invalid(out_msgs_ptr=None)
    invalid(peer_offsets_ptr=None)
    invalid(out_offsets_ptr=None)
    invalid(msg_pos_ptr=None)
    invalid(n_in=1 << 32)
    invalid(n_peers=0xFFFFFFFF)                         # the header's limit: n_peers < 2^32 - 1
    lib = load_library()
    assert lib.wq_peer_budget_device(None, None, None, 0, 0, None, 0, None, 0, 0, None, ctypes.c_void_p(call.oo.ptr),
                                     None, None) == abi.WQ_E_INVALID
    import torch
    torch.cuda.synchronize()
    for a in (call.oo, call.om, call.cnt):
        assert a.unchanged()                            # nothing was launched
    # with positions in the handle the same call runs; a missing peer then has none
    r.set_peer_positions(c.peer_pos)
    hp = Call(c, handle_positions=True)
    check("len_edges_k64", *hp.run(r))
    r.close()


@pytest.mark.parametrize("mode", ["cube", "replicate"])
def test_multi_gpu_handle(mode):
    """A handle over two sub-handles (G = 2 on device 0): explicit positions run on its own stream and
    match the single handle; NULL positions are refused, set_peer_positions or not."""
    from worldql_server_amd.router import Router, WQError
    r = Router.multi(16, (0, 0), mode=mode)
    for name in ("len_edges_k64", "budget_array", "keys_nan_position_700"):
        run_case(r, name)
    c = cases()["len_edges_k64"]
    r.set_peer_positions(c.peer_pos)
    call = Call(c, handle_positions=True)
    with pytest.raises(WQError) as e:
        call.launch(r)
    assert e.value.code == abi.WQ_E_INVALID
    r.close()


def test_tracker_chains_budget_after_peer_major():
    """InterestTracker.peer_budget on the lists peer_major returned."""
    from worldql_server_amd.router import Router
    c5 = synth_ext.config_c5(scale=0.005)
    n = c5.n
    r = Router(16, 0)
    r.set_radius(c5.radius)
    r.follow_peers(np.zeros(n, np.uint32), c5.pos)
    r.set_peer_positions(c5.pos)
    tracker = interest.InterestTracker(r, n, 16 * n)
    pos, w, s, rp = c5.messages()
    d = [_dev(x) for x in (pos, w, s, rp)]
    tracker.route(*(x.data_ptr() for x in d))
    po, rows = tracker.peer_major("entered", None, n)
    oo, om = tracker.peer_budget(po, rows, d[0].data_ptr(), k=1)
    w_oo, w_om, w_cnt = interest.peer_budget_np(_u32(po), _u32(rows), pos, c5.pos, k=1)
    assert w_cnt["rows_cut"] > 0
    assert _u32(oo).tobytes() == w_oo.tobytes() and _u32(om).tobytes() == w_om.tobytes()
    r.route_health()
    r.close()
