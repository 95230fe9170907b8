"""GPU parity for the byte budgets (include/wq_router.h wq_peer_budget_bytes_device, csrc/wq_budget.hip):
of every peer's send list the nearest messages whose sizes fit in W bytes, in input order.

Bars, all bit-exact against worldql_server_amd/interest.py peer_budget_bytes_np (the shared case list of
tests/test_peer_budget_bytes_host.py, where the definition itself is checked against a restatement):
  - d_out_offsets[0 .. n_peers], d_out_msgs[0 .. n_kept), d_out_bytes[0 .. n_peers) and the counters are
    the definition's bytes, for ascending offsets and for hostile ones;
  - the guarded arrays of tests/test_gpu_peer_budget.py: every device array is sized exactly, with FRONT
    canary words before it and SLACK behind it; the guards of every output, d_out_msgs behind n_kept and
    every input are as they were;
  - every case runs twice on one handle, and the largest after the smallest, so stale scratch and
    histograms that were not left zero show;
  - a count-budget call between two byte-budget calls on one handle, nothing waited for in between:
    all three exact, so the two share no live state;
  - the count budget's output fed to the byte budget without leaving the device is "rank < B and
    running bytes <= W"."""
import ctypes

import numpy as np
import pytest

from worldql_server_amd import abi, interest, synth_ext

import test_gpu_peer_budget as count_gpu
import test_peer_budget_host as count_host
from test_gpu_peer_budget import CANARY, FRONT, SLACK, Guarded
from test_peer_budget_bytes_host import cases, exact_names, hostile_names, restated, want, well_formed

pytestmark = pytest.mark.gpu

DT = abi.BUDGET_BYTES_COUNTERS_DTYPE
CANARY64 = (CANARY << 32) | CANARY


class Call:
    """One case on the device: guarded inputs and outputs, and the checks after a call."""

    def __init__(self, c, device="cuda:0", handle_positions=False, with_bytes=True, with_counters=True):
        self.c, self.n_in = c, len(c.msgs)
        self.handle_positions = handle_positions
        g = lambda a: Guarded(a, device=device)
        self.off, self.msgs, self.mpos, self.ppos = g(c.offsets), g(c.msgs), g(c.msg_pos), g(c.peer_pos)
        self.msize = g(c.msg_size)
        self.budget = g(c.budget) if c.budget is not None else None
        self.oo = Guarded(n=c.n_peers + 1, device=device)
        self.om = Guarded(n=self.n_in, device=device)
        self.ob = Guarded(n=2 * c.n_peers, device=device) if with_bytes else None
        self.cnt = Guarded(n=10, device=device) if with_counters else None

    def launch(self, r):
        """Enqueues the call; nothing is waited for."""
        c = self.c
        explicit = not self.handle_positions
        r.peer_budget_bytes_device(self.off.ptr, self.msgs.ptr if self.n_in else None, c.n_peers, self.n_in,
                                   self.mpos.ptr if len(c.msg_pos) else None,
                                   self.msize.ptr if len(c.msg_pos) else None, len(c.msg_pos),
                                   self.ppos.ptr if explicit else None, len(c.peer_pos) if explicit else 0, c.w,
                                   self.budget.ptr if self.budget is not None else None, self.oo.ptr,
                                   self.om.ptr if self.n_in else None, self.ob.ptr if self.ob else None,
                                   self.cnt.ptr if self.cnt else None)

    def outputs(self):
        """(out_offsets, out_msgs[:n_kept], out_bytes or None, counters or None) after the canary checks."""
        import torch
        torch.cuda.synchronize()
        c = self.c
        oo, om = self.oo.read(), self.om.read()
        assert (oo[c.n_peers + 1:] == CANARY).all(), "written behind d_out_offsets[n_peers]"
        n_kept = int(oo[c.n_peers])
        assert n_kept <= self.n_in
        assert (om[n_kept:] == CANARY).all(), "written behind d_out_msgs[n_kept)"
        counters = ob = None
        if self.cnt:
            cnt = self.cnt.read(np.uint8)[:40].view(DT)[0]
            counters = {k: int(cnt[k]) for k in DT.names}
            assert counters["n_kept"] == n_kept
            assert (self.cnt.read()[10:] == CANARY).all(), "written behind the counters"
        if self.ob:
            ob = self.ob.read(np.uint64)
            assert (ob[c.n_peers:] == CANARY64).all(), "written behind d_out_bytes[n_peers)"
            ob = ob[:c.n_peers]
        for a, what in ((self.oo, "d_out_offsets"), (self.om, "d_out_msgs"), (self.ob, "d_out_bytes"),
                        (self.cnt, "the counters")):
            assert a is None or a.front_intact(), "written before " + what
        for a in (self.off, self.msgs, self.mpos, self.msize, self.ppos, self.budget):
            assert a is None or a.unchanged(), "an input was written"
        return oo[:c.n_peers + 1], om[:n_kept], ob, counters

    def run(self, r):
        import torch
        torch.cuda.synchronize()
        self.launch(r)
        return self.outputs()


def check(name, oo, om, ob, counters):
    w_oo, w_om, w_ob, w_cnt = want(name)
    assert counters is None or counters == w_cnt, name
    assert oo.tobytes() == w_oo.tobytes(), (name, "offsets")
    assert om.tobytes() == w_om.tobytes(), (name, "messages")
    assert ob is None or ob.tobytes() == w_ob.tobytes(), (name, "bytes")
    well_formed(cases()[name], oo, om, ob, counters)


def run_case(r, name, device="cuda:0"):
    check(name, *Call(cases()[name], device).run(r))


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    yield r
    r.close()


LARGEST = max(cases(), key=lambda n: len(cases()[n].msgs))


# ---- the shared cases ---------------------------------------------------------------------

@pytest.mark.parametrize("name", exact_names())
def test_exact_on_the_shared_cases(router, name):
    """Twice on one handle (the second call sees the first one's scratch and histograms)."""
    run_case(router, name)
    run_case(router, name)


@pytest.mark.parametrize("name", hostile_names())
def test_hostile_offsets(router, name):
    """Descending, wrapped and overlapping offsets: in bounds, error bit 0, the definition's result for
    the rows the header describes, twice."""
    first = Call(cases()[name]).run(router)
    assert first[3]["error"] & abi.BUDGET_ERROR_ROWS
    check(name, *first)
    run_case(router, name)


def test_stale_scratch_largest_after_smallest():
    """A fresh handle: the smallest cases, the largest one, and small ones again."""
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    for name in ("size_nothing", "w_zero", LARGEST, "w_zero", "mid_tile_w150", "huge_sizes", "size_no_elements",
                 "ties_all_equal", LARGEST):
        run_case(r, name)
    r.close()


def test_count_budget_between_two_byte_budgets(router):
    """Byte budget, count budget, byte budget on one handle and stream, nothing waited for in between."""
    import torch
    a, b = Call(cases()["mid_tile_w20000"]), Call(cases()["zero_sizes_at_cut"])
    k = count_gpu.Call(count_host.cases()["len_edges_k64"])
    torch.cuda.synchronize()
    a.launch(router)
    k.launch(router)
    b.launch(router)
    check("mid_tile_w20000", *a.outputs())
    count_gpu.check("len_edges_k64", *k.outputs())
    check("zero_sizes_at_cut", *b.outputs())
    for call, name in ((k, None), (a, "mid_tile_w20000"), (k, None), (b, "zero_sizes_at_cut")):   # and alternating
        if name is None:
            count_gpu.check("len_edges_k64", *call.run(router))
        else:
            check(name, *call.run(router))


@pytest.mark.parametrize("name", ["mid_tile_w20000", "budget_array", "size_no_elements"])
def test_nullable_outputs(router, name):
    """d_out_bytes NULL and d_counters NULL leave the other outputs identical."""
    c = cases()[name]
    for with_bytes, with_counters in ((False, True), (True, False), (False, False)):
        check(name, *Call(c, with_bytes=with_bytes, with_counters=with_counters).run(router))


def test_steady_state_allocates_nothing(router):
    """As the count budget's test: after one call has grown the scratch, the next call of the same size
    and a smaller one, and a count-budget call between them, leave the device's free memory as it was
    (hipMemGetInfo, which other processes move too: a lower figure fails, a higher one is measured again)."""
    import torch
    call, small = Call(cases()[LARGEST]), Call(cases()["w_zero"])
    k = count_gpu.Call(count_host.cases()["len_edges_k64"])
    call.run(router)
    k.run(router)
    for _ in range(5):
        free = torch.cuda.mem_get_info()[0]
        check(LARGEST, *call.run(router))
        k.run(router)
        small.run(router)
        after = torch.cuda.mem_get_info()[0]
        assert after >= free, ("a steady-state call allocated", free - after)
        if after == free:
            return
    pytest.fail("the device's free memory kept rising: no quiet pair in five")


# ---- composition ----------------------------------------------------------------------------

@pytest.mark.parametrize("name,B,W", [("len_edges_w3000", 64, 12000), ("zero_sizes_at_cut", 100, 90000),
                                      ("huge_sizes", 30, 20 * 0xFFFFFFFF)])
def test_count_budget_feeds_byte_budget_on_the_device(router, name, B, W):
    """wq_peer_budget_device's outputs are wq_peer_budget_bytes_device's inputs, nothing read in between:
    exactly the elements with rank < B and running bytes <= W."""
    import torch
    c = cases()[name]
    n_in = len(c.msgs)
    g = lambda a: Guarded(a)
    off, msgs, mpos, ppos, msize = g(c.offsets), g(c.msgs), g(c.msg_pos), g(c.peer_pos), g(c.msg_size)
    o1, m1 = Guarded(n=c.n_peers + 1), Guarded(n=n_in)
    o2, m2, b2, cnt = Guarded(n=c.n_peers + 1), Guarded(n=n_in), Guarded(n=2 * c.n_peers), Guarded(n=10)
    torch.cuda.synchronize()
    router.peer_budget_device(off.ptr, msgs.ptr, c.n_peers, n_in, mpos.ptr, len(c.msg_pos), ppos.ptr, len(c.peer_pos), B,
                              None, o1.ptr, m1.ptr, None)
    router.peer_budget_bytes_device(o1.ptr, m1.ptr, c.n_peers, n_in, mpos.ptr, msize.ptr, len(c.msg_pos), ppos.ptr,
                                    len(c.peer_pos), W, None, o2.ptr, m2.ptr, b2.ptr, cnt.ptr)
    torch.cuda.synchronize()
    r_oo, r_om, r_ob = restated(c, [W] * c.n_peers, B)
    oo, om, ob = o2.read(), m2.read(), b2.read(np.uint64)
    assert oo[:c.n_peers + 1].tobytes() == r_oo.tobytes() and (oo[c.n_peers + 1:] == CANARY).all()
    assert om[:len(r_om)].tobytes() == r_om.tobytes() and (om[len(r_om):] == CANARY).all()
    assert ob[:c.n_peers].tobytes() == r_ob.tobytes() and (ob[c.n_peers:] == CANARY64).all()
    counters = cnt.read(np.uint8)[:40].view(DT)[0]
    assert int(counters["n_in"]) == int(o1.read()[c.n_peers]) and int(counters["n_kept"]) == len(r_om)
    assert int(counters["bytes_kept"]) == sum(int(v) for v in r_ob) and int(counters["error"]) == 0
    for a in (o2, m2, b2, cnt, o1, m1):
        assert a.front_intact()
    assert 0 < len(r_om) < int(o1.read()[c.n_peers]) < n_in


# ---- arguments ------------------------------------------------------------------------------

def test_invalid_arguments():
    from worldql_server_amd.router import Router, WQError, load_library
    c = cases()["len_edges_w3000"]
    call = Call(c)
    r = Router(16, 0)

    def invalid(**kw):
        a = dict(peer_offsets_ptr=call.off.ptr, msgs_ptr=call.msgs.ptr, n_peers=c.n_peers, n_in=call.n_in,
                 msg_pos_ptr=call.mpos.ptr, msg_size_ptr=call.msize.ptr, n_msgs=len(c.msg_pos),
                 peer_pos_ptr=call.ppos.ptr, n_peer_pos=len(c.peer_pos), w=c.w, budget_bytes_ptr=None,
                 out_offsets_ptr=call.oo.ptr, out_msgs_ptr=call.om.ptr, out_bytes_ptr=call.ob.ptr,
                 counters_ptr=call.cnt.ptr)
        a.update(kw)
        with pytest.raises(WQError) as e:
            r.peer_budget_bytes_device(**a)
        assert e.value.code == abi.WQ_E_INVALID

    invalid(msg_size_ptr=None)                          # required when n_msgs > 0
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
    assert lib.wq_peer_budget_bytes_device(None, None, None, 0, 0, None, None, 0, None, 0, 0, None,
                                           ctypes.c_void_p(call.oo.ptr), None, None, None) == abi.WQ_E_INVALID
    import torch
    torch.cuda.synchronize()
    for a in (call.oo, call.om, call.ob, call.cnt):
        assert a.unchanged()                            # nothing was launched
    # with positions in the handle the same call runs and agrees with the explicit positions
    r.set_peer_positions(c.peer_pos)
    for name in ("len_edges_w3000", "missing_peer_positions"):
        cc = cases()[name]
        r.set_peer_positions(cc.peer_pos)
        hp = Call(cc, handle_positions=True).run(r)
        check(name, *hp)
        ex = Call(cc).run(r)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(hp[:3], ex[:3])) and hp[3] == ex[3]
    r.close()


@pytest.mark.parametrize("mode", ["cube", "replicate"])
def test_multi_gpu_handle(mode):
    """A handle over two sub-handles (G = 2 on device 0): explicit positions run on its own stream and
    match the single handle; NULL positions are refused, set_peer_positions or not."""
    from worldql_server_amd.router import Router, WQError
    r = Router.multi(16, (0, 0), mode=mode)
    for name in ("len_edges_w3000", "budget_array", "huge_sizes"):
        run_case(r, name)
    c = cases()["len_edges_w3000"]
    r.set_peer_positions(c.peer_pos)
    call = Call(c, handle_positions=True)
    with pytest.raises(WQError) as e:
        call.launch(r)
    assert e.value.code == abi.WQ_E_INVALID
    r.close()


def test_tracker_chains_byte_budget_after_peer_major():
    """InterestTracker.peer_budget_bytes on the lists peer_major returned, sizes from frame_sizes."""
    import torch
    from worldql_server_amd.router import Router
    c5 = synth_ext.config_c5(scale=0.005)
    n = c5.n
    r = Router(16, 0)
    r.set_radius(c5.radius)
    r.follow_peers(np.zeros(n, np.uint32), c5.pos)
    r.set_peer_positions(c5.pos)
    tracker = interest.InterestTracker(r, n, 16 * n)
    pos, w, s, rp = c5.messages()
    d = [count_gpu._dev(x) for x in (pos, w, s, rp)]
    tracker.route(*(x.data_ptr() for x in d))
    po, rows = tracker.peer_major("entered", None, n)
    frames = np.zeros(n + 1, np.uint64)
    np.cumsum(np.random.default_rng(3).integers(100, 201, size=n), out=frames[1:])
    sizes = interest.frame_sizes(frames)
    d_sizes = count_gpu._dev(sizes)
    oo, om, ob = tracker.peer_budget_bytes(po, rows, d[0].data_ptr(), d_sizes.data_ptr(), w=300)
    w_oo, w_om, w_ob, w_cnt = interest.peer_budget_bytes_np(count_gpu._u32(po), count_gpu._u32(rows), pos, sizes, c5.pos,
                                                            w=300)
    assert w_cnt["rows_cut"] > 0 and w_cnt["n_kept"] > 0
    assert count_gpu._u32(oo).tobytes() == w_oo.tobytes() and count_gpu._u32(om).tobytes() == w_om.tobytes()
    assert ob.cpu().numpy().view(np.uint64).tobytes() == w_ob.tobytes()
    r.route_health()
    r.close()
