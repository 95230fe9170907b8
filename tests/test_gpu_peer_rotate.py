"""GPU parity for the fair share (include/wq_router.h wq_peer_rotate_device, csrc/wq_rotate.hip): the
budget's output plus, per peer, the cut elements that follow the peer's cursor in cyclic order.

Bars, all bit-exact against worldql_server_amd/interest.py peer_rotate_np (the shared case list of
tests/test_peer_rotate_host.py, where the definition itself is checked against a restatement):
  - d_out_offsets[0 .. n_peers], d_out_msgs[0 .. n_out), d_cursor[0 .. n_peers), d_out_bytes and the
    counters are the definition's bytes on every exact case and on every hostile one whose rows ascend;
    the other hostile cases are well formed and give the same bytes twice;
  - every device array is sized exactly, with FRONT guard words before it and SLACK behind it, all
    holding a canary (Guarded, from tests/test_gpu_peer_budget.py): the words around every output and
    around (and inside) every input are as they were;
  - every case runs twice on one handle, and the largest after the smallest, so stale scratch shows;
  - budget -> rotate -> pack for six ticks on one handle with nothing waited for in between, the
    cursors left on the device, is the host chain's bytes, and every pair that stayed cut arrives;
  - the budgets interleave with the call on one handle: the shared scratch holds no live state.
Nothing here provokes a fault: hostile inputs are hostile values inside exactly sized, guarded arrays."""
import ctypes

import numpy as np
import pytest

from worldql_server_amd import abi, interest

import test_gpu_peer_budget as count_gpu
import test_gpu_peer_budget_bytes as bytes_gpu
import test_peer_budget_bytes_host as bytes_host
import test_peer_budget_host as count_host
from test_gpu_peer_budget import CANARY, Guarded
from test_peer_rotate_host import cases, exact_names, hostile_names, rows_ascend, want, well_formed

pytestmark = pytest.mark.gpu

DT = abi.ROTATE_COUNTERS_DTYPE
NAMES = [n for n in DT.names if n != "pad_"]
CANARY64 = (CANARY << 32) | CANARY
LARGEST = max(cases(), key=lambda n: len(cases()[n].msgs))
SMALLEST = "size_nothing"


class Call:
    """One case on the device: guarded inputs, cursors and outputs, and the checks after a call."""

    def __init__(self, c, device="cuda:0", with_bytes=True, with_counters=True):
        self.c, self.n_in, self.n_kin = c, len(c.msgs), len(c.kmsgs)
        self.sizes = c.msg_size is not None
        g = lambda a: Guarded(a, device=device) if a is not None else None
        self.off, self.msgs, self.koff, self.kmsgs = g(c.offsets), g(c.msgs), g(c.koffsets), g(c.kmsgs)
        self.msize, self.extra, self.extra_bytes = g(c.msg_size), g(c.extra), g(c.extra_bytes)
        self.cursor = Guarded(c.cursor, device=device)
        self.oo = Guarded(n=c.n_peers + 1, device=device)
        self.om = Guarded(n=self.n_in, device=device)
        self.ob = Guarded(n=2 * c.n_peers, device=device) if with_bytes and self.sizes else None
        self.cnt = Guarded(n=16, device=device) if with_counters else None

    def launch(self, r):
        """Enqueues the call; nothing is waited for."""
        c = self.c
        r.peer_rotate_device(self.off.ptr, self.msgs.ptr if self.n_in else None, c.n_peers, self.n_in,
                             self.koff.ptr, self.kmsgs.ptr if self.n_kin else None, self.n_kin,
                             self.msize.ptr if self.sizes else None,          # non-NULL with n_msgs 0: sizes, all 0
                             len(c.msg_size) if self.sizes else 0, c.r, self.extra.ptr if self.extra else None, c.v,
                             self.extra_bytes.ptr if self.extra_bytes else None,
                             self.cursor.ptr if c.n_peers else None, self.oo.ptr, self.om.ptr if self.n_in else None,
                             self.ob.ptr if self.ob else None, self.cnt.ptr if self.cnt else None)

    def outputs(self):
        """(out_offsets, out_msgs[:n_out], out_bytes or None, cursors, counters or None) after the canary
        checks on every array."""
        import torch
        torch.cuda.synchronize()
        c = self.c
        oo, om, cursor = self.oo.read(), self.om.read(), self.cursor.read()
        assert (oo[c.n_peers + 1:] == CANARY).all(), "written behind d_out_offsets[n_peers]"
        n_out = int(oo[c.n_peers])
        assert n_out <= self.n_in
        assert (om[n_out:] == CANARY).all(), "written behind d_out_msgs[n_out)"
        assert (cursor[c.n_peers:] == CANARY).all(), "written behind d_cursor[n_peers)"
        counters = ob = None
        if self.cnt:
            cnt = self.cnt.read(np.uint8)[:64].view(DT)[0]
            counters = {k: int(cnt[k]) for k in NAMES}
            assert counters["n_out"] == n_out and int(cnt["pad_"]) == 0
            assert (self.cnt.read()[16:] == CANARY).all(), "written behind the counters"
        if self.ob:
            ob = self.ob.read(np.uint64)
            assert (ob[c.n_peers:] == CANARY64).all(), "written behind d_out_bytes[n_peers)"
            ob = ob[:c.n_peers]
        for a, what in ((self.oo, "d_out_offsets"), (self.om, "d_out_msgs"), (self.ob, "d_out_bytes"),
                        (self.cursor, "d_cursor"), (self.cnt, "the counters")):
            assert a is None or a.front_intact(), "written before " + what
        for a in (self.off, self.msgs, self.koff, self.kmsgs, self.msize, self.extra, self.extra_bytes):
            assert a is None or a.unchanged(), "an input was written"
        return oo[:c.n_peers + 1], om[:n_out], ob, cursor[:c.n_peers], counters

    def run(self, r):
        import torch
        torch.cuda.synchronize()
        self.launch(r)
        return self.outputs()


def check(name, oo, om, ob, cursor, counters):
    w_oo, w_om, w_ob, w_cursor, w_cnt = want(name)
    assert counters is None or counters == w_cnt, name
    assert oo.tobytes() == w_oo.tobytes(), (name, "offsets")
    assert om.tobytes() == w_om.tobytes(), (name, "messages")
    assert cursor.tobytes() == w_cursor.tobytes(), (name, "cursors")
    assert ob is None or ob.tobytes() == w_ob.tobytes(), (name, "bytes")
    well_formed(cases()[name], oo, om, cursor, counters)


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
    """Twice on one handle (the second call sees the first one's scratch), from the same cursors."""
    run_case(router, name)
    run_case(router, name)


@pytest.mark.parametrize("name", hostile_names())
def test_hostile_input(router, name):
    """Descending, wrapped and overlapping offsets in either CSR, arrays cut short, rows that do not
    ascend: in bounds, well formed, the same bytes twice; the definition's bytes where the rows ascend."""
    c = cases()[name]
    first = Call(c).run(router)
    well_formed(c, first[0], first[1], first[3], first[4])
    again = Call(c).run(router)
    for a, b in zip(first[:4], again[:4]):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    assert first[4] == again[4]
    if rows_ascend(c):
        check(name, *first)


def test_stale_scratch_largest_after_smallest():
    """A fresh handle: the smallest cases, the largest one, and small ones again."""
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    assert len(cases()[SMALLEST].msgs) == 0 and len(cases()[LARGEST].msgs) >= 70_000
    for name in (SMALLEST, "repeats_small", LARGEST, "repeats_small", "lens_kept_some_sizes", "long_row_70000_sizes",
                 "size_no_elements", "cursor_places_r3", "long_row_5000_rmax", LARGEST):
        run_case(r, name)
    r.close()


@pytest.mark.parametrize("name", ["lens_kept_some_sizes", "after_byte_budget", "size_nothing"])
def test_nullable_outputs(router, name):
    c = cases()[name]
    for with_bytes, with_counters in ((False, True), (True, False), (False, False)):
        check(name, *Call(c, with_bytes=with_bytes, with_counters=with_counters).run(router))


def test_steady_state_allocates_nothing(router):
    """After one call has grown the scratch, the very next call of the same size and a smaller one
    leave the device's free memory as it was (read as in tests/test_gpu_peer_budget.py: a lower figure
    fails at once, a higher one, which another process alone can cause, is measured again)."""
    import torch
    big, small = "long_row_70000_sizes", "lens_kept_some_sizes"
    Call(cases()[big]).run(router)
    for _ in range(5):
        call, other = Call(cases()[big]), Call(cases()[small])
        torch.cuda.synchronize()
        free = torch.cuda.mem_get_info()[0]
        check(big, *call.run(router))
        other.run(router)
        after = torch.cuda.mem_get_info()[0]
        assert after >= free, ("a steady-state call allocated", free - after)
        if after == free:
            return
    pytest.fail("the device's free memory kept rising: no quiet pair in five")


def test_budgets_interleaved_with_rotate_calls(router):
    """A count-budget call and a byte-budget call between rotate calls on one handle and stream, nothing
    waited for in between, and then alternating: the shared scratch holds no live state."""
    import torch
    a, b = Call(cases()["after_byte_budget"]), Call(cases()["long_row_5000_sizes"])
    c = Call(cases()["lens_kept_some_extra_T"])
    k = count_gpu.Call(count_host.cases()["len_edges_k64"])
    w = bytes_gpu.Call(bytes_host.cases()["mid_tile_w20000"])
    torch.cuda.synchronize()
    a.launch(router)
    k.launch(router)
    b.launch(router)
    w.launch(router)
    c.launch(router)
    check("after_byte_budget", *a.outputs())
    count_gpu.check("len_edges_k64", *k.outputs())
    check("long_row_5000_sizes", *b.outputs())
    bytes_gpu.check("mid_tile_w20000", *w.outputs())
    check("lens_kept_some_extra_T", *c.outputs())
    for name in ("after_count_budget_sizes", "repeats_long_sizes", "long_row_5000"):
        count_gpu.check("len_edges_k64", *k.run(router))
        run_case(router, name)
        bytes_gpu.check("mid_tile_w20000", *w.run(router))
        run_case(router, name)


# ---- the chain ------------------------------------------------------------------------------

TICKS, K, R = 6, 8, 3
N_PEERS, N_MSGS = 300, 400


def _chain_workload():
    """One crowd: 300 peers and 400 messages in a box, positions jittered every tick. Peer p's list is
    its K + 1 + p % 12 nearest messages, ascending, so every list exceeds K and T = 1 + p % 12 <= 12: a
    fixed list is through after ceil(12 / 3) = 4 ticks, which leaves two ticks, six chosen elements, for
    the entities that the jitter moves into a list ahead of the cursor."""
    rng = np.random.default_rng(77)
    mpos0, ppos0 = rng.random((N_MSGS, 3)) * 40.0, rng.random((N_PEERS, 3)) * 40.0
    fo = np.zeros(N_MSGS + 1, np.uint64)
    np.cumsum(rng.integers(1, 60, size=N_MSGS), out=fo[1:])
    frames = rng.integers(0, 256, size=int(fo[-1]), dtype=np.uint8)
    ticks = []
    for _ in range(TICKS):
        mpos = mpos0 + rng.normal(0.0, 0.4, size=mpos0.shape)
        ppos = ppos0 + rng.normal(0.0, 0.4, size=ppos0.shape)
        d = mpos[None, :, :] - ppos[:, None, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        order = np.argsort(d2, axis=1, kind="stable")
        rows = [np.sort(order[p, :K + 1 + p % 12]).astype(np.uint32) for p in range(N_PEERS)]
        off = np.zeros(N_PEERS + 1, np.uint32)
        np.cumsum([len(x) for x in rows], out=off[1:])
        ticks.append((off, np.concatenate(rows), np.ascontiguousarray(mpos), np.ascontiguousarray(ppos)))
    return ticks, frames, fo


def test_six_ticks_budget_rotate_pack_on_one_stream():
    """wq_peer_budget_device -> wq_peer_rotate_device -> wq_peer_pack_device, six ticks enqueued back to
    back on one handle, the cursor array left on the device: every tick's three outputs and the final
    cursors are the host chain's, and every (peer, message) pair that stayed in the list for all six
    ticks appears in some tick's packed run (T <= 12 <= 18 = 6 R for every list, see _chain_workload)."""
    import torch
    from worldql_server_amd.router import Router
    ticks, frames, fo = _chain_workload()
    # the host chain
    cursor = np.full(N_PEERS, abi.ROTATE_CURSOR_START, np.uint32)
    host, sent = [], [set() for _ in range(N_PEERS)]
    for off, msgs, mpos, ppos in ticks:
        ko, km, _ = interest.peer_budget_np(off, msgs, mpos, ppos, k=K)
        assert (np.diff(off.astype(np.int64)) > K).all() and (np.diff(off.astype(np.int64)) - K <= TICKS * R).all()
        oo, om, _, cnt = interest.peer_rotate_np(off, msgs, ko, km, cursor, r=R)
        assert cnt["error"] == 0 and cnt["rows_rotated"] == N_PEERS
        out, pb, _, pc = interest.peer_pack_np(oo, om, frames, fo)
        assert pc["error"] == 0
        host.append((ko, km, oo, om, out, pb))
        for p in range(N_PEERS):
            sent[p] |= set(om[oo[p]:oo[p + 1]].tolist())
    stayed = [set.intersection(*(set(m[o[p]:o[p + 1]].tolist()) for o, m, _, _ in ticks)) for p in range(N_PEERS)]
    assert sum(len(s) for s in stayed) > 5 * N_PEERS and len({t[1].tobytes() for t in ticks}) == TICKS   # lists change
    assert all(stayed[p] <= sent[p] for p in range(N_PEERS))
    # the device chain: everything uploaded first, then 18 calls, then one wait
    r = Router(16, 0)
    g = Guarded
    d_frames, d_fo = g(np.concatenate([frames, np.zeros(-len(frames) % 4, np.uint8)])), g(fo)
    d_cursor = g(np.full(N_PEERS, abi.ROTATE_CURSOR_START, np.uint32))
    dev = []
    for (off, msgs, mpos, ppos), (ko, km, oo, om, out, pb) in zip(ticks, host):
        n_in = len(msgs)
        dev.append(dict(off=g(off), msgs=g(msgs), mpos=g(mpos), ppos=g(ppos), ko=g(n=N_PEERS + 1), km=g(n=n_in),
                        oo=g(n=N_PEERS + 1), om=g(n=n_in), out=g(n=(len(out) + 3) // 4), pb=g(n=2 * (N_PEERS + 1)),
                        rcnt=g(n=16), pcnt=g(n=10)))
    torch.cuda.synchronize()
    for t, ((off, msgs, mpos, ppos), h) in zip(dev, zip(ticks, host)):
        n_in = len(msgs)
        r.peer_budget_device(t["off"].ptr, t["msgs"].ptr, N_PEERS, n_in, t["mpos"].ptr, N_MSGS, t["ppos"].ptr, N_PEERS, K,
                             None, t["ko"].ptr, t["km"].ptr, None)
        r.peer_rotate_device(t["off"].ptr, t["msgs"].ptr, N_PEERS, n_in, t["ko"].ptr, t["km"].ptr, n_in, None, 0, R, None,
                             0, None, d_cursor.ptr, t["oo"].ptr, t["om"].ptr, None, t["rcnt"].ptr)
        r.peer_pack_device(t["oo"].ptr, t["om"].ptr, N_PEERS, n_in, d_frames.ptr, d_fo.ptr, N_MSGS, len(frames), 0,
                           t["out"].ptr, 4 * ((len(h[4]) + 3) // 4), t["pb"].ptr, None, t["pcnt"].ptr)
    torch.cuda.synchronize()
    packed = [set() for _ in range(N_PEERS)]
    for i, (t, (ko, km, oo, om, out, pb)) in enumerate(zip(dev, host)):
        assert t["ko"].read()[:N_PEERS + 1].tobytes() == ko.tobytes(), (i, "budget offsets")
        assert t["km"].read()[:len(km)].tobytes() == km.tobytes(), (i, "budget messages")
        assert (t["km"].read()[len(km):] == CANARY).all()
        assert t["oo"].read()[:N_PEERS + 1].tobytes() == oo.tobytes(), (i, "rotate offsets")
        assert t["om"].read()[:len(om)].tobytes() == om.tobytes(), (i, "rotate messages")
        assert (t["om"].read()[len(om):] == CANARY).all() and (t["oo"].read()[N_PEERS + 1:] == CANARY).all()
        rc = t["rcnt"].read(np.uint8)[:64].view(DT)[0]
        assert int(rc["error"]) == 0 and int(rc["n_out"]) == len(om) and int(rc["n_chosen"]) == len(om) - len(km)
        pc = t["pcnt"].read(np.uint8)[:40].view(abi.PACK_COUNTERS_DTYPE)[0]
        assert int(pc["error"]) == 0 and int(pc["overflow"]) == 0 and int(pc["bytes_need"]) == len(out)
        raw = t["out"].read(np.uint8)
        assert raw[:len(out)].tobytes() == out.tobytes(), (i, "packed bytes")
        assert (t["out"].read()[(len(out) + 3) // 4:] == CANARY).all()
        d_pb = t["pb"].read(np.uint64)[:N_PEERS + 1]
        assert d_pb.tobytes() == pb.tobytes(), (i, "run starts")
        for a in t.values():
            assert a.front_intact()
        for a in (t["off"], t["msgs"], t["mpos"], t["ppos"]):
            assert a.unchanged()
        # what each peer's run holds, from the device's own offsets: frames differ in length only, so
        # the run's length against the list's frame sizes pins the list
        d_oo, d_om = t["oo"].read()[:N_PEERS + 1], t["om"].read()
        sizes = np.diff(fo).astype(np.int64)
        for p in range(N_PEERS):
            row = d_om[d_oo[p]:d_oo[p + 1]]
            assert int(d_pb[p + 1] - d_pb[p]) == int(sizes[row].sum())
            at = int(d_pb[p])
            for m in row.tolist():
                assert raw[at:at + int(sizes[m])].tobytes() == frames[int(fo[m]):int(fo[m + 1])].tobytes()
                at += int(sizes[m])
            packed[p] |= set(row.tolist())
    assert d_cursor.read()[:N_PEERS].tobytes() == cursor.tobytes(), "the final cursors"
    assert (d_cursor.read()[N_PEERS:] == CANARY).all() and d_cursor.front_intact()
    assert all(stayed[p] <= packed[p] for p in range(N_PEERS)), "a pair that stayed in the list never arrived"
    assert d_frames.unchanged() and d_fo.unchanged()
    r.close()


# ---- arguments ------------------------------------------------------------------------------

def test_invalid_arguments():
    from worldql_server_amd.router import Router, WQError, load_library
    c = cases()["lens_kept_some_sizes"]
    call = Call(c)
    r = Router(16, 0)

    def invalid(**kw):
        a = dict(peer_offsets_ptr=call.off.ptr, msgs_ptr=call.msgs.ptr, n_peers=c.n_peers, n_in=call.n_in,
                 kept_offsets_ptr=call.koff.ptr, kept_msgs_ptr=call.kmsgs.ptr, n_kept_in=call.n_kin,
                 msg_size_ptr=call.msize.ptr, n_msgs=len(c.msg_size), r=c.r, extra_ptr=None, v=c.v, extra_bytes_ptr=None,
                 cursor_ptr=call.cursor.ptr, out_offsets_ptr=call.oo.ptr, out_msgs_ptr=call.om.ptr,
                 out_bytes_ptr=call.ob.ptr, counters_ptr=call.cnt.ptr)
        a.update(kw)
        with pytest.raises(WQError) as e:
            r.peer_rotate_device(**a)
        assert e.value.code == abi.WQ_E_INVALID

    invalid(msgs_ptr=None)
    invalid(out_msgs_ptr=None)
    invalid(peer_offsets_ptr=None)
    invalid(kept_offsets_ptr=None)
    invalid(kept_msgs_ptr=None)
    invalid(out_offsets_ptr=None)
    invalid(cursor_ptr=None)
    invalid(msg_size_ptr=None)                          # d_out_bytes needs sizes
    invalid(n_in=1 << 32)
    invalid(n_kept_in=1 << 32)
    invalid(n_peers=0xFFFFFFFF)                         # the header's limit: n_peers < 2^32 - 1
    lib = load_library()
    assert lib.wq_peer_rotate_device(None, None, None, 0, 0, None, None, 0, None, 0, 0, None, 0, None, None,
                                     ctypes.c_void_p(call.oo.ptr), None, None, None) == abi.WQ_E_INVALID
    import torch
    torch.cuda.synchronize()
    for a in (call.oo, call.om, call.ob, call.cnt, call.cursor):
        assert a.unchanged()                            # nothing was launched
    check("lens_kept_some_sizes", *call.run(r))         # and the same arrays then run
    r.close()


@pytest.mark.parametrize("mode", ["cube", "replicate"])
def test_multi_gpu_handle(mode):
    """A handle over two sub-handles (G = 2 on device 0) runs the call on its own stream."""
    from worldql_server_amd.router import Router
    r = Router.multi(16, (0, 0), mode=mode)
    for name in ("lens_kept_some_sizes", "after_count_budget", "repeats_long_r50", "lens_kept_some_sizes"):
        run_case(r, name)
    r.close()


def test_tracker_owns_the_cursors():
    """InterestTracker.peer_rotate after peer_budget, into peer_pack, three ticks on the same lists: the
    cursors start at 0xFFFFFFFF, stay on the device and move."""
    import torch
    from worldql_server_amd.router import Router
    ticks, frames, fo = _chain_workload()
    off, msgs, mpos, ppos = ticks[0]
    r = Router(16, 0)
    r.set_peer_positions(ppos)
    tracker = interest.InterestTracker(r, N_MSGS, 1)
    _dev, _u32 = count_gpu._dev, count_gpu._u32
    d_off, d_msgs, d_mpos, d_fo = _dev(off), _dev(msgs), _dev(mpos), Guarded(fo)
    d_frames = Guarded(np.concatenate([frames, np.zeros(-len(frames) % 4, np.uint8)]))
    cursor = np.full(N_PEERS, abi.ROTATE_CURSOR_START, np.uint32)
    for _ in range(3):
        ko, km = tracker.peer_budget(d_off, d_msgs, d_mpos.data_ptr(), k=K)
        oo, om, ob = tracker.peer_rotate(d_off, d_msgs, ko, km, r=R)
        out, pb, eb = tracker.peer_pack(oo, om, d_frames.ptr, d_fo.ptr, len(frames))
        h_ko, h_km, _ = interest.peer_budget_np(off, msgs, mpos, ppos, k=K)
        w_oo, w_om, _, _ = interest.peer_rotate_np(off, msgs, h_ko, h_km, cursor, r=R)
        w_out, w_pb, _, _ = interest.peer_pack_np(w_oo, w_om, frames, fo)
        assert ob is None and _u32(oo).tobytes() == w_oo.tobytes() and _u32(om)[:len(w_om)].tobytes() == w_om.tobytes()
        assert _u32(tracker.cursor).tobytes() == cursor.tobytes()
        assert out.cpu().numpy().tobytes() == w_out.tobytes() and pb.cpu().numpy().astype(np.uint64).tobytes() == w_pb.tobytes()
    assert (cursor != abi.ROTATE_CURSOR_START).all()
    r.close()
