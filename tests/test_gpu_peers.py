"""GPU parity for per-peer send lists (PeerMap::broadcast_to,
worldql_server/src/transport/peer_map.rs:151-163): the transpose of a tick's CSR with the
disconnected peers dropped.

Bars, all bit-exact against worldql_server_amd/interest.py peer_major_np (the shared case list of
tests/test_peer_major_host.py, where the reference itself is checked against a brute force):
  - d_peer_offsets[0 .. n_peers] and the kept prefix of d_msgs_out are the reference's bytes;
  - d_msgs_out[kept .. n_pairs) holds row indices only (0 when there is no row);
  - every device array is SLACK words longer than the size passed and filled with a canary word that
    is no peer id, no message index and above every n_pairs: the words behind d_peer_offsets[n_peers],
    behind d_msgs_out[n_pairs] and behind (and inside) the inputs are as they were, so a kernel that
    ignored a bound fails an assertion here and does not touch foreign memory;
  - for offsets that do not ascend only the well-formedness clauses of include/wq_router.h, the
    canaries, and equal bytes from a second call.
"""
import numpy as np
import pytest

from worldql_server_amd import interest, synth

from test_peer_major_host import cases, exact_names, hostile_names, want, well_formed

pytestmark = pytest.mark.gpu

CANARY = 0xA5A5A5A5   # no peer id of an exact case's kept range, no message index, above every n_pairs
SLACK = 4096          # words behind every device array
ONES = 0xFFFFFFFF     # the guard words behind the bitmap: a bit read past its end says "connected"


def _expected(offs, peers, n_peers, connected):
    msg = np.repeat(np.arange(len(offs) - 1, dtype=np.uint32), np.diff(offs))
    on = peers < n_peers
    if connected is not None:
        on &= np.unpackbits(connected.view(np.uint8), bitorder="little")[np.minimum(peers, n_peers - 1)] == 1
    p, m = peers[on], msg[on]
    order = np.lexsort((m, p))  # by peer, then message
    p, m = p[order], m[order]
    po = np.searchsorted(p, np.arange(n_peers + 1), side="left").astype(np.uint32)
    return po, m


@pytest.mark.parametrize("frac_connected", [1.0, 0.7, 0.0])
def test_peer_major_matches_transpose(frac_connected):
    import torch
    from worldql_server_amd.router import Router
    w = synth.config_c2(repl_mode="mixed", scale=0.05)
    r = Router(16, 0)
    r.apply_ops(w.ops)
    offs, peers, _ = r.route(w.pos, w.world, w.sender, w.repl)
    M, P = len(offs) - 1, len(peers)
    n_peers = w.n_peers - 7  # a few recipients fall outside: dropped like disconnected peers
    rng = np.random.default_rng(4)
    connected = None
    if frac_connected < 1.0:
        bits = rng.random(((n_peers + 31) // 32) * 32) < frac_connected
        connected = np.packbits(bits, bitorder="little").view(np.uint32)
    dev = torch.device("cuda:0")
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    t_off = torch.from_numpy(offs.view(np.int32)).to(dev)
    t_peers = torch.from_numpy(peers.view(np.int32)).to(dev)
    t_conn = torch.from_numpy(connected.view(np.int32)).to(dev) if connected is not None else None
    po = torch.empty(n_peers + 1, dtype=torch.int32, device=dev)
    mo = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    r.peer_major_device(t_off.data_ptr(), t_peers.data_ptr(), M, P, t_conn.data_ptr() if t_conn is not None else None,
                        n_peers, po.data_ptr(), mo.data_ptr())
    torch.cuda.synchronize()
    want_po, want_m = _expected(offs, peers, n_peers, connected)
    got_po = po.cpu().numpy().view(np.uint32)
    assert (got_po == want_po).all()
    assert (mo.cpu().numpy().view(np.uint32)[:got_po[-1]] == want_m).all()
    if frac_connected == 0.0:
        assert got_po[-1] == 0
    else:
        assert got_po[-1] > 0
    # the shared host definition says the same
    ref_po, ref_m = interest.peer_major_np(offs, peers, n_peers, connected)
    assert ref_po.tobytes() == want_po.tobytes() and ref_m.tobytes() == want_m.astype(np.uint32).tobytes()
    r.set_stream(None)


# ---- harness ------------------------------------------------------------------------------

class Guarded:
    """A u32 device array of n words followed by SLACK guard words (the canary, or all ones)."""

    def __init__(self, data=None, n=None, guard=CANARY, device="cuda:0"):
        import torch
        n = len(data) if data is not None else n
        host = np.full(n + SLACK, guard, np.uint32)
        host[:n] = data if data is not None else CANARY
        self.n, self.host = n, host
        self.t = torch.from_numpy(host.view(np.int32)).to(device)
        self.ptr = self.t.data_ptr()

    def read(self):
        return self.t.cpu().numpy().view(np.uint32)

    def unchanged(self):
        return self.read().tobytes() == self.host.tobytes()


class Call:
    """One case on the device: guarded inputs and outputs, and the checks after a call."""

    def __init__(self, c, device="cuda:0"):
        self.c = c
        self.n_pairs = len(c.peers)
        assert self.n_pairs < CANARY and c.n_msgs < CANARY
        self.off = Guarded(c.offsets, device=device)
        self.peers = Guarded(c.peers, device=device)
        self.conn = Guarded(c.connected, guard=ONES, device=device) if c.connected is not None else None
        self.po = Guarded(n=c.n_peers + 1, device=device)
        self.mo = Guarded(n=self.n_pairs, device=device)

    def launch(self, r):
        """Enqueues the call; nothing is waited for."""
        c = self.c
        # n_msgs == 0: the offsets pointer may be anything; pass the array all the same
        r.peer_major_device(self.off.ptr, self.peers.ptr if self.n_pairs else None, c.n_msgs, self.n_pairs,
                            self.conn.ptr if self.conn is not None else None, c.n_peers, self.po.ptr,
                            self.mo.ptr if self.n_pairs else None)

    def outputs(self):
        """(peer_offsets, msgs_out) after the canary checks on every array."""
        import torch
        torch.cuda.synchronize()
        c = self.c
        po, mo = self.po.read(), self.mo.read()
        assert (po[c.n_peers + 1:] == CANARY).all(), "written behind d_peer_offsets[n_peers]"
        assert (mo[self.n_pairs:] == CANARY).all(), "written behind d_msgs_out[n_pairs]"
        assert self.off.unchanged() and self.peers.unchanged(), "an input was written"
        assert self.conn is None or self.conn.unchanged(), "the bitmap was written"
        return po[:c.n_peers + 1], mo[:self.n_pairs]

    def run(self, r):
        import torch
        torch.cuda.synchronize()
        self.launch(r)
        return self.outputs()


def check_exact(c, name, po, mo):
    w_po, w_rows = want(name)
    assert po.tobytes() == w_po.tobytes(), (name, "peer offsets", int(po[-1]), int(w_po[-1]))
    assert mo[:len(w_rows)].tobytes() == w_rows.tobytes(), (name, "messages")
    well_formed(c, po, mo)   # the words behind the kept ones hold row indices only


def run_exact(r, name, device="cuda:0"):
    c = cases()[name]
    po, mo = Call(c, device).run(r)
    check_exact(c, name, po, mo)


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    yield r
    r.close()


# ---- the shared cases ---------------------------------------------------------------------

SEPARATE = ("padded_", "all_valid_", "cut_", "size_no_msgs")   # rows with a test of their own below


@pytest.mark.parametrize("name", [n for n in exact_names() if not n.startswith(SEPARATE)])
def test_exact_on_the_shared_cases(router, name):
    """The n_peers sweep, the bitmap word edges, the rows and the sizes, on one handle."""
    run_exact(router, name)


def test_no_messages_after_a_call_that_left_keys():
    """n_msgs == 0 with n_pairs == 1000 on a handle whose scratch holds 20k valid, connected keys."""
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    run_exact(r, "all_valid_larger")
    run_exact(r, "size_no_msgs_1000_pairs")
    r.close()


@pytest.mark.parametrize("order", ["larger_first", "padded_first"])
def test_padded_buffer_after_stale_scratch(order):
    """n_pairs = offsets[M] + 1000 on a handle whose scratch holds the keys of another call, every one
    a valid, connected peer: the padding contributes nothing. Then the other order and sizes."""
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    names = {"larger_first": ("all_valid_larger", "padded_1000", "all_valid_smaller", "padded_1000"),
             "padded_first": ("padded_1000", "all_valid_smaller", "padded_1000", "all_valid_larger")}[order]
    for name in names:
        run_exact(r, name)
    r.close()


@pytest.mark.parametrize("name", [n for n in exact_names() if n.startswith("cut_")])
def test_cut_csr(router, name):
    """n_pairs below offsets[M]: the rows are clamped to the buffer (Guarded: the words behind
    peers[n_pairs) are canaries, and no output word is written for them)."""
    run_exact(router, name)


def test_cut_tick_straight_into_peer_major():
    """The asynchronous chain: a tick into a buffer of `capacity` words that ends in the middle of a
    hot-cube message, then wq_peer_major_device with n_pairs = capacity on the same stream with no
    synchronise between them; expected: peer_major_np of the oracle's CSR at that capacity."""
    import torch
    import test_gpu_truncation as tr
    w = tr.workload()
    ref = tr.oracle_refs(w).plain
    hot = np.flatnonzero((w.cube == tr.HOT) & (ref.e > 256))
    m = int(hot[len(hot) // 2])
    cap = int(ref.offs[m]) + int(ref.e[m]) // 2
    assert int(ref.offs[m]) < cap < int(ref.offs[m + 1]) and cap < ref.P
    n_peers = w.n_peers - 9
    connected = np.packbits(np.random.default_rng(5).random(((n_peers + 31) // 32) * 32) < 0.7,
                            bitorder="little").view(np.uint32)
    w_po, w_rows = interest.peer_major_np(ref.offs, ref.peers[:cap], n_peers, connected, capacity=cap)
    assert 0 < len(w_rows) < cap
    r = tr.mk_router(w)
    t = tr.Tick(w, cap)                      # peers / msgs: cap + SLACK words
    conn = Guarded(connected, guard=ONES)
    po, mo = Guarded(n=n_peers + 1), Guarded(n=cap)
    torch.cuda.synchronize()
    pos, world, sender, repl, M = t.inputs()
    r.route_device(pos, world, sender, repl, M, t.offs.data_ptr(), t.peers.data_ptr(), t.msgs.data_ptr(), cap,
                   t.cnt.data_ptr())
    r.peer_major_device(t.offs.data_ptr(), t.peers.data_ptr(), M, cap, conn.ptr, n_peers, po.ptr, mo.ptr)
    offs, peers, msgs, c = t.read()          # synchronises
    tr.check_outputs(offs, peers, msgs, ref, cap, "cut tick before peer_major")
    assert (int(c["n_pairs"]), int(c["overflow"]), int(c["error"])) == (ref.P, 1, 0)
    g_po, g_mo = po.read(), mo.read()
    assert (g_po[n_peers + 1:] == CANARY).all() and (g_mo[cap:] == CANARY).all() and conn.unchanged()
    assert g_po[:n_peers + 1].tobytes() == w_po.tobytes()
    assert g_mo[:len(w_rows)].tobytes() == w_rows.tobytes()
    assert (g_mo[len(w_rows):cap] < M).all()
    assert r.route_health() == (0, 1)        # read here: the sticky overflow does not reach a later test
    assert r.route_health() == (0, 0)
    r.close()


@pytest.mark.parametrize("name", hostile_names())
def test_hostile_offsets_stay_well_formed(router, name):
    """Offsets that wrap, descend or are all 2^32 - 1: the result is unspecified but well formed,
    nothing outside the arrays is touched, and a second call gives the same bytes."""
    c = cases()[name]
    call = Call(c)
    po, mo = call.run(router)
    well_formed(c, po, mo)
    first = (po.tobytes(), mo.tobytes())
    po, mo = Call(c).run(router)
    assert (po.tobytes(), mo.tobytes()) == first


# ---- a multi-GPU handle -------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["cube", "replicate"])
@pytest.mark.parametrize("devices", [(0, 0), (0, 1)], ids=["one_device_twice", "two_devices"])
def test_multi_gpu_handle(mode, devices):
    """A handle over two sub-handles runs the call on its own stream with the arrays on devices[0]."""
    import torch
    from worldql_server_amd.router import Router
    if torch.cuda.device_count() <= max(devices):
        pytest.skip("needs two devices")
    r = Router.multi(16, devices, mode=mode)
    run_exact(r, "sweep_65536_bitmap")
    run_exact(r, "cut_mid_row")
    r.close()
