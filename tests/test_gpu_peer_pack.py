"""GPU parity for the send buffers (include/wq_router.h wq_peer_pack_device, csrc/wq_pack.hip): every
peer's frames gathered into one contiguous byte run, in list order, optionally behind u32 sizes.

Bars, all bit-exact against worldql_server_amd/interest.py peer_pack_np (the shared case list of
tests/test_peer_pack_host.py, where the definition itself is checked against a restatement):
  - d_out[0 .. bytes_written), d_out_peer_bytes[0 .. n_peers], d_out_elem_bytes[0 .. walked) and the
    counters are the definition's bytes, with and without the prefix, for every capacity cut and for
    hostile rows, message indices and frame offsets;
  - every device array is guarded: d_out is sized exactly to capacity_bytes with canary bytes before and
    behind it, the bytes behind bytes_written are untouched, the other outputs have canaries before
    them and behind their last entry, and every input is as it was; the frame bytes sit at an odd address;
  - every case runs twice on one handle, and the largest after the smallest;
  - the nullable outputs and the sizing call leave the rest identical;
  - pack, count budget, byte budget, pack on one handle with nothing waited for in between;
  - the whole path on the device: routed tick -> per-peer lists -> byte budget -> pack, with real frames."""
import ctypes
import struct

import numpy as np
import pytest

from worldql_server_amd import abi, codec, interest, synth_ext

import test_gpu_peer_budget as count_gpu
import test_gpu_peer_budget_bytes as bytes_gpu
import test_peer_budget_bytes_host as bytes_host
import test_peer_budget_host as count_host
from test_gpu_peer_budget import CANARY, FRONT, SLACK, Guarded
from test_peer_pack_host import cap_of, cases, exact_names, hostile_names, names, uncut, want, well_formed

pytestmark = pytest.mark.gpu

DT = abi.PACK_COUNTERS_DTYPE
CANARY64 = (CANARY << 32) | CANARY
CANARY8 = CANARY & 0xFF
assert CANARY == CANARY8 * 0x01010101


class Bytes:
    """A device byte array of exactly n bytes (the bytes of `data`, or canaries) `shift` bytes behind a
    16-byte aligned address, with 4 * FRONT canary bytes before it and 4 * SLACK behind it."""

    def __init__(self, data=None, n=None, shift=0, device="cuda:0"):
        import torch
        body = np.ascontiguousarray(data, np.uint8) if data is not None else np.full(n, CANARY8, np.uint8)
        self.n = len(body)
        self.front = 4 * FRONT + shift
        self.host = np.concatenate([np.full(self.front, CANARY8, np.uint8), body, np.full(4 * SLACK, CANARY8, np.uint8)])
        self.t = torch.from_numpy(self.host.copy()).to(device)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.front

    def read(self):
        """The array and the canary bytes behind it."""
        return self.t.cpu().numpy()[self.front:]

    def front_intact(self):
        return bool((self.t[:self.front].cpu().numpy() == CANARY8).all())

    def unchanged(self):
        return self.t.cpu().numpy().tobytes() == self.host.tobytes()


class Call:
    """One case on the device: guarded inputs and outputs, and the checks after a call."""

    def __init__(self, name, prefix, device="cuda:0", with_elem=True, with_counters=True, capacity=None, shift=3):
        c = self.c = cases()[name]
        self.name, self.prefix, self.n_in = name, prefix, len(c.msgs)
        self.cap = cap_of(name, prefix) if capacity is None else capacity
        g = lambda a: Guarded(a, device=device)
        self.off, self.msgs, self.fo = g(c.offsets), g(c.msgs), g(c.frame_offsets)
        self.frames = Bytes(c.frames, shift=shift, device=device)        # any alignment
        self.out = Bytes(n=self.cap, device=device) if self.cap else None
        self.pb = Guarded(n=2 * (c.n_peers + 1), device=device)
        self.eb = Guarded(n=2 * self.n_in, device=device) if with_elem else None
        self.cnt = Guarded(n=10, device=device) if with_counters else None

    def launch(self, r):
        """Enqueues the call; nothing is waited for."""
        c = self.c
        r.peer_pack_device(self.off.ptr, self.msgs.ptr if self.n_in else None, c.n_peers, self.n_in,
                           self.frames.ptr if len(c.frames) else None, self.fo.ptr, len(c.frame_offsets) - 1,
                           len(c.frames), abi.PACK_LEN_PREFIX if self.prefix else 0,
                           self.out.ptr if self.out else None, self.cap, self.pb.ptr,
                           self.eb.ptr if self.eb and self.n_in else None, self.cnt.ptr if self.cnt else None)

    def outputs(self):
        """(out[:bytes_written], PB, E or None, counters or None) after the canary checks."""
        import torch
        torch.cuda.synchronize()
        c = self.c
        pb = self.pb.read(np.uint64)
        assert (pb[c.n_peers + 1:] == CANARY64).all(), "written behind d_out_peer_bytes[n_peers]"
        written = min(int(pb[c.n_peers]), self.cap)
        out = np.zeros(0, np.uint8)
        if self.out:
            raw = self.out.read()
            assert (raw[written:] == CANARY8).all(), "written behind d_out[bytes_written)"
            assert self.out.front_intact(), "written before d_out"
            out = raw[:written].copy()
        counters = eb = None
        walked = len(uncut(self.name, self.prefix)[2])
        if self.cnt:
            cnt = self.cnt.read(np.uint8)[:40].view(DT)[0]
            counters = {k: int(cnt[k]) for k in DT.names}
            assert counters["bytes_written"] == written and counters["n_in"] == walked
            assert (self.cnt.read()[10:] == CANARY).all(), "written behind the counters"
        if self.eb:
            eb = self.eb.read(np.uint64)
            assert (eb[walked:] == CANARY64).all(), "written behind d_out_elem_bytes[walked)"
            eb = eb[:walked]
        for a, what in ((self.pb, "d_out_peer_bytes"), (self.eb, "d_out_elem_bytes"), (self.cnt, "the counters")):
            assert a is None or a.front_intact(), "written before " + what
        for a in (self.off, self.msgs, self.fo, self.frames):
            assert a.unchanged(), "an input was written"
        return out, pb[:c.n_peers + 1], eb, counters

    def run(self, r):
        import torch
        torch.cuda.synchronize()
        self.launch(r)
        return self.outputs()


def check(name, prefix, out, pb, eb, counters):
    w_out, w_pb, w_eb, w_cnt = want(name, prefix)
    assert counters is None or counters == w_cnt, (name, counters, w_cnt)
    assert pb.tobytes() == w_pb.tobytes(), (name, "peer bytes")
    assert eb is None or eb.tobytes() == w_eb.tobytes(), (name, "element bytes")
    assert len(out) == len(w_out)
    if out.tobytes() != w_out.tobytes():
        first = int(np.flatnonzero(out != w_out)[0])
        pytest.fail(f"{name}: d_out differs from byte {first} of {len(out)}")
    well_formed(cases()[name], prefix, out, pb, w_eb, counters)


def run_case(r, name, prefix, device="cuda:0", **kw):
    check(name, prefix, *Call(name, prefix, device=device, **kw).run(r))


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    yield r
    r.close()


LARGEST = max(names(), key=lambda n: uncut(n, True)[3]["bytes_need"])
SMALLEST = "nothing"


# ---- the shared cases ---------------------------------------------------------------------

@pytest.mark.parametrize("prefix", [False, True], ids=["plain", "prefix"])
@pytest.mark.parametrize("name", exact_names())
def test_exact_on_the_shared_cases(router, name, prefix):
    """Twice on one handle (the second call sees the first one's scratch)."""
    run_case(router, name, prefix)
    run_case(router, name, prefix, shift=0)


@pytest.mark.parametrize("prefix", [False, True], ids=["plain", "prefix"])
@pytest.mark.parametrize("name", hostile_names())
def test_hostile_rows(router, name, prefix):
    """Descending, overlapping and far offsets: in bounds, error bit 0, the definition's walk, twice."""
    first = Call(name, prefix).run(router)
    assert first[3]["error"] & abi.PACK_ERROR_ROWS
    check(name, prefix, *first)
    run_case(router, name, prefix)


def test_stale_scratch_largest_after_smallest():
    """A fresh handle: the smallest cases, the largest one, and small ones again."""
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    for name, prefix in ((SMALLEST, False), ("no_elements", True), (LARGEST, True), ("no_peers", False),
                         ("cap_in_frame", True), ("tiny_runs", False), (LARGEST, False), ("msgs_junk", True)):
        run_case(r, name, prefix)
    r.close()


@pytest.mark.parametrize("prefix", [False, True], ids=["plain", "prefix"])
@pytest.mark.parametrize("name", names())
def test_nullable_outputs_and_the_sizing_call(router, name, prefix):
    """Without d_out_elem_bytes, without counters, without both: the same bytes. d_out NULL with capacity
    0: the same PB and bytes_need, nothing else."""
    for with_elem, with_counters in ((False, True), (True, False), (False, False)):
        run_case(router, name, prefix, with_elem=with_elem, with_counters=with_counters)
    out, pb, eb, cnt = Call(name, prefix, capacity=0).run(router)
    w_out, w_pb, w_eb, w_cnt = want(name, prefix)
    assert len(out) == 0 and pb.tobytes() == w_pb.tobytes() and eb.tobytes() == w_eb.tobytes()
    assert cnt["bytes_need"] == w_cnt["bytes_need"] and cnt["bytes_written"] == 0
    assert cnt["overflow"] == int(w_cnt["bytes_need"] > 0) and cnt["error"] == w_cnt["error"]


@pytest.mark.parametrize("prefix", [False, True], ids=["plain", "prefix"])
def test_capacity_sweep(router, prefix):
    """A capacity on every byte of two chunks around a prefix, a frame's end and the output's end."""
    name = "cap_need"
    c = cases()[name]
    whole, _, eb, cnt = uncut(name, prefix)
    need = cnt["bytes_need"]
    q = list(c.msgs).index(4)
    caps = set(range(int(eb[q]) - 3, int(eb[q]) + 20)) | set(range(need - 18, need + 2)) | {1, 15, 16, 17}
    for cap in sorted(caps):
        out, pb, e2, counters = Call(name, prefix, capacity=cap).run(router)
        w = interest.peer_pack_np(c.offsets, c.msgs, c.frames, c.frame_offsets, len_prefix=prefix, capacity=cap)
        assert out.tobytes() == whole[:cap].tobytes() == w[0].tobytes() and counters == w[3], cap


def test_steady_state_allocates_nothing(router):
    """After one call has grown the scratch, the same call, a smaller one and both budgets between them
    leave the device's free memory as it was (other processes move it too: a lower figure fails, a
    higher one is measured again)."""
    import torch
    call, small = Call(LARGEST, True), Call("cap_need", False)
    k = count_gpu.Call(count_host.cases()["len_edges_k64"])
    b = bytes_gpu.Call(bytes_host.cases()["mid_tile_w20000"])
    for x in (call, k, b):
        x.run(router)
    for _ in range(5):
        free = torch.cuda.mem_get_info()[0]
        check(LARGEST, True, *call.run(router))
        k.run(router)
        small.run(router)
        b.run(router)
        after = torch.cuda.mem_get_info()[0]
        assert after >= free, ("a steady-state call allocated", free - after)
        if after == free:
            return
    pytest.fail("the device's free memory kept rising: no quiet pair in five")


def test_pack_between_the_budgets(router):
    """Pack, count budget, byte budget, pack on one handle and stream, nothing waited for in between."""
    import torch
    a, d = Call("tiny_runs", True), Call("residues", False)
    k = count_gpu.Call(count_host.cases()["len_edges_k64"])
    b = bytes_gpu.Call(bytes_host.cases()["mid_tile_w20000"])
    torch.cuda.synchronize()
    a.launch(router)
    k.launch(router)
    b.launch(router)
    d.launch(router)
    check("tiny_runs", True, *a.outputs())
    count_gpu.check("len_edges_k64", *k.outputs())
    bytes_gpu.check("mid_tile_w20000", *b.outputs())
    check("residues", False, *d.outputs())
    b.launch(router)
    d.launch(router)
    k.launch(router)
    a.launch(router)
    bytes_gpu.check("mid_tile_w20000", *b.outputs())
    check("residues", False, *d.outputs())
    count_gpu.check("len_edges_k64", *k.outputs())
    check("tiny_runs", True, *a.outputs())


# ---- arguments ------------------------------------------------------------------------------

def test_invalid_arguments():
    from worldql_server_amd.router import Router, WQError, load_library
    name = "cap_need"
    c = cases()[name]
    call = Call(name, True)
    r = Router(16, 0)

    def invalid(**kw):
        a = dict(peer_offsets_ptr=call.off.ptr, msgs_ptr=call.msgs.ptr, n_peers=c.n_peers, n_in=call.n_in,
                 frames_ptr=call.frames.ptr, frame_offsets_ptr=call.fo.ptr, n_msgs=len(c.frame_offsets) - 1,
                 n_frame_bytes=len(c.frames), flags=abi.PACK_LEN_PREFIX, out_ptr=call.out.ptr, capacity_bytes=call.cap,
                 out_peer_bytes_ptr=call.pb.ptr, out_elem_bytes_ptr=call.eb.ptr, counters_ptr=call.cnt.ptr)
        a.update(kw)
        with pytest.raises(WQError) as e:
            r.peer_pack_device(**a)
        assert e.value.code == abi.WQ_E_INVALID

    invalid(peer_offsets_ptr=None)
    invalid(msgs_ptr=None)
    invalid(frames_ptr=None)
    invalid(frame_offsets_ptr=None)
    invalid(out_peer_bytes_ptr=None)                    # always required
    invalid(out_ptr=None)                               # with capacity_bytes > 0
    invalid(out_ptr=call.out.ptr + 4)                   # misaligned
    invalid(out_ptr=call.out.ptr + 8)
    invalid(flags=2)
    invalid(flags=abi.PACK_LEN_PREFIX | 0x80000000)
    invalid(n_in=1 << 32)
    invalid(n_peers=0xFFFFFFFF)                         # the header's limit: n_peers < 2^32 - 1
    lib = load_library()
    assert lib.wq_peer_pack_device(None, None, None, 0, 0, None, None, 0, 0, 0, None, 0,
                                   ctypes.c_void_p(call.pb.ptr), None, None) == abi.WQ_E_INVALID
    import torch
    torch.cuda.synchronize()
    for a in (call.out, call.pb, call.eb, call.cnt):
        assert a.unchanged()                            # nothing was launched
    check(name, True, *call.run(r))                     # and the same arrays run
    r.close()


@pytest.mark.parametrize("devices", [(0, 0), (0, 1)], ids=["one_device_twice", "two_devices"])
def test_multi_gpu_handle(devices):
    """A replicate handle over two sub-handles runs the call on its own stream with the arrays on
    devices[0]."""
    import torch
    from worldql_server_amd.router import Router
    if torch.cuda.device_count() <= max(devices):
        pytest.skip("needs two devices")
    r = Router.multi(16, devices, mode="replicate")
    run_case(r, "sizes", True)
    run_case(r, "cap_in_frame", False)
    r.close()


# ---- the whole path on the device -----------------------------------------------------------

def _walk_prefixed(raw):
    """The frames of one peer's run, prefix by prefix."""
    frames, at = [], 0
    while at < len(raw):
        n = struct.unpack_from("<I", raw, at)[0]
        frames.append(raw[at + 4:at + 4 + n])
        at += 4 + n
    assert at == len(raw)
    return frames


def test_routed_tick_to_send_buffers_on_the_device():
    """A routed tick with real frames, uploaded once: wq_peer_major_device -> wq_peer_budget_bytes_device
    -> wq_peer_pack_device, enqueued back to back. Without the prefix every peer's run has the byte
    budget's d_out_bytes[p] bytes, and the frames cut out at E decode to the sender and position of the
    message in that list slot; with the prefix a walk of each run recovers the same frames."""
    import torch
    from worldql_server_amd.router import Router
    _dev, _u32 = count_gpu._dev, count_gpu._u32
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
    src = tracker.ent
    n_pairs = src[2]
    assert 2000 < n < 20000 and n_pairs > n
    rng = np.random.default_rng(5)
    uuids = [int(i).to_bytes(16, "little") for i in range(n)]
    frames, fo = codec.serialize_messages([
        dict(instruction=7, sender_uuid=uuids[i], world_name="w", position=tuple(pos[i]),
             parameter="x" * int(rng.integers(0, 90))) for i in range(n)])
    sizes = interest.frame_sizes(fo)
    d_frames, d_fo, d_sizes = Bytes(frames, shift=1), Guarded(fo), _dev(sizes)
    W = 700
    i32 = dict(dtype=torch.int32, device="cuda:0")
    po, rows = torch.empty(n + 1, **i32), torch.empty(n_pairs, **i32)
    oo, om = torch.empty(n + 1, **i32), torch.empty(n_pairs, **i32)
    ob = torch.empty(n, dtype=torch.int64, device="cuda:0")
    cap = n * W + 4 * int(n_pairs)       # every peer keeps at most W bytes, and a prefix per element
    outs = {pf: (Bytes(n=cap), torch.empty(n + 1, dtype=torch.int64, device="cuda:0"),
                 torch.empty(n_pairs, dtype=torch.int64, device="cuda:0"), Guarded(n=10)) for pf in (False, True)}
    torch.cuda.synchronize()
    r.peer_major_device(src[0].data_ptr(), src[1].data_ptr(), n, n_pairs, None, n, po.data_ptr(), rows.data_ptr())
    r.peer_budget_bytes_device(po.data_ptr(), rows.data_ptr(), n, n_pairs, d[0].data_ptr(), d_sizes.data_ptr(), n, None, 0,
                               W, None, oo.data_ptr(), om.data_ptr(), ob.data_ptr(), None)
    for pf, (out, pb, eb, cnt) in outs.items():
        r.peer_pack_device(oo.data_ptr(), om.data_ptr(), n, n_pairs, d_frames.ptr, d_fo.ptr, n, len(frames),
                           abi.PACK_LEN_PREFIX if pf else 0, out.ptr, cap, pb.data_ptr(), eb.data_ptr(), cnt.ptr)
    torch.cuda.synchronize()
    h_oo, h_ob = _u32(oo).astype(np.int64), ob.cpu().numpy()
    kept = int(h_oo[n])
    h_om = _u32(om)[:kept]
    assert 0 < kept < n_pairs, "the byte budget cuts some rows and keeps some elements"
    raw_frames = frames.tobytes()
    slot_frames = [raw_frames[int(fo[m]):int(fo[m + 1])] for m in h_om.tolist()]
    # without the prefix
    out, pb, eb, cnt = outs[False]
    c = {k: int(cnt.read(np.uint8)[:40].view(DT)[0][k]) for k in DT.names}
    assert c["error"] == 0 and c["overflow"] == 0 and c["n_in"] == kept == c["n_complete"]
    h_pb, h_eb = pb.cpu().numpy(), eb.cpu().numpy()[:kept]
    assert (np.diff(h_pb) == h_ob).all(), "d_out_bytes sizes every peer's send buffer"
    assert c["bytes_need"] == int(h_pb[n]) == int(h_ob.sum()) == c["bytes_written"]
    raw = out.read()[:c["bytes_written"]]
    assert (out.read()[c["bytes_written"]:c["bytes_written"] + 4096] == CANARY8).all() and out.front_intact()
    ends = np.append(h_eb[1:], c["bytes_need"]).astype(np.uint64)
    dec = codec.decode_packed(raw, np.append(h_eb, c["bytes_need"]).astype(np.uint64))
    assert (dec["status"] == 0).all()
    senders = np.array([int.from_bytes(bytes(u), "little") for u in dec["sender_uuid"]])
    assert (senders == h_om).all() and (dec["position"] == pos[h_om]).all()
    assert all(raw[int(a):int(b)].tobytes() == f for a, b, f in zip(h_eb[:200], ends[:200], slot_frames[:200]))
    w_out, w_pb, w_eb, w_cnt = interest.peer_pack_np(h_oo, h_om, frames, fo)
    assert raw.tobytes() == w_out.tobytes() and h_pb.astype(np.uint64).tobytes() == w_pb.tobytes()
    # with the prefix: a pure-Python walk of every peer's run
    out, pb, eb, cnt = outs[True]
    c = {k: int(cnt.read(np.uint8)[:40].view(DT)[0][k]) for k in DT.names}
    assert c["error"] == 0 and c["overflow"] == 0 and c["bytes_need"] == int(h_ob.sum()) + 4 * kept
    h_pb = pb.cpu().numpy()
    raw = out.read()[:c["bytes_written"]].tobytes()
    walked = []
    for p in range(n):
        run = _walk_prefixed(raw[int(h_pb[p]):int(h_pb[p + 1])])
        assert len(run) == h_oo[p + 1] - h_oo[p]
        walked += run
    assert walked == slot_frames
    assert d_frames.unchanged() and d_fo.unchanged()
    # the tracker's convenience on the same lists: grows its buffer once and returns views
    t_out, t_pb, t_eb = tracker.peer_pack(oo, om[:kept], d_frames.ptr, d_fo.ptr, len(frames), len_prefix=True)
    assert t_out.cpu().numpy().tobytes() == raw and (t_pb.cpu().numpy() == h_pb).all() and t_eb.numel() == kept
    small = tracker.pack_buf.numel()
    tracker.pack_buf = torch.empty(4096, dtype=torch.uint8, device="cuda:0")     # too small: one more call
    t_out, t_pb, t_eb = tracker.peer_pack(oo, om[:kept], d_frames.ptr, d_fo.ptr, len(frames), len_prefix=True)
    assert t_out.cpu().numpy().tobytes() == raw and 4096 < tracker.pack_buf.numel() <= small + (1 << 20)
    r.route_health()
    r.close()
