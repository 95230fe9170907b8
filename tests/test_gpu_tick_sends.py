"""GPU parity for the tick sends (include/wq_router.h wq_tick_sends_device, csrc/wq_sends.hip): one
per-peer list of received frames, ascending, from all the CSR regions a tick's read runs left.

Bars, all bit-exact against worldql_server_amd/interest.py tick_sends_np (the shared case list of
tests/test_tick_sends_host.py, where the definition itself is checked against a restatement):
  - d_peer_offsets[0 .. n_peers], the kept prefix of d_frames_out, the zeros behind it and the counters are
    the definition's bytes, for both key widths;
  - every device array is guarded: canary words before and behind every output, and every input is as it
    was;
  - for offsets that descend only the well-formedness clauses of include/wq_router.h, the canaries, and
    equal bytes from a second call;
  - a second call is byte-identical and a steady-state call allocates nothing;
  - every refused call leaves the outputs untouched;
  - the call between a decode, a route and a pack on one handle, and on a multi-GPU handle;
  - end to end on one handle: frames -> decode -> dispatch -> IngestTick.process -> IngestTick.sends ->
    wq_peer_pack_device over the tick's received frames, over 6,000 random events in ticks of 97 and 400
    frames, equals the reference's sequential loop: recipients event by event, and every peer's packed
    bytes."""
import ctypes
import uuid

import numpy as np
import pytest

from worldql_server_amd import abi, ingest, synth

import test_gpu_frames_decode as decode_gpu
import test_gpu_peer_pack as pack_gpu
from test_frames_build_host import WORLDS as BUILD_WORLDS
from test_frames_decode_host import PEER_IDS, PEER_UUIDS, batches, same as decode_same
from test_gpu_peer_budget import CANARY, Guarded
from test_ingest_dispatch_host import N_PEERS, all_worlds, check_events, sanitized, stream, ticks_of, wire
from test_tick_sends_host import cases, exact_names, hostile_names, invalid_cases, want, well_formed
from tests.seq_reference import SequentialReference

pytestmark = pytest.mark.gpu

DT = abi.TICK_SENDS_COUNTERS_DTYPE


class Call:
    """One case on the device: guarded inputs and outputs, and the checks after a call."""

    def __init__(self, c, device="cuda:0", with_counters=True):
        self.c = c
        g = lambda a: Guarded(a if a is not None else np.zeros(0, np.uint32), device=device)
        self.off, self.peers, self.src = g(c.offsets), g(c.peers), (g(c.srcs[0]), g(c.srcs[1]))
        self.conn = g(c.connected) if c.connected is not None else None
        # the two refused calls whose sizes no buffer holds write nothing: small outputs do
        self.po = Guarded(n=c.n_peers + 1 if c.n_peers < 0xFFFFFFFF else 64, device=device)
        self.fo = Guarded(n=c.n_elems if c.n_elems <= 1 << 24 else 64, device=device)
        self.cnt = Guarded(n=16, device=device) if with_counters else None

    def launch(self, r):
        """Enqueues the call; nothing is waited for."""
        c = self.c
        n = lambda a: 0 if a is None else len(a)
        r.tick_sends_device(c.regions, self.off.ptr if len(c.offsets) else None, len(c.offsets),
                            self.peers.ptr if c.n_pairs else None, c.n_pairs,
                            [s.ptr if n(a) else None for s, a in zip(self.src, c.srcs)], [n(a) for a in c.srcs],
                            self.conn.ptr if self.conn is not None else None, c.n_peers, c.n_frames, self.po.ptr,
                            self.fo.ptr if c.n_elems else None, c.n_elems, self.cnt.ptr if self.cnt else None)

    def inputs_unchanged(self):
        return all(a.unchanged() for a in (self.off, self.peers, *self.src)) and (self.conn is None or self.conn.unchanged())

    def outputs(self):
        """(peer_offsets, frames_out, counters or None) after the canary checks on every array."""
        import torch
        torch.cuda.synchronize()
        c = self.c
        po, fo = self.po.read(), self.fo.read()
        assert (po[c.n_peers + 1:] == CANARY).all(), "written behind d_peer_offsets[n_peers]"
        assert (fo[c.n_elems:] == CANARY).all(), "written behind d_frames_out[n_elems]"
        assert self.po.front_intact() and self.fo.front_intact(), "written before an output"
        counters = None
        if self.cnt:
            raw = self.cnt.read()
            assert (raw[16:] == CANARY).all() and self.cnt.front_intact(), "written beside the counters"
            rec = raw[:16].copy().view(DT)[0]
            assert int(rec["pad_"]) == 0 and int(rec["reserved_"]) == 0
            counters = {k: int(rec[k]) for k in DT.names if not k.endswith("_")}
        assert self.inputs_unchanged(), "an input was written"
        return po[:c.n_peers + 1].copy(), fo[:c.n_elems].copy(), counters

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(a.unchanged() for a in (self.po, self.fo, self.cnt) if a is not None) and self.inputs_unchanged()

    def run(self, r):
        import torch
        torch.cuda.synchronize()
        self.launch(r)
        return self.outputs()


def check_exact(name, po, fo, counters):
    w_po, w_frames, w_cnt = want(name)
    assert po.tobytes() == w_po.tobytes(), (name, "peer offsets", int(po[-1]), int(w_po[-1]))
    assert fo[:len(w_frames)].tobytes() == w_frames.tobytes(), (name, "frames")
    assert counters is None or counters == w_cnt, (name, counters, w_cnt)
    well_formed(cases()[name], po, fo, counters)   # the words behind the kept ones are zeros


def run_exact(r, name, device="cuda:0", **kw):
    check_exact(name, *Call(cases()[name], device=device, **kw).run(r))


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    yield r
    r.close()


# ---- the shared cases ---------------------------------------------------------------------

@pytest.mark.parametrize("name", exact_names())
def test_exact_on_the_shared_cases(router, name):
    """Every named case, both key widths among them ('mixed_32bit', 'exactly_32_bits': u32 keys;
    'mixed_64bit', 'exactly_33_bits', 'frames_2_pow_32': u64 keys), on one handle."""
    run_exact(router, name)


def test_without_counters(router):
    for name in ("mixed_32bit", "mixed_64bit", "no_regions"):
        run_exact(router, name, with_counters=False)


@pytest.mark.parametrize("name", hostile_names())
def test_hostile_offsets_stay_well_formed(router, name):
    """Offsets that descend or are junk: the result is unspecified but well formed, error bit 0 is set,
    nothing outside the arrays is touched, and a second call gives the same bytes."""
    c = cases()[name]
    po, fo, cnt = Call(c).run(router)
    well_formed(c, po, fo, cnt)
    assert cnt["error"] & abi.SENDS_ERROR_ROWS
    again = Call(c).run(router)
    assert (po.tobytes(), fo.tobytes(), cnt) == (again[0].tobytes(), again[1].tobytes(), again[2])


def test_two_calls_are_identical_and_scratch_is_reused(router):
    """The same call twice, the largest case after the smallest, and no allocation at steady state."""
    import torch
    big, small = Call(cases()["mixed_64bit"]), Call(cases()["interleaved"])
    narrow = Call(cases()["mixed_32bit"])
    first = big.run(router)
    check_exact("mixed_64bit", *first)
    narrow.run(router)
    for _ in range(5):
        free = torch.cuda.mem_get_info()[0]
        small.run(router)
        check_exact("mixed_32bit", *narrow.run(router))
        again = big.run(router)
        assert (again[0].tobytes(), again[1].tobytes(), again[2]) == (first[0].tobytes(), first[1].tobytes(), first[2])
        after = torch.cuda.mem_get_info()[0]
        assert after >= free, ("a steady-state call allocated", free - after)
        if after == free:
            return
    pytest.fail("the device's free memory kept rising: no quiet pair in five")


def test_regions_are_free_to_reuse_when_the_call_returns(router):
    """Eight calls back to back, nothing waited for, each from the same host array overwritten in between."""
    names = ["interleaved", "two_runs_odd", "cut_mid_row", "unit_frame_base"] * 2
    calls = [Call(cases()[n]) for n in names]
    k = max(len(c.c.regions) for c in calls)
    shared = np.zeros(k, abi.SEND_REGION_DTYPE)
    for call in calls:
        n = len(call.c.regions)
        shared[:n] = call.c.regions
        shared[n:] = abi.send_region(off_at=0, n_rows=5, capacity=9)          # never part of a call
        call.c = type(call.c)(**{**vars(call.c), "regions": shared[:n]})
        call.launch(router)
        shared[:] = abi.send_region(off_at=77, peers_at=99, n_rows=3, capacity=1 << 20)
    for name, call in zip(names, calls):
        call.c = cases()[name]
        check_exact(name, *call.outputs())


@pytest.mark.parametrize("name", sorted(invalid_cases()))
def test_invalid_calls_leave_the_outputs_untouched(router, name):
    from worldql_server_amd.router import WQError
    call = Call(invalid_cases()[name])
    with pytest.raises(WQError) as e:
        call.launch(router)
    assert e.value.code == abi.WQ_E_INVALID and "tick_sends" in str(e.value)
    assert call.untouched()
    run_exact(router, "two_runs_odd")                      # the handle is as usable as before


def test_null_arguments(router):
    from worldql_server_amd.router import load_library
    lib = load_library()
    call = Call(cases()["two_runs_odd"])
    c = call.c
    reg = np.ascontiguousarray(c.regions)
    src = abi.TickSendsIn(regions=reg.ctypes.data, d_offsets=call.off.ptr, n_offsets=len(c.offsets), d_peers=call.peers.ptr,
                          n_pairs=c.n_pairs, d_src=(ctypes.c_void_p * 2)(call.src[0].ptr, call.src[1].ptr),
                          n_src=(ctypes.c_size_t * 2)(len(c.srcs[0]), len(c.srcs[1])), n_regions=len(reg), n_peers=c.n_peers,
                          n_frames=c.n_frames)
    f = lib.wq_tick_sends_device
    assert f(None, ctypes.byref(src), call.po.ptr, call.fo.ptr, c.n_elems, None) == abi.WQ_E_INVALID
    assert f(router.h, None, call.po.ptr, call.fo.ptr, c.n_elems, None) == abi.WQ_E_INVALID
    assert f(router.h, ctypes.byref(src), None, call.fo.ptr, c.n_elems, None) == abi.WQ_E_INVALID
    assert f(router.h, ctypes.byref(src), call.po.ptr, None, c.n_elems, None) == abi.WQ_E_INVALID
    for field in ("regions", "d_offsets", "d_peers"):
        bad = abi.TickSendsIn()
        ctypes.memmove(ctypes.byref(bad), ctypes.byref(src), ctypes.sizeof(src))
        setattr(bad, field, None)
        assert f(router.h, ctypes.byref(bad), call.po.ptr, call.fo.ptr, c.n_elems, None) == abi.WQ_E_INVALID, field
    assert call.untouched()
    assert f(router.h, ctypes.byref(src), call.po.ptr, call.fo.ptr, c.n_elems, call.cnt.ptr) == 0
    check_exact("two_runs_odd", *call.outputs())


def test_sends_between_decode_route_and_pack():
    """Sends, decode, route, pack, sends on one handle and stream, nothing waited for, both orders."""
    import torch
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    r.set_worlds(BUILD_WORLDS)
    r.set_ingest_peers(PEER_UUIDS, PEER_IDS)
    w = synth.config_c2(repl_mode="mixed", scale=0.05)
    r.apply_ops(w.ops)
    w_offs, w_peers, _ = r.route(w.pos, w.world, w.sender, w.repl)
    dev = torch.device("cuda:0")
    t_in = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
            (np.asarray(w.pos, np.float64), w.world.view(np.int32), w.sender.view(np.int32), np.asarray(w.repl, np.uint8))]
    M, P = len(w_offs) - 1, len(w_peers)
    t_off = torch.zeros(M + 1, dtype=torch.int32, device=dev)
    t_peers = torch.zeros(max(P, 1), dtype=torch.int32, device=dev)

    class Route:
        def launch(self, r):
            r.route_device(*[t.data_ptr() for t in t_in], M, t_off.data_ptr(), t_peers.data_ptr(), None, P)

    d1, o1, _ = batches()["corpus_3"]
    w1 = ingest.decode_frames_np(d1, o1, BUILD_WORLDS, PEER_UUIDS, PEER_IDS)
    a, b = Call(cases()["mixed_32bit"]), Call(cases()["mixed_64bit"])
    dec, p, rt = decode_gpu.Call(d1, o1), pack_gpu.Call("tiny_runs", True), Route()
    torch.cuda.synchronize()
    for order in ((a, dec, rt, p, b), (p, b, rt, a, dec)):
        t_off.zero_()
        t_peers.zero_()
        torch.cuda.synchronize()
        for x in order:
            x.launch(r)
        check_exact("mixed_32bit", *a.outputs())
        decode_same(dec.outputs(), w1, "corpus_3")
        pack_gpu.check("tiny_runs", True, *p.outputs())
        check_exact("mixed_64bit", *b.outputs())
        assert t_off.cpu().numpy().view(np.uint32).tobytes() == w_offs.tobytes()
        assert t_peers.cpu().numpy().view(np.uint32)[:P].tobytes() == w_peers.tobytes()
    assert r.route_health() == (0, 0)
    r.close()


@pytest.mark.parametrize("mode", ["cube", "replicate"])
@pytest.mark.parametrize("devices", [(0, 0), (0, 1)], ids=["one_device_twice", "two_devices"])
def test_multi_gpu_handle(mode, devices):
    """A handle over two sub-handles runs the call on its own stream with the arrays on devices[0]."""
    import torch
    from worldql_server_amd.router import Router
    if torch.cuda.device_count() <= max(devices):
        pytest.skip("needs two devices")
    r = Router.multi(16, devices, mode=mode)
    for name in ("mixed_32bit", "mixed_64bit", "cut_mid_row"):
        run_exact(r, name)
    r.close()


# ---- from the wire to the send buffers -------------------------------------------------------------

class Recorder:
    """The sequential reference, keeping what it answered event by event."""

    def __init__(self, ref):
        self.ref, self.log = ref, []

    def event(self, ev):
        self.log.append(self.ref.event(ev))
        return self.log[-1]


def test_frames_to_send_buffers_equal_the_sequential_reference():
    """The 6,000-event stream of test_frames_to_routed_runs_equal_the_sequential_reference in ticks of 97 and
    400 frames on one handle: decode, dispatch, process, IngestTick.sends, wq_peer_pack_device over the tick's
    received frames. Every peer's list ascends; inverted (frame -> peers) the lists are the reference's
    recipients event by event; every peer's packed run is the received frames the reference sends it, in
    arrival order, byte for byte."""
    import torch
    from worldql_server_amd.router import Router
    events = stream(6000, seed=33)
    worlds = all_worlds()
    peers = [uuid.UUID(int=k + 1) for k in range(N_PEERS)]
    r = Router(16, 0)
    r.set_worlds(worlds)
    r.set_ingest_peers(peers)
    dev = torch.device("cuda:0")
    offs = torch.zeros(400 + 4 * 400 + 8, dtype=torch.int32, device=dev)
    out_peers = torch.zeros(400 * 512, dtype=torch.int32, device=dev)
    last_seen = torch.zeros(N_PEERS, dtype=torch.int32, device=dev)
    PACK_CAP = 64 << 20
    packed = torch.zeros(PACK_CAP, dtype=torch.uint8, device=dev)
    pb = torch.zeros(N_PEERS + 1, dtype=torch.int64, device=dev)
    pcnt = torch.zeros(abi.PACK_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    tick = ingest.IngestTick(r, capacity=16)
    ref = Recorder(SequentialReference(16))
    nonempty = both_kinds = multi_region_peers = 0
    for t, chunk in enumerate(ticks_of(events, (97, 400))):
        data, offsets = wire(chunk)
        d_frames = torch.from_numpy(data.copy()).to(dev)
        d_off = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        tick.decode(d_frames, d_off).dispatch(last_seen=last_seen, now=t + 1)
        cnt, runs, reads = tick.process(offs, out_peers)
        po_t, fo_t = tick.sends(reads, offs, out_peers, N_PEERS)
        n_elems = fo_t.numel()
        r.peer_pack_device(po_t.data_ptr(), fo_t.data_ptr() if n_elems else None, N_PEERS, n_elems, d_frames.data_ptr(),
                           d_off.data_ptr(), len(chunk), len(data), 0, packed.data_ptr(), PACK_CAP, pb.data_ptr(), None,
                           pcnt.data_ptr())
        got_s = tick.read_sends()
        got_d = tick.read_dispatch()
        po, frames, sc = got_s["peer_offsets"].astype(np.int64), got_s["frames"], got_s["counters"]
        assert cnt["error"] == 0 and cnt["n_frames"] == len(chunk) and cnt["n_bad"] == 0
        assert sc["error"] == 0 and sc["n_drop_peer"] == 0 and sc["n_drop_frame"] == 0 and sc["n_regions"] > 0
        both_kinds += sum(1 for read in reads if read["local"] is not None and read["global"] is not None)
        # the region every routed frame lies in
        region_of = np.full(len(chunk), -1, np.int64)
        k = 0
        for read in reads:
            for key, src in (("local", got_d["l_src"]), ("global", got_d["g_src"])):
                if read[key] is not None:
                    lo, hi = read[key]["rows"]
                    region_of[src[lo:hi]] = k
                    k += 1
        assert k == sc["n_regions"]
        # every list ascends; inverted, the lists give each frame's recipients
        res = [[] for _ in chunk]
        for p in np.flatnonzero(np.diff(po)):
            mine = frames[po[p]:po[p + 1]]
            assert (np.diff(mine.astype(np.int64)) > 0).all(), (t, p, mine)
            assert (region_of[mine] >= 0).all()
            multi_region_peers += len(set(region_of[mine].tolist())) >= 2
            for f in mine.tolist():
                res[f].append(int(p))
        first = len(ref.log)
        dec = dict(repl=tick.buf["repl"][:len(chunk)].cpu().numpy())
        nonempty += check_events(chunk, dec, got_d, res, ref, lambda ids: [f"peer-{q}" for q in ids])
        # the packed runs: per peer the frames the reference sends it, in arrival order
        c = pcnt.cpu().numpy().view(abi.PACK_COUNTERS_DTYPE)[0]
        assert int(c["error"]) == 0 and int(c["overflow"]) == 0 and int(c["bytes_written"]) == int(c["bytes_need"])
        wire_of = [data[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(len(chunk))]
        want_run = [[] for _ in range(N_PEERS)]
        for i, answer in enumerate(ref.log[first:]):
            if isinstance(answer, list):
                for name in answer:
                    want_run[int(name.split("-")[1])].append(wire_of[i])
        g_pb = pb.cpu().numpy().view(np.uint64)
        g_out = packed[:int(g_pb[N_PEERS])].cpu().numpy().tobytes()
        assert int(g_pb[N_PEERS]) == int(c["bytes_written"]) == sum(len(b) for run in want_run for b in run)
        for p in range(N_PEERS):
            assert g_out[int(g_pb[p]):int(g_pb[p + 1])] == b"".join(want_run[p]), (t, p)
    assert r.route_health() == (0, 0)
    assert nonempty > 500 and both_kinds > 100 and multi_region_peers > 100
    r.close()
