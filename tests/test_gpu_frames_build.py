"""GPU parity for the frame builder (include/wq_router.h wq_frames_build_device, csrc/wq_frames.hip): a
tick's flat messages serialized on the device.

Bars, all bit-exact against worldql_server_amd/frames.py build_frames_np, which is the host serializer
under the call's malformed-input rules (the shared case list of tests/test_frames_build_host.py):
  - d_frames[0 .. bytes_written), d_frame_offsets[0 .. n], d_frame_size[0 .. n) and the counters are
    the definition's, for the whole grid, the alignment sweep, megabyte payloads, every capacity cut
    and malformed worlds, offsets and flags;
  - every device array is guarded: d_frames is sized exactly to capacity_bytes with canary bytes before
    and behind it, the other outputs have canaries before them and behind their last entry, every input
    is as it was, and every input sits at an odd address in one of the two runs of a case;
  - the frames decode (codec.decode_packed) to the fields they were built from;
  - build -> byte budget -> pack on the device equals peer_pack_np on the host serializer's frames;
  - the call alternates with both budgets and the pack on one handle with nothing waited for."""
import ctypes

import numpy as np
import pytest

from worldql_server_amd import abi, codec, frames, interest

import test_gpu_peer_budget as count_gpu
import test_gpu_peer_budget_bytes as bytes_gpu
import test_gpu_peer_pack as pack_gpu
import test_peer_budget_bytes_host as bytes_host
import test_peer_budget_host as count_host
from test_frames_build_host import (WORLDS, Case, cases, decoded_fields_match, malformed_cases, nullable_cases, payload,
                                    positions, want)
from test_gpu_peer_budget import CANARY, Guarded
from test_gpu_peer_pack import CANARY8, CANARY64, Bytes

pytestmark = pytest.mark.gpu

DT = abi.FRAMES_COUNTERS_DTYPE


class Call:
    """One case on the device: guarded inputs and outputs, and the checks after a call."""

    def __init__(self, c, capacity, device="cuda:0", with_size=True, with_counters=True, shift=1):
        self.c, self.n, self.cap = c, c.n, capacity
        b = lambda a: None if a is None else Bytes(np.ascontiguousarray(a).view(np.uint8).reshape(-1), shift=shift,
                                                   device=device)
        arr = lambda v, dt: None if np.isscalar(v) else np.asarray(v, dt)
        self.ins = {k: b(v) for k, v in dict(
            instruction=arr(c.instruction, np.uint8), replication=arr(c.replication, np.uint8),
            sender_uuid=c.sender_uuid, world=c.world, pos=None if c.pos is None else np.asarray(c.pos, np.float64),
            param=c.param, param_offsets=c.param_offsets, flex=c.flex, flex_offsets=c.flex_offsets,
            msg_flags=c.msg_flags).items()}
        p = lambda k: self.ins[k].ptr if self.ins[k] is not None else None
        nb = lambda given, data: 0 if data is None else (len(data) if given is None else given)
        self.src = abi.FramesSrc(
            instruction=p("instruction"), instruction_all=int(c.instruction) if np.isscalar(c.instruction) else 0,
            replication=p("replication"), replication_all=int(c.replication) if np.isscalar(c.replication) else 0,
            sender_uuid=p("sender_uuid"), world=p("world"), pos=p("pos"), param=p("param"),
            param_offsets=p("param_offsets"), n_param_bytes=nb(c.n_param_bytes, c.param), flex=p("flex"),
            flex_offsets=p("flex_offsets"), n_flex_bytes=nb(c.n_flex_bytes, c.flex), msg_flags=p("msg_flags"))
        self.out = Bytes(n=capacity, device=device) if capacity else None
        self.fo = Guarded(n=2 * (self.n + 1), device=device)
        self.fs = Guarded(n=self.n, device=device) if with_size else None
        self.cnt = Guarded(n=10, device=device) if with_counters else None

    def launch(self, r):
        """Enqueues the call; nothing is waited for."""
        r.build_frames_device(self.src, self.n, self.out.ptr if self.out else None, self.cap, self.fo.ptr,
                              self.fs.ptr if self.fs else None, self.cnt.ptr if self.cnt else None)

    def outputs(self):
        """(frames[:bytes_written], offsets, sizes or None, counters or None) after the canary checks."""
        import torch
        torch.cuda.synchronize()
        n = self.n
        fo = self.fo.read(np.uint64)
        assert (fo[n + 1:] == CANARY64).all(), "written behind d_frame_offsets[n]"
        written = min(int(fo[n]), self.cap)
        data = np.zeros(0, np.uint8)
        if self.out:
            raw = self.out.read()
            assert (raw[written:] == CANARY8).all(), "written behind d_frames[bytes_written)"
            assert self.out.front_intact(), "written before d_frames"
            data = raw[:written].copy()
        sizes = counters = None
        if self.fs:
            fs = self.fs.read()
            assert (fs[n:] == CANARY).all(), "written behind d_frame_size[n)"
            sizes = fs[:n].copy()
        if self.cnt:
            cnt = self.cnt.read(np.uint8)[:40].view(DT)[0]
            counters = {k: int(cnt[k]) for k in DT.names}
            assert counters["bytes_written"] == written and counters["n_frames"] == n
            assert (self.cnt.read()[10:] == CANARY).all(), "written behind the counters"
        for a, what in ((self.fo, "d_frame_offsets"), (self.fs, "d_frame_size"), (self.cnt, "the counters")):
            assert a is None or a.front_intact(), "written before " + what
        for a in self.ins.values():
            assert a is None or a.unchanged(), "an input was written"
        return data, fo[:n + 1].copy(), sizes, counters

    def run(self, r):
        import torch
        torch.cuda.synchronize()
        self.launch(r)
        return self.outputs()


def check(got, wanted, what=""):
    data, off, sizes, cnt = got
    w_data, w_off, w_sizes, w_cnt = wanted
    assert cnt is None or cnt == w_cnt, (what, cnt, w_cnt)
    assert off.tobytes() == w_off.tobytes(), (what, "offsets")
    assert sizes is None or sizes.tobytes() == w_sizes.tobytes(), (what, "sizes")
    assert len(data) == len(w_data)
    if data.tobytes() != w_data.tobytes():
        bad = int(np.flatnonzero(data != w_data)[0])
        i = int(np.searchsorted(w_off, bad, side="right")) - 1
        pytest.fail(f"{what}: d_frames differs from byte {bad}: frame {i}, byte {bad - int(w_off[i])} of {int(w_sizes[i])}")


def run_case(r, name, **kw):
    w = want(name)
    got = Call(cases()[name], len(w[0]), **kw).run(r)
    check(got, w, name)
    return got


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    r.set_worlds(WORLDS)
    yield r
    r.close()


# ---- the shared cases ---------------------------------------------------------------------

def test_the_grid_in_one_call(router):
    """All 1,960 flat messages: frames, offsets, sizes and counters are the host's; twice, the inputs at
    odd and at aligned addresses."""
    a = run_case(router, "grid")
    b = run_case(router, "grid", shift=0)
    assert a[0].tobytes() == b[0].tobytes() and a[3]["n_complete"] == 1960


def test_alignment_sweep(router):
    """Parameter and flex packed back to back, their starts on every residue mod 16, lengths 0..40,
    1022..1026 and 4095..4097."""
    for shift in (1, 0, 7):
        run_case(router, "residues", shift=shift)
    for name in ("payload_0_40", "payload_edges", "world_lens", "param_only", "flex_only", "entity_updates"):
        run_case(router, name)


def test_megabyte_payloads_among_grid_messages(router):
    """One message with a 1 MiB flex and one with a 1 MiB parameter among 1,000 grid messages."""
    run_case(router, "with_big")
    run_case(router, "with_big", shift=0)


@pytest.mark.parametrize("name", ["residues", "cap_300"])
def test_capacity(router, name):
    """The sizing call, then capacities around the result: the written prefix is whole[:cap], the bytes
    behind it are untouched, and offsets, sizes and counters are always complete."""
    c = cases()[name]
    whole, off, sizes, cnt = want(name)
    need = len(whole)
    data, o, s, k = Call(c, 0).run(router)
    assert len(data) == 0 and o.tobytes() == off.tobytes() and s.tobytes() == sizes.tobytes()
    assert k == dict(cnt, bytes_written=0, overflow=1, n_complete=0)
    for cap in (1, (need // 2) | 1, need - 1, need, need + 1):
        got = Call(c, cap).run(router)
        check(got, frames.build_frames_np(capacity=cap, **c.kw()), f"{name} at capacity {cap}")
        assert got[0].tobytes() == whole[:cap].tobytes()


@pytest.mark.parametrize("name", list(malformed_cases()))
def test_malformed_inputs(name):
    """A world id outside the table, offsets that descend, reach past the end or span 2^32, flags that
    ask for a field whose array is NULL: the definition's bytes and error bits, the neighbours whole."""
    from worldql_server_amd.router import Router
    c, bits = malformed_cases()[name]
    r = Router(16, 0)
    if c.worlds:
        r.set_worlds(c.worlds)
    w = frames.build_frames_np(**c.kw())
    for shift in (1, 0):
        got = Call(c, len(w[0]), shift=shift).run(r)
        check(got, w, name)
        assert got[3]["error"] == bits
    r.close()


@pytest.mark.parametrize("combo,c", nullable_cases(), ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else "")
def test_every_nullable_combination(router, combo, c):
    w = frames.build_frames_np(**c.kw())
    check(Call(c, len(w[0])).run(router), w, str(combo))


def test_nullable_outputs(router):
    c, w = cases()["payload_0_40"], want("payload_0_40")
    for with_size, with_counters in ((False, True), (True, False), (False, False)):
        check(Call(c, len(w[0]), with_size=with_size, with_counters=with_counters).run(router), w)


def test_no_messages_and_table_changes():
    """n = 0; a handle with no table; set_worlds between two builds on one stream, nothing waited for."""
    import torch
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    got = Call(cases()["empty"], 0).run(r)
    assert got[3] == dict(n_frames=0, n_complete=0, bytes_need=0, bytes_written=0, overflow=0, error=0)
    assert list(got[1]) == [0]
    got = Call(cases()["empty"], 64).run(r)
    assert len(got[0]) == 0 and got[3]["overflow"] == 0
    c = Case(world=[0, 1, 2, 1], pos=positions(4, 40))
    c.worlds = None
    w_none = frames.build_frames_np(**c.kw())
    got = Call(c, len(w_none[0])).run(r)
    check(got, w_none, "no table")
    assert got[3]["error"] == frames.ERROR_WORLD
    tables = (["alpha", "b", ""], ["x", "a longer name that moves every byte", "zz"], [], ["only"])
    calls = []
    torch.cuda.synchronize()
    for t in tables:
        c.worlds = t
        r.set_worlds(t)
        calls.append((Call(c, 1024), frames.build_frames_np(capacity=1024, **c.kw())))
        calls[-1][0].launch(r)
    for call, w in calls:
        check(call.outputs(), w, "table replaced")
    assert [w[3]["error"] for _, w in calls] == [0, 0, 1, 1]
    r.close()


def test_device_frames_decode_to_their_fields(router):
    for name in ("grid", "with_big", "world_lens"):
        c = cases()[name]
        data, off, _, _ = Call(c, len(want(name)[0])).run(router)
        decoded_fields_match(c, data, off)


def test_two_calls_are_identical_and_scratch_is_reused(router):
    """The same call twice, the largest case after the smallest, and no allocation at steady state."""
    import torch
    big, small = Call(cases()["with_big"], len(want("with_big")[0])), Call(cases()["cap_300"], 512)
    first = big.run(router)
    check(first, want("with_big"))
    for _ in range(5):
        free = torch.cuda.mem_get_info()[0]
        small.run(router)
        again = big.run(router)
        assert again[0].tobytes() == first[0].tobytes() and again[3] == first[3]
        after = torch.cuda.mem_get_info()[0]
        assert after >= free, ("a steady-state call allocated", free - after)
        if after == free:
            return
    pytest.fail("the device's free memory kept rising: no quiet pair in five")


def test_build_between_the_budgets_and_the_pack(router):
    """Build, count budget, byte budget, pack, build on one handle and stream, nothing waited for."""
    import torch
    a = Call(cases()["residues"], len(want("residues")[0]))
    d = Call(cases()["grid"], len(want("grid")[0]), shift=0)
    k = count_gpu.Call(count_host.cases()["len_edges_k64"])
    b = bytes_gpu.Call(bytes_host.cases()["mid_tile_w20000"])
    p = pack_gpu.Call("tiny_runs", True)
    torch.cuda.synchronize()
    for x in (a, k, b, p, d):
        x.launch(router)
    check(a.outputs(), want("residues"), "residues")
    count_gpu.check("len_edges_k64", *k.outputs())
    bytes_gpu.check("mid_tile_w20000", *b.outputs())
    pack_gpu.check("tiny_runs", True, *p.outputs())
    check(d.outputs(), want("grid"), "grid")
    for x in (p, d, b, a, k):
        x.launch(router)
    pack_gpu.check("tiny_runs", True, *p.outputs())
    check(d.outputs(), want("grid"), "grid")
    bytes_gpu.check("mid_tile_w20000", *b.outputs())
    check(a.outputs(), want("residues"), "residues")
    count_gpu.check("len_edges_k64", *k.outputs())


# ---- arguments ------------------------------------------------------------------------------

def test_invalid_arguments():
    import torch
    from worldql_server_amd.router import Router, WQError, load_library
    c, w = cases()["cap_300"], want("cap_300")
    call = Call(c, len(w[0]))
    r = Router(16, 0)
    r.set_worlds(WORLDS)

    def invalid(src=None, **kw):
        a = dict(src=call.src, n_msgs=c.n, frames_ptr=call.out.ptr, capacity_bytes=call.cap,
                 frame_offsets_ptr=call.fo.ptr, frame_size_ptr=call.fs.ptr, counters_ptr=call.cnt.ptr)
        a.update(kw)
        if src:
            s = abi.FramesSrc.from_buffer_copy(call.src)
            for key, v in src.items():
                setattr(s, key, v)
            a["src"] = s
        with pytest.raises(WQError) as e:
            r.build_frames_device(**a)
        assert e.value.code == abi.WQ_E_INVALID

    invalid(src=dict(sender_uuid=None))
    invalid(src=dict(world=None))
    invalid(src=dict(param=None))                       # param_offsets without param
    invalid(src=dict(param_offsets=None))               # and the reverse
    invalid(src=dict(flex=None))
    invalid(src=dict(flex_offsets=None))
    invalid(frame_offsets_ptr=None)                     # always required
    invalid(frames_ptr=None)                            # with capacity_bytes > 0
    invalid(frames_ptr=call.out.ptr + 4)                # misaligned
    invalid(frames_ptr=call.out.ptr + 8)
    invalid(n_msgs=0xFFFFFFFF)                          # the header's limit: n_msgs < 2^32 - 1
    lib = load_library()
    vp = ctypes.c_void_p
    assert lib.wq_frames_build_device(None, ctypes.byref(call.src), c.n, vp(call.out.ptr), call.cap, vp(call.fo.ptr),
                                      None, None) == abi.WQ_E_INVALID
    assert lib.wq_frames_build_device(r.h, None, c.n, vp(call.out.ptr), call.cap, vp(call.fo.ptr), None,
                                      None) == abi.WQ_E_INVALID
    # a table whose offsets descend or whose name is not UTF-8 is refused and the old table kept
    off = np.array([0, 3, 2], np.uint32)
    assert lib.wq_frames_set_worlds(r.h, b"abc", off.ctypes.data, 2) == abi.WQ_E_INVALID
    off = np.array([0, 2], np.uint32)
    assert lib.wq_frames_set_worlds(r.h, b"\xc3\x28", off.ctypes.data, 1) == abi.WQ_E_INVALID
    assert lib.wq_frames_set_worlds(r.h, b"ab", None, 1) == abi.WQ_E_INVALID
    assert lib.wq_frames_set_worlds(None, b"ab", off.ctypes.data, 1) == abi.WQ_E_INVALID
    torch.cuda.synchronize()
    for a in (call.out, call.fo, call.fs, call.cnt):
        assert a.unchanged()                            # nothing was launched
    check(call.run(r), w, "after the refused calls")    # the same arrays run, on the old table
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
    r.set_worlds(WORLDS)
    run_case(r, "residues")
    run_case(r, "cap_300")
    r.close()


# ---- the whole path on the device -----------------------------------------------------------

def test_build_budget_pack_on_the_device(router):
    """64 peers, 200 messages: the frames built on the device, d_frame_size into
    wq_peer_budget_bytes_device, its lists into wq_peer_pack_device with the device frames, enqueued
    back to back. The result is peer_pack_np over the host serializer's frames and the host budget."""
    import torch
    n, n_peers = 200, 64
    rng = np.random.default_rng(50)
    c = Case(world=rng.integers(0, len(WORLDS), n), instruction=rng.choice([0, 6, 7], n).astype(np.uint8),
             replication=rng.integers(0, 3, n).astype(np.uint8), pos=rng.uniform(-100, 100, (n, 3)),
             param=payload(rng.integers(0, 60, n), 51, True), flex=payload(rng.integers(0, 300, n), 52, False),
             msg_flags=rng.integers(0, 8, n).astype(np.uint8) | 1, seed=53)
    lens = rng.integers(0, 40, n_peers)
    po = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    rows = rng.integers(0, n, int(po[-1])).astype(np.uint32)
    peer_pos = rng.uniform(-100, 100, (n_peers, 3))
    W = 1500
    # the host path: serializer, byte budget, pack
    h_msgs = []
    for i in range(n):
        m = dict(instruction=int(c.instruction[i]), replication=int(c.replication[i]), sender_uuid=c.sender_uuid[i].tobytes(),
                 world_name=WORLDS[c.world[i]], position=c.pos[i])
        if c.msg_flags[i] & 2:
            m["parameter"] = c.param[int(c.param_offsets[i]):int(c.param_offsets[i + 1])].tobytes()
        if c.msg_flags[i] & 4:
            m["flex"] = c.flex[int(c.flex_offsets[i]):int(c.flex_offsets[i + 1])].tobytes()
        h_msgs.append(m)
    h_frames, h_fo = codec.serialize_messages(h_msgs)
    h_oo, h_om, h_ob, _ = interest.peer_budget_bytes_np(po, rows, c.pos, interest.frame_sizes(h_fo), peer_pos, w=W)
    w_out, w_pb, w_eb, w_cnt = interest.peer_pack_np(h_oo, h_om, h_frames, h_fo, len_prefix=True)
    assert 0 < len(h_om) < len(rows), "the byte budget cuts some rows and keeps some elements"
    # the device path
    call = Call(c, len(h_frames), shift=0)
    g = lambda a: Guarded(a)
    d_po, d_rows, d_pp = g(po), g(rows), g(peer_pos)
    oo, om = Guarded(n=n_peers + 1), Guarded(n=len(rows))
    cap = len(w_out)
    out, pb, eb, cnt = Bytes(n=cap), Guarded(n=2 * (n_peers + 1)), Guarded(n=2 * len(rows)), Guarded(n=10)
    torch.cuda.synchronize()
    call.launch(router)
    router.peer_budget_bytes_device(d_po.ptr, d_rows.ptr, n_peers, len(rows), call.ins["pos"].ptr, call.fs.ptr, n,
                                    d_pp.ptr, n_peers, W, None, oo.ptr, om.ptr, None, None)
    router.peer_pack_device(oo.ptr, om.ptr, n_peers, len(rows), call.out.ptr, call.fo.ptr, n, len(h_frames),
                            abi.PACK_LEN_PREFIX, out.ptr, cap, pb.ptr, eb.ptr, cnt.ptr)
    data, fo, fs, k = call.outputs()
    assert data.tobytes() == h_frames.tobytes() and fo.tobytes() == h_fo.tobytes() and k["error"] == 0
    assert oo.read()[:n_peers + 1].tobytes() == h_oo.tobytes() and om.read()[:len(h_om)].tobytes() == h_om.tobytes()
    p = {key: int(cnt.read(np.uint8)[:40].view(abi.PACK_COUNTERS_DTYPE)[0][key]) for key in abi.PACK_COUNTERS_DTYPE.names}
    assert p == w_cnt
    assert out.read()[:cap].tobytes() == w_out.tobytes() and (out.read()[cap:] == CANARY8).all()
    assert pb.read(np.uint64)[:n_peers + 1].tobytes() == w_pb.tobytes()
    assert eb.read(np.uint64)[:len(w_eb)].tobytes() == w_eb.tobytes()


def test_tracker_builds_the_frames(router):
    """InterestTracker.build_frames: views of the grow-only buffer, grown once when it is too small."""
    import torch
    c, w = cases()["with_big"], want("with_big")
    tracker = interest.InterestTracker(router, c.n, 16)
    call = Call(c, 16, shift=0)
    data, fo, fs = tracker.build_frames(call.src)
    assert data.cpu().numpy().tobytes() == w[0].tobytes() and tracker.frame_buf.numel() > 2 << 20
    assert fo.cpu().numpy().astype(np.uint64).tobytes() == w[1].tobytes()
    assert fs.cpu().numpy().view(np.uint32).tobytes() == w[2].tobytes()
    data2, _, _ = tracker.build_frames(call.src)
    assert data2.data_ptr() == data.data_ptr() and torch.equal(data2, data)
