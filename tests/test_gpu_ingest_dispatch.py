"""GPU parity for the ingest dispatch (include/wq_router.h wq_ingest_dispatch_device, csrc/wq_dispatch.hip):
a decoded tick split by instruction on the device.

Bars, all bit-exact against worldql_server_amd/ingest.py dispatch_np (the shared case list of
tests/test_ingest_dispatch_host.py):
  - every output array, the run table, the counters and the heartbeat stamps are the definition's;
  - every device array is guarded: every output is sized exactly to the rows the definition writes, with
    canaries before and behind it, every input is as it was, and the inputs begin one element behind an
    aligned address in one of the two runs of a case (the arrays are typed: natural alignment is the
    contract), so the byte arrays sit at odd addresses;
  - every nullable output left out in turn;
  - end to end on one handle: frames -> wq_frames_decode_device -> wq_ingest_dispatch_device ->
    IngestTick.process issuing wq_apply_ops_device / wq_route_tick_device / wq_route_global_device per run,
    over 6,000 random events in ticks of 97 and 400 frames, equals the reference's sequential loop: the
    route calls read slices of the rows that begin at odd rows;
  - one tick of 65,537 frames with 3 run changes; the call alternating with decode, builder and pack."""
import ctypes
import uuid

import numpy as np
import pytest

from worldql_server_amd import abi, ingest

import test_gpu_frames_build as build_gpu
import test_gpu_frames_decode as decode_gpu
import test_gpu_peer_pack as pack_gpu
from test_frames_build_host import WORLDS as BUILD_WORLDS, cases as build_cases, want as build_want
from test_frames_decode_host import PEER_IDS, PEER_UUIDS, batches, same as decode_same
from test_gpu_peer_pack import CANARY8, Bytes
from test_ingest_dispatch_cpp_mirror import WIDTH, rows_written, shape
from test_ingest_dispatch_host import (N_PEERS, OracleRuns, all_worlds, cases, check_events, definition, same, sanitized,
                                       stream, ticks_of, wire)
from tests.seq_reference import SequentialReference

pytestmark = pytest.mark.gpu

IN_WIDTH = dict(instruction=1, flags=1, world=4, sender=4, repl=1, pos=8)   # bytes per element
CSIZE = abi.DISPATCH_COUNTERS_DTYPE.itemsize


class Call:
    """One case on the device: guarded inputs and outputs, and the checks after a call."""

    def __init__(self, d, runs_capacity=None, last_seen=None, now=0, fields=abi.DISPATCH_OUT_ARRAYS, with_counters=True,
                 shift=1, device="cuda:0"):
        self.want = ingest.dispatch_np(d, runs_capacity, last_seen, now)
        self.n = len(d["instruction"])
        self.cap = (self.want["counters"]["n_runs"] + 1 if runs_capacity is None else runs_capacity) if "runs" in fields else 0
        self.src = {k: Bytes(np.ascontiguousarray(d[k]).view(np.uint8).reshape(-1), shift=shift * w, device=device)
                    for k, w in IN_WIDTH.items()}
        self.seen = None if last_seen is None else Bytes(np.asarray(last_seen, np.uint32).view(np.uint8), shift=4 * shift,
                                                         device=device)
        self.a = abi.DispatchIn(**{k: b.ptr for k, b in self.src.items()}, last_seen=self.seen.ptr if self.seen else None,
                                n_last_seen=0 if last_seen is None else len(last_seen), now=now)
        self.rows = {k: rows_written(k, self.want, self.cap) for k in fields}
        self.outs = {k: Bytes(n=self.rows[k] * WIDTH[k], device=device) for k in fields}
        self.cnt = Bytes(n=CSIZE, device=device) if with_counters else None
        self.out = abi.DispatchOut(**{k: b.ptr for k, b in self.outs.items()}, runs_capacity=self.cap)

    def launch(self, r):
        """Enqueues the call; nothing is waited for."""
        r.dispatch_device(self.a, self.n, self.out, self.cnt.ptr if self.cnt else None)

    def outputs(self):
        """A dict like dispatch_np's (outputs left out: None) after the canary checks."""
        import torch
        torch.cuda.synchronize()
        got = dict.fromkeys(abi.DISPATCH_OUT_ARRAYS)
        for k, b in self.outs.items():
            raw = b.read()
            assert (raw[self.rows[k] * WIDTH[k]:] == CANARY8).all(), "written behind " + k
            assert b.front_intact(), "written before " + k
            got[k] = shape(k, raw, self.rows[k])
        if self.cnt:
            raw = self.cnt.read()
            assert (raw[CSIZE:] == CANARY8).all() and self.cnt.front_intact(), "written beside the counters"
            got["counters"] = ingest.dispatch_counters(raw[:CSIZE].copy())
        for k, b in self.src.items():
            assert b.unchanged(), "an input was written: " + k
        if self.seen:
            raw = self.seen.read()
            assert (raw[self.seen.n:] == CANARY8).all() and self.seen.front_intact(), "written beside last_seen"
            got["last_seen"] = raw[:self.seen.n].copy().view(np.uint32)
        return got

    def run(self, r):
        import torch
        torch.cuda.synchronize()
        self.launch(r)
        return self.outputs()

    def check(self, what=""):
        fields = tuple(self.outs)
        want = self.want if "runs" in fields else dict(self.want, counters=dict(self.want["counters"], overflow=1))
        same(self.outputs(), want, what, fields=fields, counters=self.cnt is not None)


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    yield r
    r.close()


# ---- the shared cases ---------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases()))
def test_case_equals_the_definition(router, name):
    """Twice: the inputs one element behind an aligned address, and aligned. 'big_3_changes' is the tick of
    65,537 frames with 3 run changes: 65 blocks under the one scanning block."""
    d, kw = cases()[name]
    for shift in (1, 0):
        c = Call(d, shift=shift, **kw)
        c.launch(router)
        c.check(f"{name} shift {shift}")
        same(c.want, definition(name), name)


def test_nullable_outputs(router):
    d, kw = cases()["mix_4097"]
    all_ = abi.DISPATCH_OUT_ARRAYS
    combos = [tuple(k for k in all_ if k != left_out) for left_out in all_] + [(), ("runs",), ("ops", "l_pos")]
    calls = [Call(d, fields=f, with_counters=wc, **kw) for f in combos for wc in ((True, False) if len(f) < 3 else (True,))]
    for c in calls:
        c.launch(router)
    for c in calls:
        c.check(str(tuple(c.outs)))


def test_runs_capacity(router):
    d, _ = cases()["capacity_n_runs"]
    for cap in (0, 1, 6, 7, 100):
        c = Call(d, runs_capacity=cap)
        c.launch(router)
        c.check(f"capacity {cap}")


def test_two_calls_are_identical_and_scratch_is_reused(router):
    """The same call twice, the largest case after the smallest, and no allocation at steady state."""
    import torch
    d, kw = cases()["big_3_changes"]
    big, small = Call(d, **kw), Call(*cases()["mix_63"][:1], **cases()["mix_63"][1])
    first = big.run(router)
    for _ in range(5):
        free = torch.cuda.mem_get_info()[0]
        small.run(router)
        again = big.run(router)
        same(again, first, "second call", fields=tuple(big.outs))
        after = torch.cuda.mem_get_info()[0]
        assert after >= free, ("a steady-state call allocated", free - after)
        if after == free:
            return
    pytest.fail("the device's free memory kept rising: no quiet pair in five")


def test_dispatch_between_decode_builder_and_pack():
    """Dispatch, decode, build, pack, dispatch on one handle and stream, nothing waited for, both orders."""
    import torch
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    r.set_worlds(BUILD_WORLDS)
    r.set_ingest_peers(PEER_UUIDS, PEER_IDS)
    d1, o1, _ = batches()["corpus_3"]
    w1 = ingest.decode_frames_np(d1, o1, BUILD_WORLDS, PEER_UUIDS, PEER_IDS)
    a = Call(*cases()["quiet_granules"][:1])
    b = Call(cases()["hostile_3000"][0], shift=0, **cases()["hostile_3000"][1])
    dec = decode_gpu.Call(d1, o1)
    f = build_gpu.Call(build_cases()["residues"], len(build_want("residues")[0]))
    p = pack_gpu.Call("tiny_runs", True)
    torch.cuda.synchronize()
    for order in ((a, dec, f, p, b), (p, b, f, a, dec)):
        for x in order:
            x.launch(r)
        a.check("quiet_granules")
        decode_same(dec.outputs(), w1, "corpus_3")
        build_gpu.check(f.outputs(), build_want("residues"), "residues")
        pack_gpu.check("tiny_runs", True, *p.outputs())
        b.check("hostile_3000")
    r.close()


def test_invalid_arguments(router):
    import torch
    from worldql_server_amd.router import WQError, load_library
    d, kw = cases()["mix_65"]
    call = Call(d, **kw)

    def invalid(src=call.a, n=call.n, out=call.out):
        with pytest.raises(WQError) as e:
            router.dispatch_device(src, n, out, call.cnt.ptr)
        assert e.value.code == abi.WQ_E_INVALID

    def without(struct, field):
        c = type(struct)()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(struct), ctypes.sizeof(struct))
        setattr(c, field, None)
        return c

    invalid(src=None)
    invalid(out=None)
    for k in IN_WIDTH:
        invalid(src=without(call.a, k))
    invalid(out=without(call.out, "runs"))
    invalid(n=0xFFFFFFFF)
    lib = load_library()
    assert lib.wq_ingest_dispatch_device(None, ctypes.byref(call.a), call.n, ctypes.byref(call.out), None) == abi.WQ_E_INVALID
    torch.cuda.synchronize()
    for b in list(call.outs.values()) + [call.cnt, call.seen]:
        assert b.unchanged()                               # nothing was launched
    # n_frames == 0 needs no array: the counters and the closing run only
    empty = Call(*cases()["empty"][:1])
    empty.a = abi.DispatchIn()
    empty.launch(router)
    empty.check("empty, null inputs")
    call.launch(router)
    call.check("after the refused calls")


@pytest.mark.parametrize("devices", [(0, 0), (0, 1)], ids=["one_device_twice", "two_devices"])
def test_multi_gpu_handle(devices):
    """A replicate handle over two sub-handles runs the call on its own stream with the arrays on
    devices[0]."""
    import torch
    from worldql_server_amd.router import Router
    if torch.cuda.device_count() <= max(devices):
        pytest.skip("needs two devices")
    r = Router.multi(16, devices, mode="replicate")
    for name in ("mix_4097", "quiet_granules"):
        c = Call(cases()[name][0], **cases()[name][1])
        c.launch(r)
        c.check(name)
    r.close()


# ---- from the wire to the routed runs -----------------------------------------------------------

def test_frames_to_routed_runs_equal_the_sequential_reference():
    """6,000 random events (disconnects left out: they arrive on another channel) in ticks of 97 and 400
    frames on one handle: decode, dispatch, IngestTick.process. Every run's route calls read slices of the
    rows that begin wherever the run before ended, odd rows included. Event by event the recipients are
    the reference's sequential loop's, as sets of uuids."""
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
    rc = torch.zeros(24 * 400, dtype=torch.uint8, device=dev)
    last_seen = torch.zeros(N_PEERS, dtype=torch.int32, device=dev)
    tick = ingest.IngestTick(r, capacity=16)
    ref = SequentialReference(16)
    nonempty = n_runs = odd_slices = 0
    for t, chunk in enumerate(ticks_of(events, (97, 400))):
        data, offsets = wire(chunk)
        d_frames = torch.from_numpy(data.copy()).to(dev)
        d_off = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        tick.decode(d_frames, d_off).dispatch(last_seen=last_seen, now=t + 1)
        cnt, runs, reads = tick.process(offs, out_peers, rc)
        got_d = tick.read_dispatch()
        o, p = offs.cpu().numpy().view(np.uint32), out_peers.cpu().numpy().view(np.uint32)
        route_cnt = rc.cpu().numpy().view(abi.COUNTERS_DTYPE)
        assert cnt["error"] == 0 and cnt["n_frames"] == len(chunk) and cnt["n_bad"] == 0
        sb = cnt["side_begin"]
        assert all(sanitized(chunk[i].world_name) is None for i in got_d["side_src"][sb[4]:sb[5]])  # refused names
        n_runs += cnt["n_runs"]
        res = [None] * len(chunk)
        for read in reads:
            for key, src in (("local", got_d["l_src"]), ("global", got_d["g_src"])):
                reg = read[key]
                if reg is None:
                    continue
                c = route_cnt[reg["call"]]
                assert c["error"] == 0 and c["overflow"] == 0, (t, read, c)
                lo, hi = reg["rows"]
                odd_slices += lo % 2
                ro = o[reg["offsets"]:reg["offsets"] + hi - lo + 1]
                assert ro[0] == 0 and ro[-1] == c["n_pairs"]
                for k in range(hi - lo):
                    res[int(src[lo + k])] = p[reg["peers"] + ro[k]:reg["peers"] + ro[k + 1]].tolist()
        dec = dict(repl=tick.buf["repl"][:len(chunk)].cpu().numpy())
        nonempty += check_events(chunk, dec, got_d, res, ref, lambda ids: [f"peer-{q}" for q in ids])
    assert r.route_health() == (0, 0)
    assert nonempty > 500 and n_runs > 1000 and odd_slices > 100
    r.close()


def test_process_equals_the_runs_on_the_oracle():
    """One tick of 400 events: the calls IngestTick.process issues are the runs OracleRuns executes from
    dispatch_np's tables, row for row."""
    import torch
    from worldql_server_amd.router import Router
    events = stream(420, seed=3)[:400]
    worlds, peers = all_worlds(), [uuid.UUID(int=k + 1) for k in range(N_PEERS)]
    data, offsets = wire(events)
    dec = ingest.decode_frames_np(data, offsets, worlds, peers)
    disp = ingest.dispatch_np(dec)
    want = OracleRuns(16).execute(disp, len(events))
    r = Router(16, 0)
    r.set_worlds(worlds)
    r.set_ingest_peers(peers)
    dev = torch.device("cuda:0")
    offs = torch.zeros(2008, dtype=torch.int32, device=dev)
    out_peers = torch.zeros(400 * 512, dtype=torch.int32, device=dev)
    tick = ingest.IngestTick(r)
    d_frames = torch.from_numpy(data.copy()).to(dev)            # kept: the decode reads them on the handle's stream
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
    tick.decode(d_frames, d_off).dispatch()
    cnt, runs, reads = tick.process(offs, out_peers)
    got_d = tick.read_dispatch()
    same(got_d, disp, "tick", fields=ingest.DISPATCH_ROWS + ("runs",))
    assert runs.tobytes() == disp["runs"].tobytes()
    o, p = offs.cpu().numpy().view(np.uint32), out_peers.cpu().numpy().view(np.uint32)
    res = [None] * len(events)
    for read in reads:
        for key, src in (("local", disp["l_src"]), ("global", disp["g_src"])):
            reg = read[key]
            if reg is not None:
                lo, hi = reg["rows"]
                ro = o[reg["offsets"]:reg["offsets"] + hi - lo + 1]
                for k in range(hi - lo):
                    res[int(src[lo + k])] = p[reg["peers"] + ro[k]:reg["peers"] + ro[k + 1]].tolist()
    assert sum(bool(x) for x in want) > 20 and len(reads) > 50          # the oracle's tick is not a trivial one
    for k, (g, w) in enumerate(zip(res, want)):
        assert g == w, (k, events[k], g, w)
    r.close()
