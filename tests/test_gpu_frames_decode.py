"""GPU parity for the ingest decoder (include/wq_router.h wq_frames_decode_device, csrc/wq_decode.hip): a
tick's received frames verified, decoded and resolved on the device.

Bars, all bit-exact against worldql_server_amd/ingest.py decode_frames_np, which is the host decoder
under the call's rules (the shared case list of tests/test_frames_decode_host.py):
  - every output array and the counters are the definition's, for the golden frames, a seeded corpus,
    long strings on the list and the lane path, records, truncations, offset errors and table changes;
  - every device array is guarded: the frame bytes are sized exactly to n_frame_bytes, every output has
    canaries before and behind it, every input is as it was, and the inputs sit at odd addresses in one
    of the two runs of a case;
  - decode -> wq_route_tick_device straight from the decode's arrays equals the oracle on the
    host-decoded fields, with nothing waited for in between;
  - the call alternates with the builder and the pack on one handle."""
import ctypes
import uuid

import numpy as np
import pytest

from oracle import oracle as orc
from worldql_server_amd import abi, codec, ingest

import test_gpu_frames_build as build_gpu
import test_gpu_peer_pack as pack_gpu
from test_frames_build_host import WORLDS as BUILD_WORLDS, cases as build_cases, want as build_want
from test_frames_decode_host import PEER_IDS, PEER_UUIDS, WORLDS, batches, definition, flat, same
from test_gpu_peer_budget import CANARY, Guarded
from test_gpu_peer_pack import CANARY8, Bytes

pytestmark = pytest.mark.gpu

WIDTH = dict(msg=72, pos=24, world=4, sender=4, repl=1, instruction=1, sender_uuid=16, flex_range=8, flags=1)
SHAPE = dict(msg=lambda a, n: a.view(codec.DECODED_DTYPE), pos=lambda a, n: a.view(np.float64).reshape(n, 3),
             world=lambda a, n: a.view(np.uint32), sender=lambda a, n: a.view(np.uint32), repl=lambda a, n: a,
             instruction=lambda a, n: a, sender_uuid=lambda a, n: a.reshape(n, 16),
             flex_range=lambda a, n: a.view(np.uint32).reshape(n, 2), flags=lambda a, n: a)


class Call:
    """One batch on the device: guarded inputs and outputs, and the checks after a call."""

    def __init__(self, data, offsets, nb=None, device="cuda:0", fields=ingest.OUT_FIELDS, with_counters=True, shift=1):
        self.n = len(offsets) - 1
        self.nb = len(data) if nb is None else nb
        self.frames = Bytes(np.asarray(data, np.uint8), shift=shift, device=device) if len(data) else None
        off = np.asarray(offsets, np.uint64)
        self.off = Bytes(off.view(np.uint8), shift=0, device=device)     # 8-byte aligned
        self.outs = {k: Bytes(n=self.n * WIDTH[k], device=device) for k in fields}
        self.cnt = Guarded(n=16, device=device) if with_counters else None
        self.out = abi.IngestOut(**{k: b.ptr for k, b in self.outs.items()})

    def launch(self, r):
        """Enqueues the call; nothing is waited for."""
        r.decode_frames_device(self.frames.ptr if self.frames else None, self.off.ptr, self.n, self.nb, self.out,
                               self.cnt.ptr if self.cnt else None)

    def outputs(self):
        """A dict like decode_frames_np's (outputs left out: None) after the canary checks."""
        import torch
        torch.cuda.synchronize()
        n = self.n
        got = dict.fromkeys(ingest.OUT_FIELDS)
        for k, b in self.outs.items():
            raw = b.read()
            assert (raw[n * WIDTH[k]:] == CANARY8).all(), "written behind " + k
            assert b.front_intact(), "written before " + k
            got[k] = SHAPE[k](raw[:n * WIDTH[k]].copy(), n)
        if self.cnt:
            c = self.cnt.read(np.uint8)[:64].view(abi.INGEST_COUNTERS_DTYPE)[0]
            got["counters"] = {k: int(c[k]) for k in abi.INGEST_COUNTERS_DTYPE.names if k != "pad_"}
            assert c["pad_"] == 0 and (self.cnt.read()[16:] == CANARY).all() and self.cnt.front_intact()
        assert self.off.unchanged() and (self.frames is None or self.frames.unchanged()), "an input was written"
        return got

    def run(self, r):
        import torch
        torch.cuda.synchronize()
        self.launch(r)
        return self.outputs()


def run_case(r, name, **kw):
    data, offsets, nb = batches()[name]
    got = Call(data, offsets, nb, **kw).run(r)
    same(got, definition(name), name)
    return got


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    r.set_worlds(WORLDS)
    r.set_ingest_peers(PEER_UUIDS, PEER_IDS)
    yield r
    r.close()


# ---- the shared cases ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["golden", "corpus_1"])
def test_corpus_equals_the_definition(router, name):
    """All four statuses, every output and the counters; twice, the frames at odd and at aligned addresses."""
    a = run_case(router, name)
    b = run_case(router, name, shift=0)
    for k in ingest.OUT_FIELDS:
        assert a[k].tobytes() == b[k].tobytes()
    assert a["counters"] == b["counters"] and min(a["counters"][k] for k in ("n_ok", "n_invalid", "n_missing", "n_bad_uuid")) > 0


@pytest.mark.parametrize("entries", [0, -1], ids=["no_list", "default_list"])
def test_long_strings_on_the_lane_and_on_the_list(router, entries):
    """Parameters of L - 1 .. L + 1, 4095 .. 4097 and 1 MiB with a bad byte first, last and beside chunk and
    tile boundaries; multi-byte sequences across the boundaries at every split. Without a list every lane
    validates its own long strings."""
    router.set_ingest_list(entries)
    try:
        run_case(router, "long_strings")
        run_case(router, "straddle", shift=3)
        run_case(router, "nul")
    finally:
        router.set_ingest_list(-1)


def test_records_and_entities(router):
    """0, 1, 3 and 300 records, the decode errors' ranks; one frame of 300 records among 1,000 flat ones."""
    run_case(router, "records")
    got = run_case(router, "records_among_flat")
    assert got["counters"]["n_ok"] == 1001 and got["msg"]["n_records"][500] == 300
    run_case(router, "hand", shift=5)


def test_truncation_sweep_in_one_batch(router):
    """Every strict truncation of the 136-byte frame and the frame itself: 137 frames."""
    got = run_case(router, "truncations_136")
    assert got["counters"]["n_frames"] == 137
    run_case(router, "truncations_nested", shift=0)
    run_case(router, "corruptions_136")


def test_offset_errors(router):
    for name, bit in (("offsets_descend_past", abi.INGEST_ERROR_OFFSETS), ("offsets_cut_buffer", abi.INGEST_ERROR_OFFSETS),
                      ("offsets_huge", abi.INGEST_ERROR_HUGE)):
        assert run_case(router, name)["counters"]["error"] == bit
    got = run_case(router, "empty")
    assert got["counters"] == dict.fromkeys(got["counters"], 0)


def test_nullable_outputs(router):
    data, offsets, nb = batches()["corpus_2"]
    for fields, with_counters in (((), True), (("msg",), False), (("pos", "world", "sender", "repl"), True),
                                  (tuple(k for k in ingest.OUT_FIELDS if k != "msg"), True), (("flags", "flex_range"), False)):
        same(Call(data, offsets, nb, fields=fields, with_counters=with_counters).run(router), definition("corpus_2"), str(fields))


def test_tables_none_cleared_and_set_twice():
    """A handle with no table; tables set, replaced and cleared between decodes on one stream, nothing
    waited for; a refused sender table leaves the old one."""
    import torch
    from worldql_server_amd.router import Router, WQError
    data, offsets, _ = batches()["hand"]
    r = Router(16, 0)
    tables = ((None, None, None), (WORLDS, PEER_UUIDS, PEER_IDS), (WORLDS[::-1], PEER_UUIDS[::-1], None),
              ([], [], None), (["world"] * 40 + WORLDS, PEER_UUIDS[:2], [9, 8]))
    calls = []
    torch.cuda.synchronize()
    for worlds, uuids, ids in tables:
        if worlds is not None:
            r.set_worlds(worlds)
            r.set_ingest_peers(uuids, ids)
        c = Call(data, offsets)
        c.launch(r)
        calls.append((c, ingest.decode_frames_np(data, offsets, worlds, uuids, ids)))
    for c, w in calls:
        same(c.outputs(), w, "tables replaced")
    with pytest.raises(WQError) as e:
        r.set_ingest_peers([PEER_UUIDS[0], PEER_UUIDS[1], PEER_UUIDS[0]])
    assert e.value.code == abi.WQ_E_INVALID
    same(Call(data, offsets).run(r), calls[-1][1], "after the refused table")
    r.close()


def test_two_calls_are_identical_and_scratch_is_reused(router):
    """The same call twice, the largest case after the smallest, and no allocation at steady state."""
    import torch
    d, o, nb = batches()["long_strings"]
    big, small = Call(d, o, nb), Call(*batches()["nul"])
    first = big.run(router)
    same(first, definition("long_strings"))
    for _ in range(5):
        free = torch.cuda.mem_get_info()[0]
        small.run(router)
        again = big.run(router)
        for k in ingest.OUT_FIELDS:
            assert again[k].tobytes() == first[k].tobytes()
        assert again["counters"] == first["counters"]
        after = torch.cuda.mem_get_info()[0]
        assert after >= free, ("a steady-state call allocated", free - after)
        if after == free:
            return
    pytest.fail("the device's free memory kept rising: no quiet pair in five")


def test_decode_between_the_builder_and_the_pack():
    """Decode, build, pack, decode on one handle and stream, nothing waited for, both orders."""
    import torch
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    r.set_worlds(BUILD_WORLDS)
    r.set_ingest_peers(PEER_UUIDS, PEER_IDS)
    d1, o1, _ = batches()["corpus_3"]
    d2, o2, _ = batches()["straddle"]
    w1 = ingest.decode_frames_np(d1, o1, BUILD_WORLDS, PEER_UUIDS, PEER_IDS)
    w2 = ingest.decode_frames_np(d2, o2, BUILD_WORLDS, PEER_UUIDS, PEER_IDS)
    a, b = Call(d1, o1), Call(d2, o2, shift=0)
    f = build_gpu.Call(build_cases()["residues"], len(build_want("residues")[0]))
    p = pack_gpu.Call("tiny_runs", True)
    torch.cuda.synchronize()
    for order in ((a, f, p, b), (p, b, f, a)):
        for x in order:
            x.launch(r)
        same(a.outputs(), w1, "corpus_3")
        build_gpu.check(f.outputs(), build_want("residues"), "residues")
        pack_gpu.check("tiny_runs", True, *p.outputs())
        same(b.outputs(), w2, "straddle")
    r.close()


# ---- arguments ------------------------------------------------------------------------------

def test_invalid_arguments(router):
    import torch
    from worldql_server_amd.router import WQError, load_library
    data, offsets, nb = batches()["nul"]
    call = Call(data, offsets, nb)

    def invalid(**kw):
        a = dict(frames_ptr=call.frames.ptr, frame_offsets_ptr=call.off.ptr, n_frames=call.n, n_frame_bytes=call.nb,
                 out=call.out, counters_ptr=call.cnt.ptr)
        a.update(kw)
        with pytest.raises(WQError) as e:
            router.decode_frames_device(**a)
        assert e.value.code == abi.WQ_E_INVALID

    invalid(out=None)
    invalid(frame_offsets_ptr=None)
    invalid(frames_ptr=None)
    invalid(n_frames=0xFFFFFFFF)
    lib = load_library()
    vp = ctypes.c_void_p
    assert lib.wq_frames_decode_device(None, vp(call.frames.ptr), vp(call.off.ptr), call.n, call.nb, ctypes.byref(call.out),
                                       None) == abi.WQ_E_INVALID
    assert lib.wq_ingest_set_peers(None, None, None, 0) == abi.WQ_E_INVALID
    assert lib.wq_ingest_set_peers(router.h, None, None, 3) == abi.WQ_E_INVALID
    torch.cuda.synchronize()
    for b in list(call.outs.values()) + [call.cnt]:
        assert b.unchanged()                               # nothing was launched
    same(call.run(router), definition("nul"), "after the refused calls")


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
    r.set_ingest_peers(PEER_UUIDS, PEER_IDS)
    run_case(r, "corpus_2")
    run_case(r, "records")
    r.close()


# ---- from the wire to the routed tick ---------------------------------------------------------

def test_decode_then_route_on_the_device():
    """2,000 LocalMessage frames over 3 worlds and 40 peers, with unknown senders, one unknown world, some
    "@global" and some frames that do not decode: IngestTick.decode, then wq_route_tick_device straight
    from the decode's arrays, nothing waited for in between. The CSR is the oracle's on the host-decoded
    fields with the same ids."""
    import torch
    from worldql_server_amd.router import Router
    rng = np.random.default_rng(77)
    names = ["overworld", "nether", "chat_fs_lobby"]
    wire = ["overworld", "nether", "chat/lobby"]
    n_peers, M = 40, 2000
    peers = [uuid.UUID(int=int(v)) for v in rng.integers(1, 1 << 62, n_peers)]
    ops = abi.ops_array(rng.integers(0, 3, 400), rng.integers(0, n_peers, 400), np.zeros(400, np.uint8),
                        pos=rng.uniform(-24, 24, (400, 3)))
    frames = []
    for i in range(M):
        k = rng.integers(0, 100)
        sender = peers[rng.integers(0, n_peers)] if k >= 10 else uuid.UUID(int=(1 << 100) + int(rng.integers(1, 1 << 62)))
        world = "unheard_of" if i == 1234 else "@global" if k == 50 else wire[rng.integers(0, 3)]
        f = flat(world_name=world, sender_uuid=str(sender) if k % 3 else sender.hex, replication=int(rng.integers(0, 4)),
                 position=tuple(rng.uniform(-24, 24, 3)), parameter=None if k % 2 else "x" * int(k))
        frames.append(f[:-8] if k == 77 else f)
    data, offsets = codec.pack_frames(frames)
    want = ingest.decode_frames_np(data, offsets, names, peers)
    c = want["counters"]
    assert c["n_world_unresolved"] == 1 and c["n_sender_unknown"] > 50 and 0 < c["n_invalid"] < 100

    r = Router(16, 0)
    r.apply_ops(ops)
    r.set_worlds(names)
    r.set_ingest_peers(peers)
    dev = torch.device("cuda:0")
    d_frames = torch.from_numpy(data.copy()).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
    cap = 64 * M
    offs = torch.empty(M + 1, dtype=torch.int32, device=dev)
    out_peers = torch.empty(cap, dtype=torch.int32, device=dev)
    cnt = torch.zeros(24, dtype=torch.uint8, device=dev)
    tick = ingest.IngestTick(r, capacity=16)
    torch.cuda.synchronize()
    tick.decode(d_frames, d_off)
    tick.route(offs.data_ptr(), out_peers.data_ptr(), None, cap, cnt.data_ptr())
    got = tick.read()
    same(got, want, "ingest tick")

    o = orc.COracle(16)
    o.apply_ops(ops)
    o_offs, o_peers, _ = o.route(want["pos"], want["world"], want["sender"], want["repl"])
    rc = cnt.cpu().numpy().view(abi.COUNTERS_DTYPE)[0]
    assert rc["error"] == 0 and rc["overflow"] == 0 and int(rc["n_pairs"]) == len(o_peers) > M
    assert (offs.cpu().numpy().view(np.uint32) == o_offs).all()
    assert (out_peers[:len(o_peers)].cpu().numpy().view(np.uint32) == o_peers).all()
    lens = np.diff(o_offs.astype(np.int64))
    assert (lens[want["flags"] == 0] == 0).all() and (lens[want["world"] >= abi.WORLD_GLOBAL] == 0).all()
    r.close()
