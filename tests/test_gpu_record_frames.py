"""GPU parity for the record reply builder (include/wq_router.h wq_frames_build_records_device, csrc/wq_reply.hip) and
records.DeviceRecordProcessor.process_frames.

Bars, all bit-exact against worldql_server_amd/frames.py build_record_frames_np (the cases of
tests/test_record_frames_cpp_mirror.py):
  - frames, offsets, sizes and counters are the definition's, and byte-identical on a second call;
  - guard words around every output, the inputs as they were;
  - capacity cuts, the sizing call, the nullable outputs, the 2^30 rule without payload memory;
  - a 1 MiB flex stored by wq_slab_store_device and returned in a reply;
  - end to end on one handle: 3,000 random events in ticks of 97 and 400 frames through process_frames on a
    GpuRecordStore; the device frames, decoded, equal RecordProcessor.process's replies on the Python store tick by
    tick (recipients, world names, records in order, store totals), and go through wq_peer_major_device and
    wq_peer_pack_device to the bytes of the host-serialized replies packed per peer by peer_pack_np."""
import uuid

import numpy as np
import pytest

from worldql_server_amd import abi, codec, frames, ingest, interest, records
from worldql_server_amd.world_names import sanitize_world_name

from test_gpu_peer_pack import CANARY8, Bytes
from test_record_frames_cpp_mirror import CASES, IDS, small_case, too_large_case
from test_record_frames_host import WORLDS as TABLE

pytestmark = pytest.mark.gpu

CSIZE = abi.FRAMES_COUNTERS_DTYPE.itemsize


@pytest.fixture(scope="module")
def router():
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    r.set_worlds(TABLE)
    yield r
    r.close()


class Call:
    def __init__(self, case, capacity, with_size=True, with_counters=True, shift=1):
        self.case, self.capacity, self.src_bytes = case, capacity, []

        def put(a, always):
            if not a.size and not always:
                return None
            b = Bytes(a if a.size else np.zeros(0, np.uint8), shift=0 if a.size % 64 == 0 and a.size else shift)
            self.src_bytes.append(b)
            return b.ptr

        # the slab's entries must stay 16-byte aligned: 64-byte multiples are placed unshifted above
        self.src, self.rec = case.marshal(put)
        self.out = Bytes(n=capacity)
        self.offs, self.size = Bytes(n=8 * (case.n + 1)), Bytes(n=4 * case.n) if with_size else None
        self.cnt = Bytes(n=CSIZE) if with_counters else None

    def launch(self, r):
        r.build_record_frames_device(self.src, self.rec, self.case.n, self.out.ptr if self.capacity else None, self.capacity,
                                     self.offs.ptr, self.size.ptr if self.size else None, self.cnt.ptr if self.cnt else None)

    def outputs(self):
        import torch
        torch.cuda.synchronize()
        n = self.case.n
        raw = self.offs.read()
        assert (raw[8 * (n + 1):] == CANARY8).all() and self.offs.front_intact()
        offs = raw[:8 * (n + 1)].copy().view(np.uint64)
        written = min(self.capacity, int(offs[n]))
        raw = self.out.read()
        assert (raw[written:] == CANARY8).all() and self.out.front_intact(), "written outside the frames"
        got = [raw[:written].copy(), offs, None, None]
        if self.size:
            raw = self.size.read()
            assert (raw[4 * n:] == CANARY8).all() and self.size.front_intact()
            got[2] = raw[:4 * n].copy().view(np.uint32)
        if self.cnt:
            raw = self.cnt.read()
            assert (raw[CSIZE:] == CANARY8).all() and self.cnt.front_intact()
            c = raw[:CSIZE].copy().view(abi.FRAMES_COUNTERS_DTYPE)[0]
            got[3] = {k: int(c[k]) for k in abi.FRAMES_COUNTERS_DTYPE.names}
        for b in self.src_bytes:
            assert b.unchanged(), "an input was written"
        return got

    def check(self, r, want):
        self.launch(r)
        got = self.outputs()
        assert np.array_equal(got[1], want[1]), (self.case.name, "offsets")
        assert got[2] is None or np.array_equal(got[2], want[2]), (self.case.name, "sizes")
        assert got[3] is None or got[3] == want[3], (self.case.name, got[3], want[3])
        assert np.array_equal(got[0], want[0]), (self.case.name, "frames")
        return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_equals_the_definition(router, case):
    want = case.want()
    need = want[3]["bytes_need"]
    first = Call(case, need).check(router, want)
    second = Call(case, need, shift=3).check(router, want)
    assert first[0].tobytes() == second[0].tobytes()
    Call(case, need + 48, with_size=False, with_counters=False).check(router, want)
    Call(case, 0).check(router, case.want(0))
    if need > 40:
        for cap in (need - 1, (need // 2) & ~15, 17):
            Call(case, cap).check(router, case.want(cap))


def test_capacity_sweep_of_a_small_case(router):
    case = small_case()
    need = case.want()[3]["bytes_need"]
    for cap in list(range(0, 40)) + list(range(need - 40, need + 2)):
        Call(case, cap).check(router, case.want(cap))


def test_too_large_through_the_sizing_call(router):
    case = too_large_case()
    want = case.want(0)
    assert want[3]["error"] == frames.ERROR_TOO_LARGE
    Call(case, 0).check(router, want)


def test_validation(router):
    from worldql_server_amd.router import WQError
    c = Call(small_case(), 64)
    c.rec.flags = 2
    with pytest.raises(WQError):
        c.launch(router)
    c.rec.flags = 0
    c.rec.slab.entries += 8
    with pytest.raises(WQError):
        c.launch(router)


# ---- from the wire to the reply frames --------------------------------------------------------------------

def decode_replies(out):
    """process_frames's device frames as [(recipient, world_name, [(uuid, position, data, flex)])], empty frames left out."""
    data, off = out["frames"].cpu().numpy(), out["offsets"].cpu().numpy().astype(np.uint64)
    rcp = out["recipients"].cpu().numpy().view(np.uint32)
    msgs = codec.decode_packed(data, off) if len(off) > 1 else []
    got = []
    for i, m in enumerate(msgs):
        if off[i + 1] == off[i]:
            continue
        fr = data[int(off[i]):int(off[i + 1])].tobytes()
        assert m["status"] == 0 and m["instruction"] == 12 and m["n_entities"] == 0 and bytes(m["sender_uuid"]) == bytes(16)
        mm = {k: m[k] for k in m.dtype.names}
        mm["instruction"] = 8
        recs = [ingest.deferred_event(fr, mm, k)["records"][0] for k in range(int(m["n_records"]))]
        w0 = int(m["world_off"])
        got.append((int(rcp[i]), fr[w0:w0 + int(m["world_len"])].decode(), recs))
    return got


def test_frames_to_reply_frames_equal_the_record_processor():
    import torch
    from test_gpu_records_dispatch import open_router, reference_processor, ticks_of
    from test_records_dispatch_host import NOW, PEERS, WORLDS, processor_events, random_events, wire
    events = random_events(3000, seed=21, p_record=0.4, max_records=6)
    r, store = open_router()
    dev = records.DeviceRecordProcessor(store, ingest.IngestTick(r, capacity=16), WORLDS)
    ref = reference_processor()
    peer_of = {u.bytes: i for i, u in enumerate(PEERS)}
    n_replies = n_records = 0
    for t, chunk in enumerate(ticks_of(events, (97, 400))):
        data, offsets = wire(chunk)
        out = dev.process_frames(data, offsets, NOW + 1000 * t)
        want = ref.process(processor_events(chunk), NOW + 1000 * t)
        got = decode_replies(out)
        assert len(got) == len(want), t
        host_msgs = []
        for (rcp, world, recs), (su, w_world, w_recs) in zip(got, want):
            assert world == w_world, t
            # the reference's reply lists its rows in store order; both stores return a row's records by ascending uuid
            assert [(x["uuid"], x["position"], x["data"], x["flex"]) for x in recs] == \
                   [(tuple(x["uuid"]), tuple(x["position"]), x["data"], x["flex"]) for x in w_recs], t
            assert rcp == peer_of.get(su.bytes, 0xFFFFFFFF), t
            host_msgs.append(dict(instruction=12, world_name=w_world, records=[
                dict(uuid=uuid.UUID(int=(x["uuid"][0] << 64) | x["uuid"][1]), world_name=sanitize_world_name(x["world_name"]),
                     position=x["position"],
                     data=x["data"], flex=x["flex"]) for x in w_recs]))
        n_replies += len(want)
        n_records += sum(len(w[2]) for w in want)
        # the non-empty device frames are the host serializer's bytes, and pack alike
        sizes = out["sizes"].cpu().numpy()
        keep = np.flatnonzero(sizes)
        assert len(keep) == len(want)
        if len(want):
            h_data, h_off = codec.serialize_messages(host_msgs)
            d_data, d_off = out["frames"].cpu().numpy(), out["offsets"].cpu().numpy().astype(np.uint64)
            assert np.array_equal(d_data, h_data) and np.array_equal(d_off[np.r_[keep, len(sizes)]], h_off), t
            pack_and_compare(r, out, keep, [g[0] for g in got], h_data, h_off)
    assert n_replies > 100 and n_records > 300
    assert dev.totals() == ref.store.totals() and store.stats()[0] == ref.store.stats()[0] > 100
    store.close()
    r.close()


def pack_and_compare(r, out, keep, recipients, h_data, h_off):
    """A one-recipient-per-row CSR over the tick's frames through wq_peer_major_device and wq_peer_pack_device against the
    host frames packed per peer by peer_pack_np."""
    import torch
    dev = out["frames"].device
    n = out["sizes"].numel()
    known = [(int(i), p) for i, p in zip(keep, recipients) if p != 0xFFFFFFFF]
    if not known:
        return
    n_peers = max(p for _, p in known) + 1
    # message-major: row i holds frame i's one recipient (none for an empty frame or an unknown sender)
    cnt = np.zeros(n, np.int64)
    cnt[[i for i, _ in known]] = 1
    m_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    m_peers = np.array([p for _, p in known], np.uint32)
    p_off, p_msgs = interest.peer_major_np(m_off, m_peers, n_peers)
    # the same lists over the host's frames, whose index is the position among the non-empty ones
    rank = {int(i): k for k, i in enumerate(keep)}
    want = interest.peer_pack_np(p_off, np.array([rank[int(m)] for m in p_msgs], np.uint32), h_data, h_off, len_prefix=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype).copy()).to(dev)   # noqa: E731
    d_moff, d_mpeers = t(m_off), t(m_peers)
    d_poff = torch.empty(n_peers + 1, dtype=torch.int32, device=dev)
    d_pmsgs = torch.empty(max(len(m_peers), 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    r.peer_major_device(d_moff.data_ptr(), d_mpeers.data_ptr(), n, len(m_peers), None, n_peers, d_poff.data_ptr(), d_pmsgs.data_ptr())
    need = want[3]["bytes_need"]
    assert want[3]["error"] == 0 and need == len(want[0])
    d_out = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    d_pb = torch.empty(n_peers + 1, dtype=torch.int64, device=dev)
    r.peer_pack_device(d_poff.data_ptr(), d_pmsgs.data_ptr(), n_peers, len(m_peers), out["frames"].data_ptr(), out["offsets"].data_ptr(),
                       n, out["frames"].numel(), abi.PACK_LEN_PREFIX, d_out.data_ptr(), need, d_pb.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert np.array_equal(d_out[:need].cpu().numpy(), want[0]) and np.array_equal(d_pb.cpu().numpy().astype(np.uint64), want[1])


def test_a_1_mib_flex_stored_and_returned():
    """One create with a 1 MiB flex through the wire into the slab, one read: the reply frame holds it."""
    import torch
    from test_gpu_records_dispatch import open_router
    from test_records_dispatch_host import NOW, PEERS, WORLDS, wire
    flex = bytes(np.random.default_rng(4).integers(0, 256, 1 << 20, dtype=np.uint8))
    u = uuid.UUID(int=0xABCDEF)
    sender = PEERS[0]
    rec = dict(uuid=u, world_name=WORLDS[0], position=(1.0, 2.0, 3.0), data="big", flex=flex)
    evs = [dict(instruction=8, sender_uuid=sender, world_name=WORLDS[0], records=[rec]),
           dict(instruction=9, sender_uuid=sender, world_name=WORLDS[0], position=(1.0, 2.0, 3.0))]
    data, offsets = codec.serialize_messages(evs)
    r, store = open_router()
    dev = records.DeviceRecordProcessor(store, ingest.IngestTick(r, capacity=16), WORLDS)
    out = dev.process_frames(data, offsets, NOW)
    got = decode_replies(out)
    assert len(got) == 1 and len(got[0][2]) == 1 and got[0][2][0]["flex"] == flex and got[0][2][0]["data"] == "big"
    assert int(out["sizes"][0]) > 1 << 20 and dev.dslab.cursor == (1 << 20) + 3
    store.close()
    r.close()
