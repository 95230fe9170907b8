"""The device record path across compactions and a restart, from the wire: three DeviceRecordProcessors on three
routers and stores take the same ticks of random frames through process_frames.

  A never compacts;
  B compacts whenever 3% of its arena is dead (many times in this run);
  C starts halfway, restored from the file B's snapshot was saved to.

Every tick B's output equals A's byte for byte (frames, offsets, sizes, recipients), and from the restore on C's
does too; at the end the totals, the live rows and the slabs' canonical forms are equal.

The seed and mix were fixed after a run of the same events through RecordProcessor on a RecordStoreRef with the
slab's bytes counted on the host: 2,400 events, 10 ticks, 6,572 payload bytes stored of which 1,716 end dead, six
compactions at this threshold. The test asserts what keeps it from passing vacuously: A ends with dead bytes, B
compacted at least twice, on both sides of the restore, and B's cursor is below A's."""
import numpy as np
import pytest

from worldql_server_amd import ingest, records

pytestmark = pytest.mark.gpu

N_EVENTS, SEED, P_RECORD, COMPACT_AT = 2400, 33, 0.6, 0.03


def outputs(out):
    return {k: out[k].cpu().numpy() for k in ("frames", "offsets", "sizes", "recipients")}


def same(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


def test_compacting_and_restored_processors_answer_as_the_plain_one(tmp_path):
    from test_gpu_records_dispatch import open_router, ticks_of
    from test_records_dispatch_host import NOW, WORLDS, random_events, wire
    events = random_events(N_EVENTS, seed=SEED, p_record=P_RECORD, max_records=6)
    ticks = list(ticks_of(events, (97, 400)))
    half = len(ticks) // 2
    opened = [open_router() for _ in range(3)]
    procs = [records.DeviceRecordProcessor(store, ingest.IngestTick(r, capacity=16), WORLDS, compact_at=at)
             for (r, store), at in zip(opened, (None, COMPACT_AT, COMPACT_AT))]
    a, b, c = procs
    path = tmp_path / "records.npz"
    n_frames = n_bytes = at_restore = 0
    for t, chunk in enumerate(ticks):
        if t == half:
            records.save_snapshot(path, b.snapshot())
            cnt = c.restore(records.load_snapshot(path))
            assert cnt["error"] == 0 and cnt["n_live"] > 100
            at_restore = b.dslab.compactions
            assert c.totals() == b.totals() and c.d_free == b.d_free and c.d_next == b.d_next
        data, offsets = wire(chunk)
        now = NOW + 1000 * t
        want = outputs(a.process_frames(data, offsets, now))
        assert same(outputs(b.process_frames(data, offsets, now)), want), t
        if t >= half:
            assert same(outputs(c.process_frames(data, offsets, now)), want), t
        n_frames += int(np.count_nonzero(want["sizes"]))
        n_bytes += len(want["frames"])
    assert len(ticks) == 10 and n_frames > 100 and n_bytes > 10000
    # not vacuous: A holds dead bytes, B compacted on both sides of the restore, and its arena is the shorter
    assert a.dslab.compactions == 0 and a.dslab.dead_bytes > 0
    assert at_restore >= 1 and b.dslab.compactions - at_restore >= 1 and b.dslab.compactions >= 2
    assert b.dslab.cursor < a.dslab.cursor and c.dslab.cursor < a.dslab.cursor
    # the same state at the end
    assert a.totals() == b.totals() == c.totals()
    live = [store.stats()[0] for _, store in opened]
    assert live[0] == live[1] == live[2] > 100
    assert a.d_free == b.d_free == c.d_free and a.d_next == b.d_next == c.d_next
    ea, eb, ec = a.dslab.export(), b.dslab.export(), c.dslab.export()
    assert len(ea[0]) > 100 and len(ea[1]) > 1000
    for other in (eb, ec):
        assert other[0].tobytes() == ea[0].tobytes() and np.array_equal(other[1], ea[1])
    for r, store in opened:
        store.close()
        r.close()
