"""The record dispatch's definition (worldql_server_amd/ingest.py records_dispatch_np) against
records.RecordProcessor: for random event lists and a table of named cases, the ops arrays and read batches
of the definition's runs equal, call by call, what a RecordProcessor over a recording stub store receives.
The cases and helpers here are shared by the CPU mirror (tests/test_records_dispatch_cpp_mirror.py) and the
GPU instance (tests/test_gpu_records_dispatch.py). No GPU needed."""
import functools
import random
import struct
import uuid

import numpy as np
import pytest

from worldql_server_amd import abi, codec, ingest, records
from worldql_server_amd.world_names import WorldIds

from fbs_builder import message

SIZES, TABLE_SIZE = (16, 16, 16), 1024
WORLDS = ["world", "w00", "chat_fs_server_1", "a_b", "arena", "lobby", "x_at_y", "Z9"]   # the handle's table, sanitized
RAW_NAMES = ["world", "w00", "chat/server_1", "a b", "arena", "lobby", "x@y", "Z9"]     # names that sanitize to it
REFUSED = ["0bad", "", "x" * 70, "café", "@global"]
UNKNOWN = ["elsewhere", "nowhere"]
PEERS = [uuid.UUID(int=k + 1) for k in range(8)]
NOW = 1_700_000_000_000_000
INS = {"RecordCreate": 8, "RecordRead": 9, "RecordDelete": 11, "LocalMessage": 7, "Heartbeat": 0, "RecordUpdate": 10}
ARRAYS = ("cls", "ops", "op_ref", "q_src", "q_world", "q_pos", "q_after", "defer", "runs")


def rec(u, world="world", position=(1.0, 2.0, 3.0), data="d", flex=b"\x01"):
    return dict(uuid=uuid.UUID(int=u) if isinstance(u, int) else u, world_name=world, position=position, data=data, flex=flex)


def ev(ins, world="world", position=None, parameter=None, records=None, sender=0):
    return dict(instruction=ins, world_name=world, position=position, parameter=parameter, records=records or [],
                sender_uuid=PEERS[sender])


def wire(events):
    """The events' frames as codec.serialize_messages writes them."""
    return codec.serialize_messages([dict(e, instruction=INS[e["instruction"]], records=e["records"]) for e in events])


def processor_events(events):
    """The events as records.RecordProcessor takes them."""
    return [dict(e, records=[dict(r, uuid=(r["uuid"].int >> 64, r["uuid"].int & (2**64 - 1))) for r in e["records"]])
            for e in events]


class Case:
    """One input of the call: frames, the decoder's arrays, the database list and the call's arguments."""

    def __init__(self, events=None, frames=None, db_src="db", worlds=WORLDS, **kw):
        self.events = events
        self.data, self.offsets = wire(events) if frames is None else codec.pack_frames(frames)
        self.data = np.array(self.data, copy=True)
        self.worlds = worlds
        self.decoded = ingest.decode_frames_np(self.data, self.offsets, worlds, PEERS)
        if db_src == "db":   # the dispatch's database list
            d = ingest.dispatch_np(self.decoded)
            sb = d["counters"]["side_begin"]
            db_src = d["side_src"][sb[2]:sb[3]].copy()
        self.db_src = None if db_src is None else np.asarray(db_src, np.uint32)
        self.n_db = len(self.offsets) - 1 if self.db_src is None else len(self.db_src)
        self.kw = dict(now_us=NOW, free_handles=None, handle_next=0)
        self.kw.update(kw)

    def definition(self, **over):
        return ingest.records_dispatch_np(self.data, self.offsets, self.decoded, self.db_src, SIZES, self.worlds,
                                          **dict(self.kw, **over))


def same(got, want, what="", fields=ARRAYS, counters=True):
    for k in fields:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k, g, w)
    if counters:
        assert got["counters"] == want["counters"], (what, got["counters"], want["counters"])


# ---- the definition against RecordProcessor ---------------------------------------------------------------

class RecordingStore:
    """A store that records what it is asked: RecordProcessor's calls, in order."""
    sizes = SIZES

    def __init__(self):
        self.calls = []

    def apply(self, ops):
        self.calls.append(("apply", np.array(ops, copy=True)))
        return {"created": 0, "deleted_rows": 0, "rejected": 0, "rows_live": 0}

    def read(self, world, pos, after, dedupe=False, capacity=0):
        if not dedupe:   # the sizing call; the answering call repeats it
            self.calls.append(("read", list(world), np.array(pos, np.float64).reshape(-1, 3).tobytes(), list(after)))   # bits: NaNs
        return {"offsets": np.zeros(len(world) + 1, np.uint32), "handles": np.zeros(0, np.uint32), "returned": 0}

    def drain_dead(self):
        return np.zeros(0, np.uint32)


def processor_calls(events, free=(), slab_len=0):
    """(the calls a RecordProcessor issues for the events, the free handles in the order it pops them, the
    handle a create gets once they are used up)."""
    store = RecordingStore()
    ids = WorldIds()
    for w in WORLDS:
        ids.intern(w)
    p = records.RecordProcessor(store, ids)
    p.slab, p.free = [None] * slab_len, list(free)
    p.process(processor_events(events), NOW)
    return store.calls, list(reversed(free)), slab_len


def definition_calls(d):
    """The definition's runs as RecordProcessor's calls."""
    out = []
    for a, b in zip(d["runs"][:-1], d["runs"][1:]):
        if a["kind"] == abi.RRUN_APPLY:
            out.append(("apply", d["ops"][int(a["op_begin"]):int(b["op_begin"])]))
        else:
            lo, hi = int(a["q_begin"]), int(b["q_begin"])
            out.append(("read", d["q_world"][lo:hi].tolist(), d["q_pos"][lo:hi].tobytes(), d["q_after"][lo:hi].tolist()))
    return out


def check_against_processor(events, free=(), slab_len=0, what=""):
    calls, free_order, nxt = processor_calls(events, free, slab_len)
    d = Case(events, free_handles=free_order, handle_next=nxt).definition()
    got = definition_calls(d)
    assert d["counters"]["error"] == 0 and d["counters"]["overflow"] == 0
    assert len(got) == len(calls) == d["counters"]["n_runs"], (what, len(got), len(calls))
    for k, (g, w) in enumerate(zip(got, calls)):
        assert g[0] == w[0], (what, k)
        if g[0] == "apply":
            assert g[1].tobytes() == w[1].tobytes(), (what, k, g[1], w[1])
        else:
            assert g[1:] == w[1:], (what, k, g, w)
    return d


def random_events(n, seed, p_record=0.4, max_records=6, unknown=False, raw_names=None):
    """n events, about p_record of them record instructions with 0 - max_records records a frame: creates,
    deletes and reads over a few regions and a small pool of uuids, with every drop rule sprinkled in."""
    r = random.Random(seed)
    names = list(raw_names or RAW_NAMES) + (UNKNOWN if unknown else [])

    def position():
        k = r.random()
        if k < 0.06:
            return None
        if k < 0.09:
            return (float("nan"), 1.0, 2.0)
        if k < 0.12:
            return (1e12, 0.0, 0.0)          # region index past 2^23
        return (r.choice([-40.0, -0.5, 0.0, 3.5, 17.0, 100.25]), r.choice([0.0, 8.0, -20.0]), r.choice([1.0, 33.0]))

    def world():
        return r.choice(REFUSED) if r.random() < 0.08 else r.choice(names)

    out = []
    for _ in range(n):
        if r.random() >= p_record:
            out.append(ev(r.choice(["LocalMessage", "Heartbeat", "RecordUpdate"]), world(), position()))
            continue
        ins = r.choice(["RecordCreate", "RecordCreate", "RecordDelete", "RecordRead", "RecordRead"])
        if ins == "RecordRead":
            param = r.choice([None, None, None, "0", "+5", "05", "abc", "", str(NOW // 1000 - 5), str(NOW // 1000 + 10**6)])
            out.append(ev(ins, world(), position(), param, sender=r.randrange(8)))
        else:
            recs = [rec(r.randrange(1, 40), world(), position(), r.choice([None, "", "payload-%d" % r.randrange(99)]),
                        r.choice([None, b"", bytes([r.randrange(256)]) * r.randrange(1, 9)]))
                    for _ in range(r.randrange(max_records + 1))]
            out.append(ev(ins, world(), position(), records=recs, sender=r.randrange(8)))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_random_events_equal_the_processor_call_by_call(seed):
    events = random_events(300, seed)
    d = check_against_processor(events, free=(7, 3, 11, 2), slab_len=12, what=f"seed {seed}")
    c = d["counters"]
    assert c["n_creates"] > 4 and c["n_deletes"] > 0 and c["n_read"] > 0 and c["n_runs"] > 10
    assert c["n_drop_no_position"] and c["n_drop_world"] and c["n_drop_unpackable"] and c["n_read_dropped"]
    assert c["n_deferred_records"] == c["n_read_deferred"] == 0 and c["first_deferred"] == len(events)
    creates = d["ops"][d["ops"]["kind"] == records.CREATE]
    assert creates["handle"][:4].tolist() == [2, 11, 3, 7] and creates["handle"][4] == 12   # the free list, then the slab's end


# ---- named cases ------------------------------------------------------------------------------------------

P = (1.0, 2.0, 3.0)
READ_PARAMS = {"+5": 5000, "05": 5000, "": None, "+": None, "-1": None, "1 ": None, str(2**64 - 1): None,
               "8210298412799999": 8210298412799999000, "8210298412800000": None, "0" * 4096 + "7": 7000,
               "++5": None, "18446744073709551616": None, "0": 0}


@functools.lru_cache(maxsize=None)
def named():
    """name -> Case. Every case's events are also RecordProcessor's, unless the case says otherwise."""
    c = {}
    c["drop_rules"] = Case([ev("RecordCreate", records=[rec(1), rec(2, position=None), rec(3, world="0bad"), rec(4, world=""),
                                                           rec(5, world="x" * 70), rec(6, position=(1e12, 0.0, 0.0)),
                                                           rec(7, position=(0.0, float("nan"), 0.0)), rec(8, world="@global"),
                                                           rec(9, world="café"), rec(10, world="chat/server_1")]),
                            ev("RecordDelete", records=[rec(1), rec(2, position=None), rec(11, world="a b")]),
                            ev("RecordRead"), ev("RecordRead", position=P, parameter="nope"),
                            ev("RecordRead", world="0bad", position=P), ev("RecordRead", position=P)])
    c["global_message_and_record"] = Case([ev("RecordCreate", "@global", records=[rec(1)]), ev("RecordRead", "@global", position=P),
                                           ev("RecordDelete", "@global", records=[rec(1)]),
                                           ev("RecordCreate", "arena", records=[rec(2, world="@global"), rec(3)])])
    u = uuid.UUID(int=0x67e5504410b1426f9247bb680e5fe0c8)
    c["uuid_forms"] = Case(frames=[message(instruction=8, sender_uuid=str(PEERS[0]), world_name="world",
                                           records=[dict(uuid=form, world_name="world", position=P, data="x", flex=None)
                                                    for form in (str(u), u.hex, "urn:uuid:" + str(u), str(u).upper())])])
    c["empty_create_between_reads"] = Case([ev("RecordRead", position=P), ev("RecordRead", "w00", position=P),
                                            ev("RecordCreate", records=[]), ev("RecordRead", position=P)])
    c["dropped_create_between_reads"] = Case([ev("RecordRead", position=P), ev("RecordCreate", records=[rec(1, position=None)]),
                                              ev("RecordRead", position=P)])
    c["dropped_read_between_creates"] = Case([ev("RecordCreate", records=[rec(1)]), ev("RecordRead"),
                                              ev("RecordCreate", records=[rec(2)]), ev("RecordDelete", records=[rec(1)])])
    c["parameters"] = Case([ev("RecordRead", position=P, parameter=p) for p in READ_PARAMS])
    c["nan_and_unpackable"] = Case([ev("RecordCreate", records=[rec(1, position=(float("nan"),) * 3), rec(2, position=(-1e12, 0.0, 0.0)),
                                                                  rec(3, position=(float("inf"), 0.0, 0.0)),
                                                                  rec(4, position=(-0.0, 134217727.0, -134217712.0)),
                                                                  rec(5, position=(0.0, 134217728.0, 0.0))]),
                                    ev("RecordRead", position=(float("nan"), 0.0, 0.0)), ev("RecordRead", position=(1e300, 0.0, 0.0))])
    c["unknown_world_on_a_record"] = Case([ev("RecordCreate", records=[rec(1), rec(2, world="elsewhere"), rec(3)]),
                                           ev("RecordRead", position=P),
                                           ev("RecordDelete", records=[rec(4, world="nowhere")])])
    c["unknown_world_on_a_read"] = Case([ev("RecordRead", position=P), ev("RecordRead", "elsewhere", position=P),
                                         ev("RecordCreate", records=[rec(1)]), ev("RecordRead", "nowhere", position=P, parameter="5")])
    c["no_table"] = Case([ev("RecordCreate", records=[rec(1)]), ev("RecordRead", position=P)], worlds=[])
    c["other_instructions_in_the_list"] = Case([ev("LocalMessage", position=P), ev("RecordCreate", records=[rec(1)]),
                                                ev("RecordUpdate", records=[rec(2)]), ev("Heartbeat"), ev("RecordRead", position=P)],
                                               db_src=None)
    return c


EXACT = ("drop_rules", "global_message_and_record", "empty_create_between_reads", "dropped_create_between_reads",
         "dropped_read_between_creates", "parameters", "nan_and_unpackable", "other_instructions_in_the_list")


@pytest.mark.parametrize("name", EXACT)
def test_named_case_equals_the_processor(name):
    check_against_processor(named()[name].events, what=name)


def kinds(d):
    return d["runs"]["kind"].tolist()


def test_drop_rules():
    d = named()["drop_rules"].definition()
    c = d["counters"]
    assert (c["n_creates"], c["n_deletes"]) == (2, 2) and d["ops"]["uuid_lo"].tolist() == [1, 10, 1, 11]
    assert d["ops"]["world"].tolist() == [0, 2, 0, 3] and d["ops"]["handle"].tolist() == [0, 1, 0, 0]
    assert (c["n_drop_no_position"], c["n_drop_world"], c["n_drop_unpackable"], c["n_drop_walk"]) == (2, 5, 2, 0)
    assert d["cls"].tolist() == [abi.RCLS_APPLY] * 2 + [abi.RCLS_READ_DROPPED] * 3 + [abi.RCLS_READ]
    assert kinds(d) == [abi.RRUN_APPLY, abi.RRUN_READ, abi.RRUN_END]
    assert d["op_ref"]["record"].tolist() == [0, 9, 0, 2] and d["op_ref"]["bits"].tolist() == [3] * 4
    case = named()["drop_rules"]
    f0 = case.data[int(case.offsets[0]):int(case.offsets[1])].tobytes()
    ref = d["op_ref"][1]
    assert f0[ref["data_off"]:ref["data_off"] + ref["data_len"]] == b"d" and f0[ref["flex_off"]:ref["flex_off"] + ref["flex_len"]] == b"\x01"


def test_global_on_the_message_and_on_a_record():
    d = named()["global_message_and_record"].definition()
    assert d["cls"].tolist() == [abi.RCLS_SKIP] * 3 + [abi.RCLS_APPLY]
    assert d["counters"]["n_drop_world"] == 1 and d["ops"]["uuid_lo"].tolist() == [3] and d["ops"]["world"].tolist() == [0]


def test_the_three_uuid_text_forms():
    d = named()["uuid_forms"].definition()
    assert d["counters"]["n_creates"] == 4 and d["counters"]["error"] == 0
    assert set(d["ops"]["uuid_hi"].tolist()) == {0x67e5504410b1426f} and set(d["ops"]["uuid_lo"].tolist()) == {0x9247bb680e5fe0c8}


def test_runs_split_at_barriers_that_yield_nothing():
    d = named()["empty_create_between_reads"].definition()
    assert kinds(d) == [abi.RRUN_READ, abi.RRUN_READ, abi.RRUN_END] and d["runs"]["q_begin"].tolist() == [0, 2, 3]
    assert d["runs"]["first_frame"].tolist() == [0, 3, 4]
    d = named()["dropped_create_between_reads"].definition()
    assert kinds(d) == [abi.RRUN_READ, abi.RRUN_READ, abi.RRUN_END]
    d = named()["dropped_read_between_creates"].definition()
    assert kinds(d) == [abi.RRUN_APPLY, abi.RRUN_APPLY, abi.RRUN_END] and d["runs"]["op_begin"].tolist() == [0, 1, 3]


def test_parameters():
    d = named()["parameters"].definition()
    want = [v for v in READ_PARAMS.values() if v is not None]
    assert d["q_after"].tolist() == want and d["counters"]["n_read_dropped"] == len(READ_PARAMS) - len(want)
    assert d["cls"].tolist() == [abi.RCLS_READ if v is not None else abi.RCLS_READ_DROPPED for v in READ_PARAMS.values()]
    for text, v in READ_PARAMS.items():
        assert ingest.parse_after(text.encode()) == v
        if len(text) < 4000:
            assert records.parse_epoch_millis(text) == v
    assert Case([ev("RecordRead", position=P)]).definition()["q_after"].tolist() == [ingest.NO_AFTER]


def test_nan_and_unpackable_positions():
    d = named()["nan_and_unpackable"].definition()
    assert d["counters"]["n_drop_unpackable"] == 4 and d["ops"]["uuid_lo"].tolist() == [4]
    assert d["ops"]["pos"].view(np.uint64)[0, 0] == 1 << 63                    # -0.0: the bits as they lie
    assert d["counters"]["n_read"] == 2 and np.isnan(d["q_pos"][0, 0])         # a read is the store's to reject


def test_unknown_worlds_are_deferred():
    d = named()["unknown_world_on_a_record"].definition()
    c = d["counters"]
    assert d["defer"].tolist() == [(0, 1), (2, 0)] and c["n_deferred_records"] == 2 and c["first_deferred"] == 0
    assert d["ops"]["uuid_lo"].tolist() == [1, 3] and kinds(d) == [abi.RRUN_APPLY, abi.RRUN_READ, abi.RRUN_END]
    d = named()["unknown_world_on_a_read"].definition()
    assert d["defer"].tolist() == [(1, abi.RDEFER_READ), (3, abi.RDEFER_READ)] and d["counters"]["first_deferred"] == 1
    assert d["cls"].tolist() == [abi.RCLS_READ, abi.RCLS_READ_DEFERRED, abi.RCLS_APPLY, abi.RCLS_READ_DEFERRED]
    assert kinds(d) == [abi.RRUN_READ, abi.RRUN_APPLY, abi.RRUN_END] and d["counters"]["n_read_deferred"] == 2
    d = named()["no_table"].definition()
    assert d["defer"].tolist() == [(0, 0), (1, abi.RDEFER_READ)] and d["counters"]["n_runs"] == 0


def test_capacities_cut_rows_and_keep_the_counters():
    case = Case(random_events(200, 9, p_record=0.7, unknown=True))
    full = case.definition()
    c = full["counters"]
    assert c["n_deferred_records"] > 3 and c["n_read_deferred"] > 0 and len(full["ops"]) > 20
    cut = case.definition(ops_capacity=7, defer_capacity=1, runs_capacity=3)
    assert cut["counters"] == dict(c, overflow=abi.RECDISP_OVERFLOW_OPS | abi.RECDISP_OVERFLOW_DEFER | abi.RECDISP_OVERFLOW_RUNS)
    assert cut["ops"].tobytes() == full["ops"][:7].tobytes() and cut["op_ref"].tobytes() == full["op_ref"][:7].tobytes()
    assert cut["defer"].tobytes() == full["defer"][:1].tobytes() and cut["runs"].tobytes() == full["runs"][:3].tobytes()
    sizing = case.definition(ops_capacity=0, defer_capacity=0, runs_capacity=0)
    assert len(sizing["ops"]) == len(sizing["runs"]) == 0 and sizing["counters"]["n_creates"] == c["n_creates"]
    total = c["n_records_total"]
    few = case.definition(max_records=total // 2)
    assert few["counters"]["overflow"] == abi.RECDISP_OVERFLOW_RECORDS and few["counters"]["n_records"] == total // 2
    assert few["counters"]["n_records_total"] == total and len(few["ops"]) < len(full["ops"])
    assert case.definition(max_records=total)["counters"] == c


def test_deferred_list_is_ascending_and_first_deferred_is_its_head():
    d = Case(random_events(300, 4, unknown=True)).definition()
    pairs = d["defer"].tolist()
    assert pairs == sorted(pairs) and len(pairs) > 5 and d["counters"]["first_deferred"] == pairs[0][0]


# ---- hostile inputs: the definition never reads outside a frame ------------------------------------------------

def hostile():
    """name -> Case whose arrays disagree with its frames."""
    out = {}
    base = [ev("RecordCreate", records=[rec(k) for k in range(1, 6)]), ev("RecordRead", position=P, parameter="12"),
            ev("RecordDelete", records=[rec(2), rec(3)]), ev("RecordRead", "w00", position=P)]
    good = Case(base)
    # msg says OK on a frame cut short: the offsets of a tick whose first frame lost its tail
    cut = Case(base)
    off = cut.offsets.copy()
    keep = _records_vector(bytes(cut.data[:int(off[1])]))[0] + 8     # inside the records vector
    lost = int(off[1]) - keep
    cut.data = np.concatenate([cut.data[:keep], cut.data[int(off[1]):]])
    off[1:] -= lost
    cut.offsets = off
    out["ok_on_a_truncated_frame"] = cut
    wrong = Case(base)
    wrong.decoded["msg"]["n_records"] = [99, 7, 0, 1]
    out["n_records_wrong"] = wrong
    for name, src in (("db_src_out_of_range", [0, 1, 4, 0xFFFFFFFF, 2]), ("db_src_descending", [3, 2, 1, 0]),
                      ("db_src_repeats", [0, 0, 2, 2])):
        out[name] = Case(base, db_src=src)
    past = Case(base)
    b = past.data
    f0 = bytes(b[:int(past.offsets[1])])
    vec, count = _records_vector(f0)
    struct.pack_into("<I", b, vec + 4, 0x7FFFFFF0)          # record 1's offset points far past the frame
    struct.pack_into("<I", b, vec + 8, int(past.offsets[1]) - vec - 8 - 2)   # record 2's lands unaligned on the frame's end
    out["record_offsets_past_the_frame"] = past
    flags = Case(base)
    flags.decoded["flags"][:] = [abi.INGEST_OK, abi.INGEST_OK | abi.INGEST_HAS_POSITION | abi.INGEST_HAS_PARAMETER | abi.INGEST_WORLD_KNOWN,
                                 abi.INGEST_OK | abi.INGEST_WORLD_GLOBAL, 0xFF]
    flags.decoded["msg"]["param_off"][1] = 0xFFFFFFF0
    flags.decoded["world"][:] = [5, 5, 5, abi.WORLD_GLOBAL]
    out["flags_and_ranges_that_disagree"] = flags
    bad_off = Case(base)
    o = bad_off.offsets.copy()
    o[2] = o[1] - 4
    bad_off.offsets = o
    out["frame_offsets_descend"] = bad_off
    assert good.definition()["counters"]["error"] == 0
    return out


def _records_vector(frame: bytes):
    rd = ingest._Reader(frame)
    fp = rd.field(rd.visit_table(rd.follow(0)), 14)
    return rd.vec_range(rd.follow(fp), 4)


@pytest.mark.parametrize("name", sorted(hostile()))
def test_hostile_input_yields_error_bits_and_no_exception(name):
    d = hostile()[name].definition()
    c = d["counters"]
    want = {"ok_on_a_truncated_frame": abi.RECDISP_ERROR_WALK, "n_records_wrong": 0,
            "db_src_out_of_range": abi.RECDISP_ERROR_LIST, "db_src_descending": abi.RECDISP_ERROR_LIST,
            "db_src_repeats": abi.RECDISP_ERROR_LIST, "record_offsets_past_the_frame": abi.RECDISP_ERROR_WALK,
            "flags_and_ranges_that_disagree": abi.RECDISP_ERROR_WALK, "frame_offsets_descend": abi.RECDISP_ERROR_WALK}[name]
    assert c["error"] == want, (name, c)
    if name == "n_records_wrong":
        assert c["n_records_total"] == 7 and c["n_creates"] == 5 and c["n_deletes"] == 2
    if name == "record_offsets_past_the_frame":
        assert c["n_drop_walk"] == 2 and c["n_creates"] == 3
    if name == "db_src_out_of_range":
        assert d["cls"].tolist() == [abi.RCLS_APPLY, abi.RCLS_READ, abi.RCLS_SKIP, abi.RCLS_SKIP, abi.RCLS_APPLY]
