"""CPU: the ingest dispatch's definition (worldql_server_amd/ingest.py dispatch_np) and the shared case list
of the mirror (tests/test_ingest_dispatch_cpp_mirror.py) and GPU (tests/test_gpu_ingest_dispatch.py) tests.

  - one hand-written frame per row of the class table of include/wq_router.h, every drop rule on its own,
    and the flag / value disagreements;
  - the run table with no effective frame, one run, alternation at every frame and a runs_capacity of 0, 1
    and n_runs; the sum identity of the counters;
  - the ordering proof: tests/seq_reference.random_events streams serialized by the host serializer,
    decoded by decode_frames_np, dispatched by dispatch_np and executed run by run on the C oracle equal
    the reference's sequential loop event by event (as sets of uuids), in ticks of 1, 2, 5, 97 and 400
    events; with unregistered joiners every tick is exact before first_deferred, and dispatching the
    suffix again after the join is exact for the rest."""
import functools
import uuid

import numpy as np
import pytest

from oracle import oracle as orc
from worldql_server_amd import abi, codec, ingest
from worldql_server_amd.processing import (AREA_SUBSCRIBE, AREA_UNSUBSCRIBE, DISCONNECT, GLOBAL_MESSAGE, LOCAL_MESSAGE,
                                           PeerMapBroadcast)
from worldql_server_amd.world_names import GLOBAL_WORLD, SanitizeError, sanitize_world_name

from tests.seq_reference import WORLD_NAMES, SequentialReference, random_events

OK, POS, ATG, WK, SK = (abi.INGEST_OK, abi.INGEST_HAS_POSITION, abi.INGEST_WORLD_GLOBAL, abi.INGEST_WORLD_KNOWN,
                        abi.INGEST_SENDER_KNOWN)
FULL = OK | POS | WK | SK           # a decoded frame with a position, a known world and a known sender
NO_PEER, W_GLOBAL, W_INVALID = abi.INGEST_NO_PEER, abi.WORLD_GLOBAL, abi.WORLD_INVALID
HB, SUB, UNSUB, GLOBAL, LOCAL = 0, 4, 5, 6, 7
ARRAYS = ingest.DISPATCH_ROWS + ("runs",)


def decoded(rows):
    """The decode's arrays from (instruction, flags, world, sender[, repl[, pos]]) tuples."""
    n = len(rows)
    d = dict(instruction=np.zeros(n, np.uint8), flags=np.zeros(n, np.uint8), world=np.zeros(n, np.uint32),
             sender=np.zeros(n, np.uint32), repl=np.zeros(n, np.uint8), pos=np.zeros((n, 3), np.float64))
    for i, r in enumerate(rows):
        d["instruction"][i], d["flags"][i], d["world"][i], d["sender"][i] = r[:4]
        d["repl"][i] = r[4] if len(r) > 4 else i % 3
        d["pos"][i] = r[5] if len(r) > 5 else (i + 0.5, -2.0 * i, 1e-3 * i)
    return d


def at_global(ins, flags=OK | POS | ATG | SK, sender=3):
    return (ins, flags, W_GLOBAL, sender)


# (name, row, the class it must get): one per row of the table, then every drop rule on its own
CLASS_ROWS = [
    ("bad", (LOCAL, FULL & ~OK, 1, 2), abi.CLS_BAD),
    ("bad_zeroed", (0, 0, W_INVALID, NO_PEER), abi.CLS_BAD),
    ("heartbeat", (HB, OK | SK | WK, 0, 4), abi.CLS_HEARTBEAT),
    ("heartbeat_unknown_sender", (HB, OK, W_INVALID, NO_PEER), abi.CLS_HEARTBEAT),
    ("local", (LOCAL, FULL, 2, 5), abi.CLS_LOCAL),
    ("local_unknown_sender", (LOCAL, FULL & ~SK, 2, NO_PEER), abi.CLS_LOCAL),
    ("global", (GLOBAL, OK | WK | SK, 1, 6), abi.CLS_GLOBAL),
    ("global_with_position_unknown_sender", (GLOBAL, OK | POS | WK, 1, NO_PEER), abi.CLS_GLOBAL),
    ("bcast", at_global(GLOBAL), abi.CLS_BCAST),
    ("bcast_no_position", at_global(GLOBAL, OK | ATG, NO_PEER), abi.CLS_BCAST),
    ("subscribe", (SUB, FULL, 0, 7), abi.CLS_OP),
    ("unsubscribe", (UNSUB, FULL, 3, 8), abi.CLS_OP),
    ("join_unknown_sender", (SUB, FULL & ~SK, 0, NO_PEER), abi.CLS_DEFERRED),
    ("join_unknown_world", (SUB, FULL & ~WK, W_INVALID, 7), abi.CLS_DEFERRED),
    ("join_both", (SUB, OK | POS, W_INVALID, NO_PEER), abi.CLS_DEFERRED),
    ("record_create", (8, FULL, 0, 1), abi.CLS_DB),
    ("record_read", (9, OK, W_INVALID, NO_PEER), abi.CLS_DB),
    ("record_delete", (11, at_global(11)[1], W_GLOBAL, 3), abi.CLS_DB),
    ("handshake", (1, FULL, 0, 1), abi.CLS_OTHER),
    ("peer_connect", (2, FULL, 0, 1), abi.CLS_OTHER),
    ("peer_disconnect", (3, FULL, 0, 1), abi.CLS_OTHER),
    ("record_update", (10, FULL, 0, 1), abi.CLS_OTHER),
    ("record_reply", (12, FULL, 0, 1), abi.CLS_OTHER),
    ("unknown", (255, FULL, 0, 1), abi.CLS_OTHER),
    ("any_other_byte", (77, FULL, 0, 1), abi.CLS_OTHER),
    ("drop_local_at_global", at_global(LOCAL), abi.CLS_DROPPED),
    ("drop_subscribe_at_global", at_global(SUB), abi.CLS_DROPPED),
    ("drop_unsubscribe_at_global", at_global(UNSUB), abi.CLS_DROPPED),
    ("drop_local_no_position", (LOCAL, FULL & ~POS, 2, 5), abi.CLS_DROPPED),
    ("drop_subscribe_no_position", (SUB, FULL & ~POS, 2, 5), abi.CLS_DROPPED),
    ("drop_subscribe_no_position_unknown_sender", (SUB, OK | WK, 2, NO_PEER), abi.CLS_DROPPED),
    ("drop_unsubscribe_no_position", (UNSUB, FULL & ~POS, 2, 5), abi.CLS_DROPPED),
    ("drop_local_unknown_world", (LOCAL, FULL & ~WK, W_INVALID, 5), abi.CLS_DROPPED),
    ("drop_global_unknown_world", (GLOBAL, OK | SK, W_INVALID, 5), abi.CLS_DROPPED),
    ("drop_unsubscribe_unknown_world", (UNSUB, FULL & ~WK, W_INVALID, 5), abi.CLS_DROPPED),
    ("drop_unsubscribe_unknown_sender", (UNSUB, FULL & ~SK, 2, NO_PEER), abi.CLS_DROPPED),
]

# (name, row, the class): a flag and its value disagree, so error bit 0 and what disagrees is unresolved
DISAGREE_ROWS = [
    ("world_flag_without_value", (LOCAL, FULL, W_INVALID, 5), abi.CLS_DROPPED),
    ("world_flag_with_global_value", (SUB, FULL, W_GLOBAL, 5), abi.CLS_DEFERRED),
    ("world_value_without_flag", (LOCAL, FULL & ~WK, 2, 5), abi.CLS_DROPPED),
    ("global_value_without_flag", (GLOBAL, OK | SK, W_GLOBAL, 5), abi.CLS_DROPPED),
    ("global_flag_without_value", (GLOBAL, OK | ATG | SK, 2, 5), abi.CLS_BCAST),
    ("global_flag_and_world_flag", (LOCAL, FULL | ATG, 2, 5), abi.CLS_DROPPED),
    ("sender_flag_without_value_subscribe", (SUB, FULL, 1, NO_PEER), abi.CLS_DEFERRED),
    ("sender_flag_without_value_unsubscribe", (UNSUB, FULL, 1, NO_PEER), abi.CLS_DROPPED),
    ("sender_value_without_flag_subscribe", (SUB, FULL & ~SK, 1, 9), abi.CLS_DEFERRED),
    ("sender_value_without_flag_local", (LOCAL, FULL & ~SK, 1, 9), abi.CLS_LOCAL),   # the row carries NO_PEER
    ("sender_value_without_flag_heartbeat", (HB, OK, 0, 2), abi.CLS_HEARTBEAT),     # and is not stamped
]

INS_MIX = np.array([HB, 1, 2, 3, SUB, UNSUB, GLOBAL, LOCAL, 8, 9, 10, 11, 12, 255, 77], np.uint8)
INS_P = np.array([4, 1, 1, 1, 12, 8, 10, 40, 3, 3, 1, 2, 1, 1, 1], np.float64)


def random_decoded(n, seed, hostile=False, p_effective=None):
    """n frames as the decoder leaves them: instructions of every code, worlds resolved, "@global" or
    unknown, senders known or not, positions present or not, some frames that did not decode. hostile:
    flags and values drawn independently, so most frames disagree."""
    rng = np.random.default_rng(seed)
    ins = rng.choice(INS_MIX, size=n, p=INS_P / INS_P.sum())
    if p_effective is not None:     # mostly frames that take no part in the runs
        ins = np.where(rng.random(n) < p_effective, ins, HB).astype(np.uint8)
    kind_w = rng.choice(3, size=n, p=[0.85, 0.07, 0.08])                 # resolved, "@global", unknown
    world = np.where(kind_w == 0, rng.integers(0, 5, n), np.where(kind_w == 1, W_GLOBAL, W_INVALID)).astype(np.uint32)
    known = rng.random(n) < 0.9
    sender = np.where(known, rng.integers(0, 50, n), NO_PEER).astype(np.uint32)
    flags = (OK | np.where(rng.random(n) < 0.93, POS, 0) | np.where(kind_w == 0, WK, 0) | np.where(kind_w == 1, ATG, 0) |
             np.where(known, SK, 0) | rng.choice([0, 4, 8, 12], size=n)).astype(np.uint8)
    bad = rng.random(n) < 0.03
    flags[bad], world[bad], sender[bad], ins[bad] = 0, W_INVALID, NO_PEER, 0
    if hostile:
        flags = rng.integers(0, 256, n).astype(np.uint8)
        world = rng.choice(np.array([0, 1, 4, W_GLOBAL, W_INVALID, 0xFFFFFFFD], np.uint32), size=n)
        sender = rng.choice(np.array([0, 1, 49, 50, 63, NO_PEER, 0xFFFFFFFE], np.uint32), size=n)
    pos = rng.uniform(-100, 100, (n, 3))
    pos[rng.random(n) < 0.02] = np.nan
    return dict(instruction=ins, flags=flags, world=world, sender=sender, repl=rng.integers(0, 3, n).astype(np.uint8), pos=pos)


def stretches(spec):
    """Frames from (instruction or "quiet", count) stretches: full LocalMessage / GlobalMessage / subscribe
    frames, "quiet" = heartbeats, database instructions and dropped frames in turn."""
    rows = []
    quiet = [(HB, OK | SK, W_INVALID, 1), (9, FULL, 0, 1), (LOCAL, FULL & ~POS, 0, 1), at_global(GLOBAL)]
    for ins, count in spec:
        for _ in range(count):
            i = len(rows)
            rows.append(quiet[i % 4] if ins == "quiet" else (ins, OK | WK | SK if ins == GLOBAL else FULL, i % 3, i % 40))
    return decoded(rows)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (the decode's arrays, dispatch_np's keyword arguments)."""
    c = {}
    c["classes"] = (decoded([r for _, r, _ in CLASS_ROWS]), dict(last_seen=np.arange(100, 110, dtype=np.uint32), now=77))
    c["disagree"] = (decoded([r for _, r, _ in DISAGREE_ROWS]), dict(last_seen=np.zeros(16, np.uint32), now=5))
    c["empty"] = (decoded([]), {})
    c["empty_no_runs"] = (decoded([]), dict(runs_capacity=0))
    c["no_effective"] = (stretches([("quiet", 70)]), dict(last_seen=np.zeros(3, np.uint32), now=1))
    c["one_run"] = (stretches([(LOCAL, 130)]), {})
    c["one_table_run"] = (stretches([(SUB, 3), (UNSUB, 2)]), {})
    c["alternate"] = (stretches([(LOCAL, 1), (SUB, 1), (GLOBAL, 1), (UNSUB, 1)] * 50), {})
    c["local_global_one_run"] = (stretches([(LOCAL, 2), (GLOBAL, 3), ("quiet", 2), (LOCAL, 1)]), {})
    for cap, name in ((0, "capacity_0"), (1, "capacity_1"), (6, "capacity_n_runs"), (7, "capacity_n_runs_plus_1")):
        c[name] = (stretches([(LOCAL, 10), (SUB, 5), ("quiet", 3)] * 3), dict(runs_capacity=cap))   # 6 runs
    for n in (1, 63, 64, 65, 4097):
        c[f"mix_{n}"] = (random_decoded(n, seed=n), dict(last_seen=np.zeros(40, np.uint32), now=n))
    c["hostile_3000"] = (random_decoded(3000, seed=9, hostile=True), dict(last_seen=np.zeros(64, np.uint32), now=3))
    c["sparse_5000"] = (random_decoded(5000, seed=11, p_effective=0.01), {})
    # run starts on a granule's first lane (frame 64), its last lane (127) and across the boundary (191 | 192)
    c["granule_edges"] = (stretches([(LOCAL, 64), (SUB, 63), (LOCAL, 64), (SUB, 1), (GLOBAL, 70)]), {})
    # granules and whole blocks with no effective frame between two runs of one kind: they must not split it
    c["quiet_granules"] = (stretches([(SUB, 40), ("quiet", 200), (UNSUB, 30), ("quiet", 2100), (SUB, 1), (LOCAL, 5),
                                      ("quiet", 130), (GLOBAL, 3), ("quiet", 1500), (LOCAL, 1), ("quiet", 64), (SUB, 2),
                                      ("quiet", 3000)]), {})
    c["quiet_head"] = (stretches([("quiet", 1100), (LOCAL, 1)]), {})
    # one tick of 65,537 frames with 3 run changes: the scan's shares hold more than one block
    c["big_3_changes"] = (stretches([(LOCAL, 30000), ("quiet", 1), (SUB, 5000), (GLOBAL, 20000), (LOCAL, 536), (UNSUB, 10000)]),
                          dict(last_seen=np.zeros(8, np.uint32), now=2))
    return c


def small_names():
    return [k for k in cases() if k != "big_3_changes"]


@functools.lru_cache(maxsize=None)
def definition(name):
    d, kw = cases()[name]
    return ingest.dispatch_np(d, **kw)


def same(got, want, what="", fields=ARRAYS, counters=True, last_seen=True):
    """Byte for byte: the arrays given, the counters and the stamps."""
    for k in fields:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape[0] == w.shape[0], (what, k, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            gb, wb = g.view(np.uint8).reshape(g.shape[0], -1), w.view(np.uint8).reshape(w.shape[0], -1)
            at = int(np.flatnonzero((gb != wb).any(axis=1))[0])
            raise AssertionError((what, k, "row", at, g[at], w[at]))
    if counters:
        assert got["counters"] == want["counters"], (what, got["counters"], want["counters"])
    if last_seen and want.get("last_seen") is not None:
        assert np.array_equal(got["last_seen"], want["last_seen"]), (what, "last_seen")


# ---- the class table ------------------------------------------------------------------------------

@pytest.mark.parametrize("name,row,cls", CLASS_ROWS, ids=[r[0] for r in CLASS_ROWS])
def test_every_row_of_the_class_table(name, row, cls):
    got = ingest.dispatch_np(decoded([row]))
    assert got["cls"].tolist() == [cls] and got["counters"]["error"] == 0
    assert got["counters"]["n_" + abi.CLS_NAMES[cls]] == 1


@pytest.mark.parametrize("name,row,cls", DISAGREE_ROWS, ids=[r[0] for r in DISAGREE_ROWS])
def test_a_flag_and_a_value_that_disagree(name, row, cls):
    got = ingest.dispatch_np(decoded([row]), last_seen=np.zeros(4, np.uint32), now=9)
    assert got["cls"].tolist() == [cls] and got["counters"]["error"] == abi.DISPATCH_ERROR_DISAGREE
    assert (got["last_seen"] == 0).all()
    if cls == abi.CLS_LOCAL:
        assert got["l_sender"].tolist() == [NO_PEER]
    # a frame that did not decode is not looked at, whatever its values
    assert ingest.dispatch_np(decoded([(row[0], row[1] & ~OK) + row[2:]]))["counters"]["error"] == 0


def test_rows_of_the_hand_written_tick():
    d, kw = cases()["classes"]
    got = definition("classes")
    names = [r[0] for r in CLASS_ROWS]
    at = names.index
    assert got["cls"].tolist() == [r[2] for r in CLASS_ROWS]
    assert got["l_src"].tolist() == [at("local"), at("local_unknown_sender")]
    assert got["l_sender"].tolist() == [5, NO_PEER] and got["l_world"].tolist() == [2, 2]
    assert got["l_pos"].tobytes() == d["pos"][got["l_src"]].tobytes() and got["l_repl"].tolist() == d["repl"][got["l_src"]].tolist()
    assert got["g_src"].tolist() == [at("global"), at("global_with_position_unknown_sender")]
    assert got["g_sender"].tolist() == [6, NO_PEER]
    ops = got["ops"]
    assert got["op_src"].tolist() == [at("subscribe"), at("unsubscribe")]
    assert ops["kind"].tolist() == [abi.OP_SUBSCRIBE, abi.OP_UNSUBSCRIBE] and ops["peer"].tolist() == [7, 8]
    assert ops["world"].tolist() == [0, 3] and (ops["key_is_raw"] == 0).all()
    assert ops["pos"].tobytes() == d["pos"][got["op_src"]].tobytes()
    raw = ops.view(np.uint8).reshape(-1, 40)
    assert (raw[:, 10:16] == 0).all()                      # pad_
    sb = got["counters"]["side_begin"]
    lists = [got["side_src"][sb[k]:sb[k + 1]].tolist() for k in range(5)]
    for k, cls in enumerate(abi.DISPATCH_SIDE_LISTS):
        assert lists[k] == [i for i, r in enumerate(CLASS_ROWS) if r[2] == cls]
    assert got["counters"]["first_deferred"] == at("join_unknown_sender")
    want_seen = kw["last_seen"].copy()
    want_seen[4] = 77                                      # the known heartbeat sender; NO_PEER stamps nothing
    assert got["last_seen"].tolist() == want_seen.tolist()


def test_nan_positions_are_copied_as_bits():
    d = decoded([(LOCAL, FULL, 0, 1), (SUB, FULL, 0, 1)])
    d["pos"][:] = np.array([0x7FF8000000000123, 0xFFF0000000000000, 0x8000000000000000], np.uint64).view(np.float64)
    got = ingest.dispatch_np(d)
    assert got["l_pos"].tobytes() == d["pos"][0].tobytes() and got["ops"]["pos"].tobytes() == d["pos"][1].tobytes()


# ---- the run table and the counters -----------------------------------------------------------------

def runs_of(got):
    return [tuple(int(v) for v in r) for r in got["runs"]]


def test_run_table_shapes():
    assert runs_of(definition("empty")) == [(abi.RUN_END, 0, 0, 0, 0)]
    assert runs_of(definition("empty_no_runs")) == [] and definition("empty_no_runs")["counters"]["overflow"] == 1
    assert runs_of(definition("no_effective")) == [(abi.RUN_END, 70, 0, 0, 0)]
    assert runs_of(definition("one_run")) == [(abi.RUN_READ, 0, 0, 0, 0), (abi.RUN_END, 130, 130, 0, 0)]
    assert runs_of(definition("one_table_run")) == [(abi.RUN_TABLE, 0, 0, 0, 0), (abi.RUN_END, 5, 0, 0, 5)]
    # LocalMessage and GlobalMessage share a read run, and frames without effect do not end it
    assert runs_of(definition("local_global_one_run")) == [(abi.RUN_READ, 0, 0, 0, 0), (abi.RUN_END, 8, 3, 3, 0)]
    alt = definition("alternate")
    assert alt["counters"]["n_runs"] == 200 and [r[1] for r in runs_of(alt)] == list(range(201))
    assert [r[0] for r in runs_of(alt)[:4]] == [abi.RUN_READ, abi.RUN_TABLE, abi.RUN_READ, abi.RUN_TABLE]
    assert runs_of(alt)[5] == (abi.RUN_TABLE, 5, 2, 1, 2)
    q = definition("quiet_granules")
    assert [r[:2] for r in runs_of(q)] == [(abi.RUN_TABLE, 0), (abi.RUN_READ, 2371), (abi.RUN_TABLE, 4074), (abi.RUN_END, 7076)]


def test_runs_capacity():
    full = runs_of(definition("capacity_n_runs_plus_1"))
    assert len(full) == 7 and definition("capacity_n_runs_plus_1")["counters"]["overflow"] == 0
    for cap, name in ((0, "capacity_0"), (1, "capacity_1"), (6, "capacity_n_runs")):
        got = definition(name)
        assert runs_of(got) == full[:cap] and got["counters"]["overflow"] == abi.DISPATCH_OVERFLOW_RUNS
        assert got["counters"]["n_runs"] == 6
        same(got, definition("capacity_n_runs_plus_1"), name, fields=ingest.DISPATCH_ROWS, counters=False)


@pytest.mark.parametrize("name", sorted(cases()))
def test_counters_and_rows_are_consistent(name):
    d, _ = cases()[name]
    got = definition(name)
    c = got["counters"]
    n = len(d["instruction"])
    assert sum(c["n_" + k] for k in abi.CLS_NAMES) == c["n_frames"] == n
    assert np.bincount(got["cls"], minlength=10).tolist() == [c["n_" + k] for k in abi.CLS_NAMES]
    assert (len(got["l_src"]), len(got["g_src"]), len(got["ops"])) == (c["n_local"], c["n_global"], c["n_op"])
    assert c["side_begin"][0] == 0 and c["side_begin"][5] == len(got["side_src"])
    assert np.diff(c["side_begin"]).tolist() == [c["n_" + abi.CLS_NAMES[k]] for k in abi.DISPATCH_SIDE_LISTS]
    for k in ("l_src", "g_src", "op_src"):
        assert (np.diff(got[k].astype(np.int64)) > 0).all()
    # no emitted op carries a reserved world or the no-peer id
    assert (got["ops"]["world"] < W_GLOBAL).all() and (got["ops"]["peer"] != NO_PEER).all()
    # the runs partition the effective frames: every run's rows are the frames between two first frames
    full = ingest.dispatch_np(d)["runs"]
    assert len(full) == c["n_runs"] + 1 and full[-1]["kind"] == abi.RUN_END and full[-1]["first_frame"] == n
    eff = np.sort(np.concatenate([got["l_src"], got["g_src"], got["op_src"]]))
    assert c["n_runs"] <= max(len(eff), 0)
    for a, b in zip(full[:-1], full[1:]):
        assert a["kind"] != b["kind"]
        rows = np.concatenate([got["l_src"][a["l_begin"]:b["l_begin"]], got["g_src"][a["g_begin"]:b["g_begin"]],
                               got["op_src"][a["op_begin"]:b["op_begin"]]])
        assert len(rows) and rows.min() == a["first_frame"] and rows.max() < b["first_frame"]
        if a["kind"] == abi.RUN_TABLE:
            assert a["l_begin"] == b["l_begin"] and a["g_begin"] == b["g_begin"]
        else:
            assert a["op_begin"] == b["op_begin"]


# ---- the ordering proof ---------------------------------------------------------------------------

N_PEERS = 300
INS_CODE = {AREA_SUBSCRIBE: SUB, AREA_UNSUBSCRIBE: UNSUB, GLOBAL_MESSAGE: GLOBAL, LOCAL_MESSAGE: LOCAL}


def peer_uuid(name: str) -> uuid.UUID:
    return uuid.UUID(int=int(name.split("-")[1]) + 1)


def sanitized(name):
    try:
        return None if name == GLOBAL_WORLD else sanitize_world_name(name)
    except SanitizeError:
        return None


def all_worlds():
    """Every world a stream can create, each once."""
    out = []
    for w in WORLD_NAMES:
        s = sanitized(w)
        if s is not None and s not in out:
            out.append(s)
    return out


def stream(n, seed):
    """random_events without the disconnects (they arrive on another channel)."""
    return [e for e in random_events(n, seed, n_peers=N_PEERS) if e.instruction != DISCONNECT]


def wire(events):
    """The events as received frames: (data, offsets) of the host serializer."""
    msgs = [dict(instruction=INS_CODE[e.instruction], sender_uuid=peer_uuid(e.sender_uuid), world_name=e.world_name,
                 position=None if e.position is None else (e.position.x, e.position.y, e.position.z),
                 replication=e.replication) for e in events]
    return codec.serialize_messages(msgs)


class OracleRuns:
    """The caller's side of a dispatched tick with the C oracle as the table: the runs issued in order."""

    def __init__(self, cube_size=16):
        self.o = orc.COracle(cube_size)
        self.calls = []

    def execute(self, disp, n):
        """Per frame the recipients' peer ids (a list), ("bcast", repl) or None."""
        res = [None] * n
        runs = disp["runs"]
        for a, b in zip(runs[:-1], runs[1:]):
            if a["kind"] == abi.RUN_TABLE:
                self.calls.append(("ops", int(b["op_begin"] - a["op_begin"])))
                self.o.apply_ops(disp["ops"][a["op_begin"]:b["op_begin"]])
                continue
            l, g = slice(a["l_begin"], b["l_begin"]), slice(a["g_begin"], b["g_begin"])
            if l.stop > l.start:
                self.calls.append(("route", l.stop - l.start))
                offs, peers, _ = self.o.route(disp["l_pos"][l], disp["l_world"][l], disp["l_sender"][l], disp["l_repl"][l])
                for k, i in enumerate(disp["l_src"][l]):
                    res[int(i)] = peers[offs[k]:offs[k + 1]].tolist()
            if g.stop > g.start:
                self.calls.append(("global", g.stop - g.start))
                offs, peers = self.o.route_global(disp["g_world"][g], disp["g_sender"][g], disp["g_repl"][g])
                for k, i in enumerate(disp["g_src"][g]):
                    res[int(i)] = peers[offs[k]:offs[k + 1]].tolist()
        return res


def check_events(events, dec, disp, got, ref, names_of, upto=None):
    """Event by event against the sequential reference, as sets of uuids. An event the reference answers
    with None (dropped, or a world nobody has subscribed to yet) reaches nobody here, and one it answers
    with nobody may be dropped here (a world the table does not hold yet has no subscribers)."""
    nonempty = 0
    for k, ev in enumerate(events[:upto]):
        want = ref.event(ev)
        if isinstance(want, PeerMapBroadcast):
            assert disp["cls"][k] == abi.CLS_BCAST and int(dec["repl"][k]) == want.replication, (k, ev)
        elif isinstance(want, list):
            assert sorted(names_of(got[k] or [])) == sorted(want), (k, ev, got[k], want)
            nonempty += bool(want)
        else:
            assert not got[k], (k, ev, got[k])
    return nonempty


TICKS = (1, 2, 5, 97, 400)


def ticks_of(events, sizes=TICKS):
    i = t = 0
    while i < len(events):
        yield events[i:i + sizes[t % len(sizes)]]
        i += sizes[t % len(sizes)]
        t += 1


@pytest.mark.parametrize("seed", [7, 21])
def test_dispatched_runs_equal_the_sequential_reference(seed):
    """Every world and peer registered in advance: no join is deferred, so the outcome is the reference's."""
    events = stream(2600, seed)
    worlds = all_worlds()
    peers = [uuid.UUID(int=k + 1) for k in range(N_PEERS)]
    ref, run = SequentialReference(16), OracleRuns(16)
    nonempty = n_runs = 0
    for chunk in ticks_of(events):
        data, offsets = wire(chunk)
        dec = ingest.decode_frames_np(data, offsets, worlds, peers)
        assert dec["counters"]["n_ok"] == len(chunk)
        disp = ingest.dispatch_np(dec)
        # what is deferred here is a subscribe to a name the sanitizer refuses: the host drops it as
        # area_subscribe.rs:23-33 does, and it never had an effect
        sb = disp["counters"]["side_begin"]
        assert all(sanitized(chunk[i].world_name) is None for i in disp["side_src"][sb[4]:sb[5]])
        assert disp["counters"]["error"] == 0
        n_runs += disp["counters"]["n_runs"]
        got = run.execute(disp, len(chunk))
        nonempty += check_events(chunk, dec, disp, got, ref, lambda ids: [f"peer-{p}" for p in ids])
    assert nonempty > 100 and n_runs > 300
    # never more calls than process_tick's batching: one op batch per table run, at most two routes per read run
    assert sum(1 for c in run.calls if c[0] == "ops") <= n_runs


def test_unregistered_joiners_are_exact_before_first_deferred():
    """A third of the peers and all worlds but one unknown at the start. A tick is exact before its first
    deferred event; the host registers the joiner and dispatches the suffix again, which is exact in turn."""
    events = stream(1500, seed=5)
    worlds = ["world"]
    known = list(range(200))
    ref, run = SequentialReference(16), OracleRuns(16)
    joins = nonempty = 0
    for chunk in ticks_of(events, (97, 400, 5)):
        while chunk:
            peers = [uuid.UUID(int=k + 1) for k in known]
            data, offsets = wire(chunk)
            dec = ingest.decode_frames_np(data, offsets, worlds, peers, known)
            disp = ingest.dispatch_np(dec)
            fd = disp["counters"]["first_deferred"]
            if fd < len(chunk):                                      # the prefix alone, then the join
                assert disp["cls"][fd] == abi.CLS_DEFERRED and not (disp["cls"][:fd] == abi.CLS_DEFERRED).any()
                dec = {k: v[:fd] for k, v in dec.items() if k != "counters"}
                disp = ingest.dispatch_np(dec)
                assert disp["counters"]["n_deferred"] == 0
            got = run.execute(disp, min(fd, len(chunk)))
            nonempty += check_events(chunk, dec, disp, got, ref, lambda ids: [f"peer-{p}" for p in ids], upto=fd)
            if fd == len(chunk):
                break
            ev = chunk[fd]
            if sanitized(ev.world_name) is None:                     # a refused name: the host drops the event
                assert ref.event(ev) is None
                chunk = chunk[fd + 1:]
                continue
            pid = int(ev.sender_uuid.split("-")[1])
            if pid not in known:
                known.append(pid)
            if sanitized(ev.world_name) not in worlds:
                worlds.append(sanitized(ev.world_name))
            joins += 1
            chunk = chunk[fd:]
    assert joins > 50 and nonempty > 50 and len(worlds) == len(all_worlds())
