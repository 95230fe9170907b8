"""The frame builder's host definition (worldql_server_amd/frames.py): frame_size_np against the host
serializer's sizes over the whole grid of flat messages, build_frames_np's malformed-input rules each
on a hand-made case, and codec.decode_packed of its output giving every field back. No GPU needed.
The cases here are shared with tests/test_frames_build_cpp_mirror.py and
tests/test_gpu_frames_build.py, which check the kernels' arithmetic and the kernels against them."""
import functools
import itertools
import uuid

import numpy as np
import pytest

from worldql_server_amd import codec, frames

GRID_N = 1960
TILE = 1024
MIB = 1 << 20
# the table: names of length 0..9 and 63 first (world id = length for 0..9), then the usual one
WORLDS = [b"abcdefghi"[:k] for k in range(10)] + [b"w" * 63, b"world", "wörld".encode("utf-8")]
W63, WORLD = 10, 11


class Case:
    """The arguments of build_frames_np / wq_frames_build_device as numpy arrays (None: not given)."""

    def __init__(self, world, instruction=7, replication=0, pos=None, param=None, flex=None, msg_flags=None,
                 worlds=WORLDS, seed=1):
        rng = np.random.default_rng(seed)
        self.worlds = worlds
        self.world = np.asarray(world, dtype=np.uint32)
        self.n = n = len(self.world)
        self.sender_uuid = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        self.instruction, self.replication = instruction, replication
        self.pos = pos
        self.param, self.param_offsets = param if param is not None else (None, None)
        self.flex, self.flex_offsets = flex if flex is not None else (None, None)
        self.msg_flags = msg_flags
        self.n_param_bytes = self.n_flex_bytes = None

    def kw(self):
        return dict(worlds=self.worlds, sender_uuid=self.sender_uuid, world=self.world, instruction=self.instruction,
                    replication=self.replication, pos=self.pos, param=self.param, param_offsets=self.param_offsets,
                    flex=self.flex, flex_offsets=self.flex_offsets, msg_flags=self.msg_flags,
                    n_param_bytes=self.n_param_bytes, n_flex_bytes=self.n_flex_bytes)


def payload(lens, seed, text):
    """Payloads of these lengths packed back to back: (bytes, u64 offsets). text: ASCII letters (a
    parameter is a string), else any byte."""
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(lens, dtype=np.uint64), out=off[1:])
    total = int(off[-1])
    data = rng.integers(97, 123, total, dtype=np.uint8) if text else rng.integers(0, 256, total, dtype=np.uint8)
    return data, off


def positions(n, seed):
    p = np.random.default_rng(seed).uniform(-1e4, 1e4, (n, 3))
    if n > 2:
        p[1, 0] = np.nan
        p[2] = [-0.0, np.inf, 5e-324]
    return p


def grid_fields():
    """The grid: has_position, instruction, replication, world_len, parameter (None, 0..5), flex (None, 0..5)."""
    opt = [None, 0, 1, 2, 3, 4, 5]
    return list(itertools.product((0, 1), (0, 7), (0, 2), range(5), opt, opt))


def grid_case(rows=None, seed=2):
    g = grid_fields()
    if rows is not None:
        g = [g[i] for i in rows]
    flags = np.array([hp | (2 if p is not None else 0) | (4 if f is not None else 0) for hp, _, _, _, p, f in g], np.uint8)
    return Case(world=[wl for _, _, _, wl, _, _ in g], instruction=np.array([i for _, i, _, _, _, _ in g], np.uint8),
                replication=np.array([r for _, _, r, _, _, _ in g], np.uint8), pos=positions(len(g), seed),
                param=payload([p or 0 for *_, p, _ in g], seed + 1, True),
                flex=payload([f or 0 for *_, f in g], seed + 2, False), msg_flags=flags, seed=seed)


def with_big(seed=9):
    """1,000 grid messages with a 1 MiB flex at message 300 and a 1 MiB parameter at message 700."""
    rows = np.random.default_rng(seed).integers(0, GRID_N, 1000)
    c = grid_case(rows, seed)
    pl, fl = np.diff(c.param_offsets).astype(np.int64), np.diff(c.flex_offsets).astype(np.int64)
    c.msg_flags[300] |= 4
    c.msg_flags[700] |= 2
    fl[300], pl[700] = MIB + 3, MIB + 1
    c.param, c.param_offsets = payload(pl, seed + 1, True)
    c.flex, c.flex_offsets = payload(fl, seed + 2, False)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    lens40 = list(range(41))
    edges = [1022, 1023, 1024, 1025, 1026, 4095, 4096, 4097]
    sweep = lens40 + edges
    out = {
        "grid": grid_case(),
        "world_lens": Case(world=list(range(11)) + [WORLD, WORLD + 1], pos=positions(13, 3)),
        "payload_0_40": Case(world=[WORLD] * 41, pos=positions(41, 4), param=payload(lens40, 5, True),
                             flex=payload(lens40[::-1], 6, False)),
        "payload_edges": Case(world=[WORLD] * 8, param=payload(edges, 7, True), flex=payload(edges[::-1], 8, False)),
        # both payloads packed back to back: their starts take every residue mod 16
        "residues": Case(world=[k % 5 for k in range(len(sweep))], pos=positions(len(sweep), 10),
                         param=payload(sweep, 11, True), flex=payload(sweep, 12, False)),
        "param_only": Case(world=[WORLD] * 20, param=payload(list(range(20)), 13, True), instruction=0, replication=255),
        "flex_only": Case(world=[WORLD] * 20, flex=payload(list(range(20)), 14, False), instruction=255),
        "entity_updates": Case(world=[WORLD] * 300, pos=positions(300, 15)),
        "cap_300": Case(world=[WORLD, 3], pos=positions(2, 16), param=payload([0, 9], 17, True),
                        flex=payload([0, 13], 18, False), msg_flags=np.array([1, 7], np.uint8)),
        "empty": Case(world=[]),
        "with_big": with_big(),
    }
    return out


def names():
    return list(cases())


@functools.lru_cache(maxsize=None)
def want(name):
    """The definition's (frames, offsets, sizes, counters) of a case, computed once and shared."""
    got = frames.build_frames_np(**cases()[name].kw())
    for a in got[:3]:
        a.setflags(write=False)
    return got


def nullable_cases():
    """Every combination of the nullable inputs over one small input."""
    n = 7
    base = dict(world=[WORLD, 0, 3, 200, 2, WORLD, 1])
    out = []
    for ins, rep, pos, par, flx, flg in itertools.product((0, 1), repeat=6):
        c = Case(instruction=np.array([0, 7, 255, 3, 0, 1, 7], np.uint8) if ins else 7,
                 replication=np.array([0, 1, 2, 0, 255, 0, 1], np.uint8) if rep else 2,
                 pos=positions(n, 20) if pos else None, param=payload([3, 0, 17, 4, 1, 30, 2], 21, True) if par else None,
                 flex=payload([0, 5, 16, 33, 2, 1, 8], 22, False) if flx else None,
                 msg_flags=np.array([7, 0, 1, 2, 4, 5, 255], np.uint8) if flg else None, **base)
        out.append(((ins, rep, pos, par, flx, flg), c))
    return out


def malformed_cases():
    """name -> (case, the error bits the rules give it)."""
    out = {}
    c = Case(world=[WORLD, len(WORLDS), 0xFFFFFFFF, 2], pos=positions(4, 30))
    out["world_out_of_range"] = (c, frames.ERROR_WORLD)
    c = Case(world=[WORLD] * 4, worlds=None)
    out["no_table"] = (c, frames.ERROR_WORLD)
    c = Case(world=[WORLD] * 5, param=payload([4, 6, 5, 3, 7], 31, True), flex=payload([4, 4, 4, 4, 4], 32, False))
    c.param_offsets = c.param_offsets.copy()
    c.param_offsets[2] = 3          # message 1 descends (10 -> 3), message 2 is [3, 15)
    out["param_descends"] = (c, frames.ERROR_PARAM)
    c = Case(world=[WORLD] * 5, param=payload([4, 6, 5, 3, 7], 31, True), flex=payload([4, 4, 4, 4, 4], 32, False))
    c.flex_offsets = c.flex_offsets.copy()
    c.flex_offsets[5] = 21          # the last message reaches one byte past the end
    out["flex_past_end"] = (c, frames.ERROR_FLEX)
    c = Case(world=[WORLD] * 3, param=payload([2, 2, 2], 33, True), flex=payload([1, 2, 3], 34, False))
    c.param_offsets = np.array([0, 2, (1 << 32) + 2, 6], np.uint64)   # spans 2^32 and past the end, then descends
    c.flex_offsets = np.array([0, 0xFFFFFFFFFFFFFFFF, 3, 6], np.uint64)
    out["both_hostile"] = (c, frames.ERROR_PARAM | frames.ERROR_FLEX)
    # flags that ask for fields whose arrays are not given: the bits count as clear, no error
    c = Case(world=[WORLD, 1, 2], msg_flags=np.array([7, 1, 6], np.uint8), flex=payload([3, 1, 2], 35, False))
    out["flags_without_arrays"] = (c, 0)
    return out


def too_large_case():
    """Offsets that claim payloads around the builder's limit, with no payload memory behind them: for
    the sizing call. Message 1's frame is exactly 2^30 bytes and stands; 0, 2 and 4 are above it."""
    lim = frames.FRAME_MAX
    over = lim - frames.frame_size_np(False, 7, 0, 5, None, 0)   # the largest flex that fits: its frame is 2^30
    assert frames.frame_size_np(False, 7, 0, 5, None, over) == lim and over % 4 == 0
    flens = [over + 1, over, lim, 5, 0]
    plens = [0, 0, 0, 0, lim]
    c = Case(world=[WORLD] * 5)
    c.msg_flags = np.array([4, 4, 4, 4, 2], np.uint8)
    c.flex = np.zeros(0, np.uint8)
    c.param = np.zeros(0, np.uint8)
    c.flex_offsets = np.concatenate([[0], np.cumsum(flens)]).astype(np.uint64)
    c.param_offsets = np.concatenate([[0], np.cumsum(plens)]).astype(np.uint64)
    c.n_flex_bytes, c.n_param_bytes = int(c.flex_offsets[-1]), int(c.param_offsets[-1])
    return c, [0, lim, 0, frames.frame_size_np(False, 7, 0, 5, None, 5), 0]


# ---- the tests ----

def test_frame_size_np_equals_the_serializer_over_the_grid():
    g = grid_fields()
    assert len(g) == GRID_N
    msgs = []
    for k, (hp, ins, rep, wl, p, f) in enumerate(g):
        m = dict(instruction=ins, replication=rep, sender_uuid=uuid.UUID(int=k * 0x9E3779B97F4A7C15 % (1 << 128)),
                 world_name=b"wxyz"[:wl])
        if hp:
            m["position"] = (1.5, -2.0, float(k))
        if p is not None:
            m["parameter"] = b"param"[:p]
        if f is not None:
            m["flex"] = bytes(range(f))
        msgs.append(m)
    data, off = codec.serialize_messages(msgs)
    sizes = np.diff(off).astype(np.int64)
    mine = np.array([frames.frame_size_np(hp, ins, rep, wl, p, f) for hp, ins, rep, wl, p, f in g])
    assert (mine == sizes).all()
    assert sizes.min() == 104 and sizes.max() == 172
    assert frames.frame_size_np(True, 7, 0, 5) == 136          # the usual entity update
    assert (codec.decode_packed(data, off)["status"] == codec.DEC_OK).all()


@pytest.mark.parametrize("name", names())
def test_definition_is_the_serializer_message_by_message(name):
    """build_frames_np on a well-formed case: frame i is serialize_message of message i's fields."""
    c = cases()[name]
    data, off, sizes, cnt = want(name)
    assert cnt == dict(n_frames=c.n, n_complete=c.n, bytes_need=len(data), bytes_written=len(data), overflow=0, error=0)
    assert off[0] == 0 and (np.diff(off) == sizes).all() and int(off[-1]) == len(data)
    flags = c.msg_flags if c.msg_flags is not None else np.full(c.n, 7, np.uint8)
    step = max(1, c.n // 60)
    for i in list(range(0, c.n, step)) + ([300, 700] if name == "with_big" else []):
        m = dict(instruction=int(np.broadcast_to(c.instruction, c.n)[i]), replication=int(np.broadcast_to(c.replication, c.n)[i]),
                 sender_uuid=c.sender_uuid[i].tobytes(), world_name=WORLDS[c.world[i]])
        if c.pos is not None and flags[i] & 1:
            m["position"] = c.pos[i]
        if c.param is not None and flags[i] & 2:
            m["parameter"] = c.param[int(c.param_offsets[i]):int(c.param_offsets[i + 1])].tobytes()
        if c.flex is not None and flags[i] & 4:
            m["flex"] = c.flex[int(c.flex_offsets[i]):int(c.flex_offsets[i + 1])].tobytes()
        assert data[int(off[i]):int(off[i + 1])].tobytes() == codec.serialize_message(m)


def test_the_sweep_takes_every_residue():
    c = cases()["residues"]
    assert set(int(v) % 16 for v in c.param_offsets[:-1]) == set(range(16))
    assert set(int(v) % 16 for v in c.flex_offsets[:-1]) == set(range(16))


def decoded_fields_match(c, data, off, sizes=None):
    """codec.decode_packed of frames: every status OK and every field the case's (under the rules)."""
    d = codec.decode_packed(data, off)
    assert (d["status"] == codec.DEC_OK).all()
    n = c.n
    flags = c.msg_flags if c.msg_flags is not None else np.full(n, 7, np.uint8)
    ins = np.broadcast_to(np.asarray(c.instruction, np.uint8), n)
    rep = np.broadcast_to(np.asarray(c.replication, np.uint8), n)
    assert (d["instruction"] == np.where(ins <= 12, ins, 255)).all()
    assert (d["replication"] == np.where(rep <= 2, rep, 0)).all()
    assert (d["sender_uuid"] == c.sender_uuid).all()
    assert (d["n_records"] == 0).all() and (d["n_entities"] == 0).all()
    has_pos = (flags & 1).astype(bool) if c.pos is not None else np.zeros(n, bool)
    assert (d["has_position"].astype(bool) == has_pos).all()
    if c.pos is not None:
        assert d["position"][has_pos].tobytes() == np.ascontiguousarray(c.pos, np.float64)[has_pos].tobytes()
    has_par = (flags & 2).astype(bool) if c.param is not None else np.zeros(n, bool)
    assert (d["has_parameter"].astype(bool) == has_par).all()
    table = c.worlds or []
    for i in range(0, n, max(1, n // 200)):
        f = data[int(off[i]):int(off[i + 1])]
        w = table[c.world[i]] if c.world[i] < len(table) else b""
        assert f[d["world_off"][i]:d["world_off"][i] + d["world_len"][i]].tobytes() == w
        if has_par[i]:
            a, b = int(c.param_offsets[i]), int(c.param_offsets[i + 1])
            ok = a <= b <= len(c.param) and b - a < 1 << 32
            assert f[d["param_off"][i]:d["param_off"][i] + d["param_len"][i]].tobytes() == (c.param[a:b].tobytes() if ok else b"")


@pytest.mark.parametrize("name", ["grid", "world_lens", "residues", "cap_300", "with_big"])
def test_decode_round_trips_every_field(name):
    data, off, _, _ = want(name)
    decoded_fields_match(cases()[name], data, off)


@pytest.mark.parametrize("name", list(malformed_cases()))
def test_malformed_input_rules(name):
    c, bits = malformed_cases()[name]
    data, off, sizes, cnt = frames.build_frames_np(**c.kw())
    assert cnt["error"] == bits and cnt["n_complete"] == c.n and cnt["overflow"] == 0
    decoded_fields_match(c, data, off)
    d = codec.decode_packed(data, off)
    frame = lambda i: data[int(off[i]):int(off[i + 1])]
    if name == "world_out_of_range":
        assert list(d["world_len"]) == [5, 0, 0, 2]
    if name == "no_table":
        assert (d["world_len"] == 0).all()
    if name == "param_descends":
        assert list(d["param_len"]) == [4, 0, 12, 3, 7] and (d["has_parameter"] == 1).all()
    if name == "flex_past_end":
        # present and empty: the frame of the same message with an empty flex
        assert sizes[4] == frames.frame_size_np(False, 7, 0, 5, 7, 0) and sizes[3] == frames.frame_size_np(False, 7, 0, 5, 3, 4)
    if name == "both_hostile":
        assert list(d["param_len"]) == [2, 0, 0]
        assert list(sizes) == [frames.frame_size_np(False, 7, 0, 5, 2, 0), frames.frame_size_np(False, 7, 0, 5, 0, 0),
                               frames.frame_size_np(False, 7, 0, 5, 0, 3)]
    if name == "flags_without_arrays":
        assert (d["has_position"] == 0).all() and (d["has_parameter"] == 0).all()
        assert list(sizes) == [frames.frame_size_np(False, 7, 0, 5, None, 3), frames.frame_size_np(False, 7, 0, 1),
                               frames.frame_size_np(False, 7, 0, 2, None, 2)]
    assert len(frame(0))


def test_too_large_frames_are_empty_in_the_sizing_call():
    c, sizes_want = too_large_case()
    data, off, sizes, cnt = frames.build_frames_np(capacity=0, **c.kw())
    assert list(sizes) == sizes_want and len(data) == 0
    assert cnt["error"] == frames.ERROR_TOO_LARGE and cnt["bytes_need"] == sum(sizes_want) and cnt["overflow"] == 1
    assert cnt["n_complete"] == 1          # the empty frame at 0 lies below any capacity


def test_capacity_cuts_the_bytes_and_nothing_else():
    whole, off, sizes, cnt = want("cap_300")
    need = len(whole)
    assert 280 <= need <= 320
    for cap in (0, 1, need // 2 + 1, need - 1, need, need + 1):
        data, o, s, k = frames.build_frames_np(capacity=cap, **cases()["cap_300"].kw())
        assert data.tobytes() == whole[:cap].tobytes() and (o == off).all() and (s == sizes).all()
        assert k == dict(n_frames=2, n_complete=sum(int(e) <= cap for e in off[1:]), bytes_need=need,
                         bytes_written=min(cap, need), overflow=int(need > cap), error=0)


def test_a_parameter_that_is_not_utf8_is_refused():
    c = Case(world=[WORLD], param=(np.array([0xC3, 0x28], np.uint8), np.array([0, 2], np.uint64)))
    with pytest.raises(ValueError):
        frames.build_frames_np(**c.kw())
