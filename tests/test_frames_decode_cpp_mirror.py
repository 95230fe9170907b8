"""The ingest decoder's arithmetic (csrc/decode_ops.hpp) on the CPU, through
tests/cpp/frames_decode_host_shim.hip: the bounded reader, the verifier walk over Message, Record and
Entity, UTF-8 by chunks, parse_uuid, the sanitizer stream and the two lookups, in the kernels' passes —
the walk with the work list at capacity 0, 1 and the default, the strings pass in the grid's order, the
finish — byte for byte against worldql_server_amd/ingest.py (decode_frames_np). No GPU needed (the GPU
instance: tests/test_gpu_frames_decode.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import abi, codec, frames, ingest

from test_frames_decode_host import (CHUNK, L, MIB, PEER_IDS, PEER_UUIDS, TILE, WORLDS, batches, definition, same,
                                     shared_data_frame, small_names)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xC5
CAPS = (0, 1, -1)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


class ShimIn(ctypes.Structure):  # struct wq_test_decode_in
    _fields_ = [("frames", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("n_frames", ctypes.c_uint64),
                ("n_frame_bytes", ctypes.c_uint64), ("world_bytes", ctypes.c_void_p), ("world_off", ctypes.c_void_p),
                ("peer_uuids", ctypes.c_void_p), ("peer_ids", ctypes.c_void_p), ("n_worlds", ctypes.c_uint32),
                ("n_peers", ctypes.c_uint32), ("list_cap", ctypes.c_int64)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("decode_shim") / "libdecodeshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                           "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "frames_decode_host_shim.hip")])
    lib = ctypes.CDLL(out)
    lib.wq_test_frames_decode_host.restype = ctypes.c_int
    lib.wq_test_frames_decode_host.argtypes = [ctypes.POINTER(ShimIn), ctypes.POINTER(abi.IngestOut), ctypes.c_void_p,
                                               ctypes.c_void_p]
    for f in ("lane", "chunk", "tile", "list_default"):
        getattr(lib, "wq_test_decode_" + f).restype = ctypes.c_uint32
    return lib


WIDTH = dict(msg=72, pos=24, world=4, sender=4, repl=1, instruction=1, sender_uuid=16, flex_range=8, flags=1)
SHAPE = dict(msg=lambda a, n: a.view(codec.DECODED_DTYPE), pos=lambda a, n: a.view(np.float64).reshape(n, 3),
             world=lambda a, n: a.view(np.uint32), sender=lambda a, n: a.view(np.uint32), repl=lambda a, n: a,
             instruction=lambda a, n: a, sender_uuid=lambda a, n: a.reshape(n, 16),
             flex_range=lambda a, n: a.view(np.uint32).reshape(n, 2), flags=lambda a, n: a)
TAIL = 64


def shim_call(lib, data, offsets, nb=None, cap=-1, fields=ingest.OUT_FIELDS, with_counters=True, shift=0, worlds=WORLDS,
              peers=(PEER_UUIDS, PEER_IDS)):
    """The shim on exactly sized inputs (the frame bytes `shift` bytes behind a 16-byte boundary, ending
    with the buffer) with canaries behind every output: a dict like decode_frames_np's, outputs left out
    as None, plus `listed` and `chunks`."""
    n = len(offsets) - 1
    nb = len(data) if nb is None else nb
    raw = np.full(len(data) + shift + 16, CANARY, np.uint8)
    base = (-raw.ctypes.data) % 16 + shift
    fr = raw[base:base + len(data)]
    fr[:] = data
    off = np.array(offsets, dtype=np.uint64, copy=True)
    wb, wo = frames.world_table(worlds or [])
    wbuf = np.frombuffer(wb, np.uint8).copy() if wb else np.zeros(1, np.uint8)
    pu = ingest.uuid_rows(peers[0] if peers else [])
    pi = None if not peers or peers[1] is None else np.asarray(peers[1], np.uint32)
    outs = {k: np.full(n * WIDTH[k] + TAIL, CANARY, np.uint8) for k in fields}
    cnt = np.full(64 + TAIL, CANARY, np.uint8)
    stats = np.zeros(2, np.uint64)
    a = ShimIn(frames=fr.ctypes.data if len(data) else None, offsets=off.ctypes.data, n_frames=n, n_frame_bytes=nb,
               world_bytes=wbuf.ctypes.data, world_off=wo.ctypes.data, peer_uuids=pu.ctypes.data if len(pu) else None,
               peer_ids=None if pi is None else pi.ctypes.data, n_worlds=len(worlds or []), n_peers=len(pu), list_cap=cap)
    o = abi.IngestOut(**{k: v.ctypes.data for k, v in outs.items()})
    rc = lib.wq_test_frames_decode_host(ctypes.byref(a), ctypes.byref(o), cnt.ctypes.data if with_counters else None,
                                        stats.ctypes.data)
    assert rc == 0
    assert fr.tobytes() == np.asarray(data, np.uint8).tobytes() and off.tobytes() == np.asarray(offsets, np.uint64).tobytes()
    got = dict.fromkeys(ingest.OUT_FIELDS)
    for k, v in outs.items():
        assert (v[n * WIDTH[k]:] == CANARY).all(), "written behind " + k
        got[k] = SHAPE[k](v[:n * WIDTH[k]].copy(), n)
    if with_counters:
        assert (cnt[64:] == CANARY).all()
        c = cnt[:64].view(abi.INGEST_COUNTERS_DTYPE)[0]
        got["counters"] = {k: int(c[k]) for k in abi.INGEST_COUNTERS_DTYPE.names if k != "pad_"}
    else:
        assert (cnt == CANARY).all()
    got["listed"], got["chunks"] = int(stats[0]), int(stats[1])
    return got


def test_constants(shim):
    assert (shim.wq_test_decode_lane(), shim.wq_test_decode_chunk(), shim.wq_test_decode_tile()) == (L, CHUNK, TILE)


@pytest.mark.parametrize("name", small_names())
def test_kernel_arithmetic_matches_the_definition(shim, name):
    data, offsets, nb = batches()[name]
    want = definition(name)
    for cap in CAPS:
        got = shim_call(shim, data, offsets, nb, cap=cap)
        same(got, want, f"{name} with list capacity {cap}")
        assert got["listed"] <= max(cap, 0) or cap < 0


def test_frames_of_2_to_the_32_bytes_are_refused_unread(shim):
    """Offsets that claim a 4 GiB frame behind frame 0: only frame 0's 136 bytes exist."""
    data, offsets, nb = batches()["offsets_huge"]
    same(shim_call(shim, data, offsets, nb), definition("offsets_huge"), "offsets_huge")


def test_long_strings_take_the_list_and_the_lane_path(shim):
    data, offsets, nb = batches()["long_strings"]
    lens = [L - 1, L, L + 1, TILE - 1, TILE, TILE + 1, MIB]
    n_long = sum(1 + len({0, n - 1, CHUNK - 1, CHUNK, L - 1, L, TILE - 1, TILE, n - CHUNK - 1, n - CHUNK} & set(range(n)))
                 for n in lens if n > L)
    ample, one, none = (shim_call(shim, data, offsets, nb, cap=c) for c in (-1, 1, 0))
    assert (ample["listed"], one["listed"], none["listed"], none["chunks"]) == (n_long, 1, 0, 0)
    assert one["chunks"] == -(-(L + 1) // CHUNK) and ample["chunks"] > 7 * MIB // CHUNK


@pytest.mark.parametrize("shift", range(16))
def test_the_frame_stream_at_every_residue(shim, shift):
    for name in ("corpus_1", "straddle"):
        data, offsets, nb = batches()[name]
        same(shim_call(shim, data, offsets, nb, shift=shift), definition(name), f"{name} at residue {shift}")


def test_nullable_outputs(shim):
    data, offsets, nb = batches()["corpus_2"]
    want = definition("corpus_2")
    combos = [()] + [(k,) for k in ingest.OUT_FIELDS] + [tuple(k for k in ingest.OUT_FIELDS if k != "msg"),
                                                       ("pos", "world", "sender", "repl"), ("msg", "flags")]
    for fields in combos:
        for with_counters in (True, False):
            same(shim_call(shim, data, offsets, nb, fields=fields, with_counters=with_counters), want, str(fields))


def test_tables_none_ids_by_index_and_duplicates(shim):
    data, offsets, nb = batches()["hand"]
    for worlds, peers in ((None, None), (WORLDS, (PEER_UUIDS, None)), (WORLDS[::-1], (PEER_UUIDS[::-1], PEER_IDS)),
                          (["world"] * 40 + WORLDS, None)):
        want = ingest.decode_frames_np(data, offsets, worlds, peers[0] if peers else None, peers[1] if peers else None)
        same(shim_call(shim, data, offsets, worlds=worlds, peers=peers), want)
    twice = ingest.uuid_rows([PEER_UUIDS[1], PEER_UUIDS[1]])
    a = ShimIn(n_peers=2, peer_uuids=twice.ctypes.data, list_cap=-1)
    assert shim.wq_test_frames_decode_host(ctypes.byref(a), ctypes.byref(abi.IngestOut()), None, None) == -1


def test_one_string_shared_past_the_apparent_size_limit(shim):
    """A 1 MiB string referenced by 2,049 records' data fields: 1.1 MB of frame, more than 2^31 apparent
    bytes. With one list slot the first reference is listed and the lane validates the rest itself."""
    f = shared_data_frame(2049, MIB)
    data, offsets = codec.pack_frames([shared_data_frame(3, 300), f, shared_data_frame(3, 300)])
    want = ingest.decode_frames_np(data, offsets, WORLDS, PEER_UUIDS, PEER_IDS)
    assert want["msg"]["status"].tolist() == [0, 1, 0]
    got = shim_call(shim, data, offsets, cap=1)
    same(got, want, "shared string")
    assert got["listed"] == 1
