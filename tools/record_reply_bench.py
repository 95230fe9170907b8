#!/usr/bin/env python3
"""The record reply builder (wq_frames_build_records_device, csrc/wq_reply.hip) against the host leg it replaces
and against the floor of its copy, in one process, the forms alternating:

  hip      Router.build_record_frames_device on a slab, a CSR of handles and the queries' world names already in
           device memory, into a buffer of bytes_need, with sizes and counters, asynchronous, no read-back;
  host     wq_serialize_messages on 16 host threads over prepared wq_message_in / wq_record_in arrays (built once,
           outside the timing, from the same slab) into pinned memory, plus the upload of frames, offsets and
           sizes: the leg the call replaces once the records are gathered;
  d2d      one device-to-device copy of bytes_need: the floor;
  python   the per-record gather before the host serializer (one dict per returned handle), on the first 1/100 of
           the rows, scaled by handles. A statement about per-record Python.

Shapes (records have a 100 - 200 byte data string and a position; every fourth a 16-byte flex):
  read_1m        1M queries of about 20 records each (the records bench's read);
  rows_100       10,000 rows of 100;
  one_big_row    one row of 1M records among 10,000 rows of 10;
  spread         the same records as 10,100 rows of 100: what one_big_row is compared with. Other
                 element-parallel calls here stay within 1.1 - 1.5x of their spread shape (README); the JSON
                 holds the ratio, and a ratio outside that band is a finding to explain, not to hide;
  flex_256x1m    256 rows of one record with a 1 MiB flex.

hip's frames on the first 200 rows are checked equal to frames.build_record_frames_np's, and a second call
byte-identical, before anything is timed. --warmup untimed and --reps timed repeats per form, a device synchronise
on both sides of each; min / mean / max with every number; every ratio as measured.

    python tools/record_reply_bench.py [--scale 1.0] [--only read_1m,...] [--reps 7] [--warmup 3]
                                       [--out profiles/record_reply_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORLDS = ["world", "nether", "the_end", "a_b"]
REC_IN = np.dtype([("uuid", np.uint8, (16,)), ("has_position", np.uint8), ("has_data", np.uint8), ("has_flex", np.uint8),
                   ("pad_", np.uint8, (5,)), ("position", np.float64, (3,)), ("world_name", np.uint64), ("world_len", np.uint64),
                   ("data", np.uint64), ("data_len", np.uint64), ("flex", np.uint64), ("flex_len", np.uint64)])
MSG_IN = np.dtype([("instruction", np.uint8), ("replication", np.uint8), ("has_position", np.uint8), ("has_parameter", np.uint8),
                   ("has_flex", np.uint8), ("pad_", np.uint8, (3,)), ("sender_uuid", np.uint8, (16,)), ("position", np.float64, (3,)),
                   ("parameter", np.uint64), ("parameter_len", np.uint64), ("world_name", np.uint64), ("world_len", np.uint64),
                   ("flex", np.uint64), ("flex_len", np.uint64), ("records", np.uint64), ("n_records", np.uint64),
                   ("entities", np.uint64), ("n_entities", np.uint64)])
assert REC_IN.itemsize == 96 and MSG_IN.itemsize == 128


def summary(v):
    return {"mean_ms": round(statistics.fmean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "reps_ms": [round(x, 4) for x in v]}


def make_slab(n_rec, rng, flex_bytes=None):
    """(entries, arena): n_rec live records."""
    from worldql_server_amd import abi
    e = np.zeros(n_rec, abi.SLAB_ENTRY_DTYPE)
    e["uuid"] = rng.integers(0, 256, (n_rec, 16), dtype=np.uint8)
    e["pos"] = rng.uniform(-4000, 4000, (n_rec, 3))
    e["world"] = rng.integers(0, len(WORLDS), n_rec)
    if flex_bytes is None:
        dl = rng.integers(100, 201, n_rec)
        fl = np.where(np.arange(n_rec) % 4 == 0, 16, 0)
        bits = abi.SLAB_DATA | abi.SLAB_POSITION | abi.SLAB_LIVE | np.where(fl > 0, abi.SLAB_FLEX, 0)
    else:
        dl, fl = np.zeros(n_rec, np.int64), np.full(n_rec, flex_bytes)
        bits = np.full(n_rec, abi.SLAB_FLEX | abi.SLAB_POSITION | abi.SLAB_LIVE)
    e["bits"], e["data_len"], e["flex_len"] = bits, dl, fl
    e["off"] = np.cumsum(dl + fl) - (dl + fl)
    arena = rng.integers(97, 123, int((dl + fl).sum()), dtype=np.uint8)
    return e, arena


def shape(name, scale, rng):
    """(entries, arena, row_offsets, handles)."""
    if name == "flex_256x1m":
        n = max(int(256 * scale), 2)
        e, arena = make_slab(n, rng, 1 << 20)
        return e, arena, np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32)
    pool = max(int(1_000_000 * scale), 1000)
    e, arena = make_slab(pool, rng)
    if name == "read_1m":
        lens = rng.integers(15, 26, max(int(1_000_000 * scale), 10))
    elif name == "rows_100":
        lens = np.full(max(int(10_000 * scale), 10), 100)
    elif name == "one_big_row":
        lens = np.full(max(int(10_000 * scale), 10) + 1, 10)
        lens[len(lens) // 2] = max(int(1_000_000 * scale), 1000)
    else:
        lens = np.full(max(int(10_100 * scale), 10), 100)
    off = np.zeros(len(lens) + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    handles = rng.integers(0, pool, int(off[-1])).astype(np.uint32)
    return e, arena, off, handles


def host_inputs(e, arena, off, handles, names):
    """wq_message_in / wq_record_in arrays over the slab's bytes: prepared once, outside the timing."""
    from worldql_server_amd import abi
    table = [np.frombuffer(w.encode(), np.uint8).copy() for w in WORLDS]
    rec = np.zeros(len(handles), REC_IN)
    h = e[handles]
    rec["uuid"], rec["position"] = h["uuid"], h["pos"]
    rec["has_position"] = 1
    rec["has_data"] = (h["bits"] & abi.SLAB_DATA) != 0
    rec["has_flex"] = (h["bits"] & abi.SLAB_FLEX) != 0
    rec["world_name"] = np.array([t.ctypes.data for t in table], np.uint64)[h["world"]]
    rec["world_len"] = np.array([len(t) for t in table], np.uint64)[h["world"]]
    rec["data"], rec["data_len"] = arena.ctypes.data + h["off"], h["data_len"]
    rec["flex"], rec["flex_len"] = arena.ctypes.data + h["off"] + h["data_len"], h["flex_len"]
    n = len(off) - 1
    msg = np.zeros(n, MSG_IN)
    msg["instruction"] = 12
    msg["world_name"], msg["world_len"] = names.ctypes.data, 5
    msg["records"] = rec.ctypes.data + 96 * off[:-1].astype(np.uint64)
    msg["n_records"] = np.diff(off.astype(np.int64))
    msg["entities"] = rec.ctypes.data
    return msg, rec, table


def run_shape(name, a, r, rng):
    import torch
    from worldql_server_amd import abi, codec, frames
    e, arena, off, handles = shape(name, a.scale, rng)
    n, dev = len(off) - 1, torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    names = np.frombuffer(b"world", np.uint8).copy()
    d_e, d_arena, d_off, d_h, d_names = up(e), up(arena), up(off), up(handles), up(names)
    d_woff, d_wlen = up(np.zeros(n, np.uint64)), up(np.full(n, 5, np.uint32))
    src = abi.FramesSrc(instruction_all=12)
    view = abi.SlabView(entries=d_e.data_ptr(), n_entries=len(e), payload=d_arena.data_ptr(), n_payload_bytes=len(arena))

    def rec_src(rows, n_handles):
        return abi.FramesRecSrc(row_offsets=d_off.data_ptr(), handles=d_h.data_ptr(), n_handles=n_handles, slab=view,
                                world_bytes=d_names.data_ptr(), world_off=d_woff.data_ptr(), world_len=d_wlen.data_ptr(),
                                n_world_bytes=5, flags=0)

    fo = torch.empty(n + 1, dtype=torch.int64, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.empty(abi.FRAMES_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    counters = lambda: cnt.cpu().numpy().view(abi.FRAMES_COUNTERS_DTYPE)[0]   # noqa: E731
    torch.cuda.synchronize()
    # the sample against the definition, twice
    k = min(n, 200)
    rk = rec_src(k, int(off[k]))
    want = frames.build_record_frames_np(WORLDS, None, None, off[:k + 1], handles[:int(off[k])], e, arena, instruction=12,
                                         world_bytes=names, world_off=np.zeros(k, np.uint64), world_len=np.full(k, 5, np.uint32))
    buf = torch.empty(max(want[3]["bytes_need"], 16), dtype=torch.uint8, device=dev)
    for _ in range(2):
        buf.zero_()
        torch.cuda.synchronize()
        r.build_record_frames_device(src, rk, k, buf.data_ptr(), want[3]["bytes_need"], fo.data_ptr(), sizes.data_ptr(), cnt.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(buf[:want[3]["bytes_need"]].cpu().numpy(), want[0]) and int(counters()["error"]) == 0, name
    rn = rec_src(n, len(handles))
    r.build_record_frames_device(src, rn, n, None, 0, fo.data_ptr(), None, cnt.data_ptr())
    torch.cuda.synchronize()
    need = int(counters()["bytes_need"])
    out = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    floor_src = torch.zeros(max(need, 16), dtype=torch.uint8, device=dev)

    def hip():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.build_record_frames_device(src, rn, n, out.data_ptr(), need, fo.data_ptr(), sizes.data_ptr(), cnt.data_ptr())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def d2d():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out.copy_(floor_src)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    msg, rec, keep = host_inputs(e, arena, off, handles, names)
    lib = codec._lib()
    pin = torch.empty(max(need, 16), dtype=torch.uint8).pin_memory()
    pin_off = torch.empty(n + 1, dtype=torch.int64).pin_memory()
    h_off = pin_off.numpy().view(np.uint64)

    def host():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.wq_serialize_messages(msg.ctypes.data, n, pin.data_ptr(), need, h_off.ctypes.data, 16)
        assert rc == 0, rc
        out.copy_(pin[:out.numel()], non_blocking=True)
        fo.copy_(pin_off, non_blocking=True)
        sizes.copy_(torch.from_numpy(np.diff(h_off.view(np.int64)).astype(np.int32)), non_blocking=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    forms = {"hip": hip, "host": host, "d2d": d2d}
    times = {f: [] for f in forms}
    for i in range(a.warmup + a.reps):
        for f, fn in forms.items():
            t = fn()
            if i >= a.warmup:
                times[f].append(t)
    hip()
    got = out[:need].cpu().numpy().copy()
    host()
    assert np.array_equal(out[:need].cpu().numpy(), got), name + ": the host serializer's bytes differ"
    s = max(n // 100, 1)
    t0 = time.perf_counter()
    gathered = [[dict(uuid=bytes(e[h]["uuid"]), position=tuple(e[h]["pos"]), data=arena[int(e[h]["off"]):int(e[h]["off"]) + int(e[h]["data_len"])].tobytes())
                 for h in handles[int(off[i]):int(off[i + 1])]] for i in range(s)]
    py_ms = (time.perf_counter() - t0) * 1e3 * len(handles) / max(int(off[s]), 1)
    del gathered
    m = {f: statistics.fmean(v) for f, v in times.items()}
    res = {"rows": n, "handles": len(handles), "bytes_need": need, "hip": summary(times["hip"]), "host": summary(times["host"]),
           "d2d": summary(times["d2d"]), "python_gather_scaled_ms": round(py_ms, 1), "python_sample_rows": s,
           "host_over_hip": round(m["host"] / m["hip"], 3), "hip_over_d2d": round(m["hip"] / m["d2d"], 3),
           "fraction_of_hbm": round(2 * need / 8e12 / (m["hip"] * 1e-3), 4)}
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default="read_1m,rows_100,one_big_row,spread,flex_256x1m")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "record_reply_bench.json"))
    a = ap.parse_args()
    import torch
    from worldql_server_amd.router import Router
    if not torch.cuda.is_available():
        raise SystemExit("record_reply_bench needs a GPU")
    rng = np.random.default_rng(17)
    r = Router(16, 0)
    r.set_worlds(WORLDS)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "scale": a.scale, "shapes": {}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for name in a.only.split(","):
        out["shapes"][name] = run_shape(name, a, r, rng)
        sh = out["shapes"]
        if "one_big_row" in sh and "spread" in sh:
            out["one_big_row_over_spread"] = round(sh["one_big_row"]["hip"]["mean_ms"] / sh["spread"]["hip"]["mean_ms"], 3)
        with open(a.out, "w") as f:   # after every shape: a later shape that runs out of memory or time loses nothing
            json.dump(out, f, indent=1)
            f.write("\n")
    r.close()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
