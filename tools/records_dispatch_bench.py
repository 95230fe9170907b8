#!/usr/bin/env python3
"""The record dispatch (wq_records_dispatch_device, csrc/wq_recdispatch.hip) against the decoder on the same
frames and against the host leg it replaces, in one process, the forms alternating:

  hip      Router.records_dispatch_device on frames and decoder outputs already in device memory, every
           output and the counters, asynchronous, no read-back;
  decode   Router.decode_frames_device on the same frames: the yardstick. The decoder verifies every byte
           of every frame; the dispatch walks the records vectors again (twice for an accepted record);
  host     the per-record Python the call replaces, on the first 1/100 of the frames, scaled by bytes:
           codec.decode_packed and ingest.records_dispatch_np (the walk, sanitize, lookup and packability of
           every record, then the wq_rec_op rows). A statement about per-record Python, not about a tuned
           host implementation.

Shapes (frames are serialized on the host from a pool of distinct messages and replicated):
  records_100     10,000 create frames of 100 records each (the decode bench's shape);
  frames_1        1M create frames of 1 record;
  one_big_frame   one create frame of 999,999 records (with its root table the verifier's limit of 1,000,000
                  tables a frame) among 10,000 frames of 1 record; the decoder walks a frame with one lane,
                  so its form is timed once here, not --reps times;
  spread          1,010,000 records as 10,100 frames of 100: what one_big_frame is compared with;
  mix             1M frames, half creates of 1 record, half reads.

hip's outputs on the sample are checked equal to records_dispatch_np's, and a second call byte-identical,
before anything is timed. Then --warmup untimed and --reps timed repeats per form, a synchronise on both
sides of each; min / mean / max with every number. bytes_moved is what the call must read and write once:
the frame bytes, the decoder's msg / world / flags per frame, the ops and references it writes, the query
rows and the classes.

    python tools/records_dispatch_bench.py [--scale 1.0] [--only records_100,...] [--reps 7] [--warmup 3]
                                           [--out profiles/records_dispatch_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import uuid

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
WORLDS = ["world", "nether", "the_end", "a_b"]
RAW = ["world", "nether", "the_end", "a b"]
SIZES, TABLE_SIZE = (16, 16, 16), 1024
NOW = 1_700_000_000_000_000
PEER = uuid.UUID(int=1)


def summary(v):
    return {"mean_ms": round(statistics.fmean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "reps_ms": [round(x, 4) for x in v]}


def record(rng):
    return dict(uuid=uuid.UUID(int=int(rng.integers(1, 1 << 62))), world_name=RAW[int(rng.integers(0, 4))],
                position=(float(rng.uniform(-4000, 4000)), float(rng.uniform(-64, 320)), float(rng.uniform(-4000, 4000))),
                data="payload-%d" % int(rng.integers(0, 1000)), flex=b"\x01\x02\x03\x04")


def create(rng, k):
    return dict(instruction=8, sender_uuid=PEER, world_name="world", records=[record(rng) for _ in range(k)])


def read(rng):
    return dict(instruction=9, sender_uuid=PEER, world_name=RAW[int(rng.integers(0, 4))], parameter="1699999999000",
                position=(float(rng.uniform(-4000, 4000)), 64.0, float(rng.uniform(-4000, 4000))))


def replicate(pool, n):
    """n frames: the pool's serialized frames repeated in order. (data u8, offsets u64)."""
    from worldql_server_amd import codec
    data, off = codec.serialize_messages(pool)
    reps = -(-n // len(pool))
    sizes = np.tile(np.diff(off.astype(np.int64)), reps)[:n]
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(sizes, out=offsets[1:])
    return np.tile(data, reps)[:int(offsets[-1])], offsets


def shape_frames(name, scale):
    rng = np.random.default_rng(11)
    n = lambda v: max(int(v * scale), 1)  # noqa: E731
    if name == "records_100":
        return replicate([create(rng, 100) for _ in range(100)], n(10_000))
    if name == "frames_1":
        return replicate([create(rng, 1) for _ in range(1000)], n(1_000_000))
    if name == "spread":
        return replicate([create(rng, 100) for _ in range(100)], n(10_100))
    if name == "mix":
        return replicate([create(rng, 1) if k % 2 else read(rng) for k in range(1000)], n(1_000_000))
    if name == "one_big_frame":
        from worldql_server_amd import codec
        small, so = replicate([create(rng, 1) for _ in range(1000)], n(10_000))
        pool = [record(rng) for _ in range(1000)]
        big, _ = codec.serialize_messages([dict(instruction=8, sender_uuid=PEER, world_name="world",
                                                records=[pool[k % 1000] for k in range(n(999_999))])])
        half = len(so) // 2   # the big frame in the middle of the small ones
        cut = int(so[half])
        data = np.concatenate([small[:cut], big, small[cut:]])
        offsets = np.concatenate([so[:half + 1], so[half:] + np.uint64(len(big))])
        return data, offsets
    raise ValueError(name)


def run_shape(name, a, torch, r, tick):
    from worldql_server_amd import abi, codec, ingest
    dev = torch.device("cuda:0")
    data, offsets = shape_frames(name, a.scale)
    n = len(offsets) - 1
    d_frames = torch.from_numpy(data).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
    tick.decode(d_frames, d_off)
    torch.cuda.synchronize()
    limit = len(data) // 64   # the caller's bound: a record of these frames takes more than 64 bytes
    out_rows = dict(cls=(n, 1), ops=(limit, 64), op_ref=(limit, 32), q_src=(n, 4), q_world=(n, 4), q_pos=(n, 24), q_after=(n, 8),
                    defer=(limit + n, 8), runs=(n + 1, 16))
    buf = {k: torch.empty(max(rows * w, 8), dtype=torch.uint8, device=dev) for k, (rows, w) in out_rows.items()}
    cnt = torch.zeros(abi.RECDISP_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    o = tick.out
    src = abi.RecDispatchIn(frames=d_frames.data_ptr(), frame_offsets=d_off.data_ptr(), n_frames=n, n_frame_bytes=len(data),
                            msg=o.msg, world=o.world, flags=o.flags, db_src=None, n_db=n, now_us=NOW, free_handles=None,
                            n_free=0, handle_next=0, max_records=limit)
    out = abi.RecDispatchOut(**{k: t.data_ptr() for k, t in buf.items()}, ops_capacity=limit, defer_capacity=limit + n,
                             runs_capacity=n + 1)

    def hip():
        r.records_dispatch_device(src, out, cnt.data_ptr())

    def decode():
        tick.decode(d_frames, d_off)

    def sync():
        torch.cuda.synchronize(dev)

    # correctness first: the whole call's counters, a second call's bytes, and the sample against the definition
    hip()
    sync()
    c = ingest.records_dispatch_counters(cnt.cpu().numpy())
    n_ops = c["n_creates"] + c["n_deletes"]
    first = buf["ops"][:64 * n_ops].cpu().numpy().copy()
    hip()
    sync()
    assert (buf["ops"][:64 * n_ops].cpu().numpy() == first).all() and c["error"] == 0 and c["overflow"] == 0, c
    assert c["n_skip"] == 0, "a frame did not decode"
    k = max(n // 100, 1)
    s_data, s_off = data[:int(offsets[k])], offsets[:k + 1]
    t0 = time.perf_counter()
    codec.decode_packed(s_data, s_off)
    t_decode = time.perf_counter() - t0
    full = ingest.decode_frames_np(s_data, s_off, WORLDS, [PEER])
    t0 = time.perf_counter()
    want = ingest.records_dispatch_np(s_data, s_off, full, None, SIZES, WORLDS, NOW)
    t_np = time.perf_counter() - t0
    n_s = len(want["ops"])
    assert first[:64 * n_s].tobytes() == want["ops"].tobytes(), "the sample's ops differ from the definition's"
    assert buf["q_after"][:8 * len(want["q_after"])].cpu().numpy().tobytes() == want["q_after"].tobytes()

    times = {"hip": [], "decode": []}
    once = name == "one_big_frame"   # one lane walks the big frame for seconds: one timed decode, no warm-up
    for rep in range(a.warmup + a.reps):
        for form, fn in (("hip", hip), ("decode", decode)) if rep % 2 == 0 else (("decode", decode), ("hip", hip)):
            if form == "decode" and once and rep != a.warmup:
                continue
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rep >= a.warmup:
                times[form].append((time.perf_counter() - t0) * 1e3)
    moved = len(data) + n * (8 + 72 + 4 + 1) + n_ops * 96 + c["n_read"] * 40 + n
    res = dict(n_frames=n, frame_bytes=int(len(data)), counters=c, hip=summary(times["hip"]), decode=summary(times["decode"]),
               bytes_moved=int(moved))
    res["hip_over_decode"] = round(res["hip"]["mean_ms"] / res["decode"]["mean_ms"], 3)
    res["fraction_of_8TBs"] = round(moved / (res["hip"]["mean_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
    res["host_sample"] = dict(frames=k, decode_packed_ms=round(t_decode * 1e3, 3), records_dispatch_np_ms=round(t_np * 1e3, 3),
                              scaled_to_all_frames_ms=round((t_decode + t_np) * 1e3 * len(data) / len(s_data), 1),
                              note="per-record Python on the first 1/100 of the frames, scaled by the frame bytes")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default="records_100,frames_1,one_big_frame,spread,mix")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records_dispatch_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("records_dispatch_bench: no GPU; the measurement does not fall back")
    from worldql_server_amd import ingest, records
    from worldql_server_amd.router import Router
    r = Router(16, 0)
    r.set_worlds(WORLDS)
    r.set_ingest_peers([PEER])
    store = records.GpuRecordStore(r, *SIZES, TABLE_SIZE)
    tick = ingest.IngestTick(r)
    result = dict(device=torch.cuda.get_device_name(0), scale=a.scale, reps=a.reps, warmup=a.warmup, shapes={})
    for name in a.only.split(","):
        t0 = time.perf_counter()
        result["shapes"][name] = run_shape(name, a, torch, r, tick)
        s = result["shapes"][name]
        print(f"{name}: hip {s['hip']['mean_ms']} ms ({s['hip']['min_ms']} - {s['hip']['max_ms']}), decode {s['decode']['mean_ms']} ms, "
              f"ratio {s['hip_over_decode']}, {s['fraction_of_8TBs']} of 8 TB/s, host sample scaled {s['host_sample']['scaled_to_all_frames_ms']} ms "
              f"[{time.perf_counter() - t0:.1f} s]", flush=True)
    store.close()
    r.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"hip_ms": v["hip"]["mean_ms"], "decode_ms": v["decode"]["mean_ms"]} for k, v in result["shapes"].items()}))


if __name__ == "__main__":
    main()
