#!/usr/bin/env python3
"""The record store (wq_records_*, csrc/wq_records.hip) on an entity-persistence shape derived from
C5, in one process, the forms alternating:

  read         wq_records_read_device without dedupe: 1M queries at C5's entity positions
  read_dedupe  the same with dedupe, on a store that got a batch of fresh duplicates (newer copies of
               stored uuids, most of them in a neighbouring region) before every repeat
  apply        wq_records_apply_device: 1M creates plus 100k deletes (asynchronous; the repeat ends at
               a device synchronise)
  cpu          RecordStoreRef (plain Python) on a 1/100 sample of the rows and queries, reported as such

The store, at --scale 1: 16M rows over ~1M regions of 16 x 256 x 16 (table 1,024), 5% of them under a
uuid another row has too. Before anything is timed a sample of the GPU read is checked against
RecordStoreRef on the same sample store. --warmup untimed and --reps timed repeats per form, a
synchronise on both sides of each; min / mean / max are reported with every number.

Byte budget of a read: per query 24 + 4 + 8 in and 4 out; per row walked 4 (view
entry) + 8 (ts_us) + 16 (uuid); per returned row 12 out.

    python tools/records_bench.py [--scale 1.0] [--reps 5] [--out profiles/records_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes/s
CFG = (16, 256, 16, 1024)


def summary(v):
    return {"mean_ms": round(statistics.fmean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "reps_ms": [round(x, 4) for x in v]}


def ops_tensor(torch, dev, kind, pos, uuid, ts, handle):
    """wq_rec_op records (64 bytes) built on the device: 8 little-endian i64 words per op."""
    n = pos.shape[0]
    t = torch.zeros((n, 8), dtype=torch.int64, device=dev)
    t[:, 0] = kind  # world 0 in the high half
    t[:, 1:4] = pos.view(torch.int64)
    t[:, 5] = uuid  # uuid_hi stays 0
    t[:, 6] = ts
    t[:, 7] = handle
    return t


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records_bench.json"))
    a = ap.parse_args()
    import torch
    from worldql_server_amd import records as R, synth_ext
    from worldql_server_amd.router import Router

    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)
    n_rows = max(1024, int(16_000_000 * a.scale))
    n_q = max(64, int(1_000_000 * a.scale))
    n_create, n_delete = n_q, n_q // 10
    chunk = min(n_rows, 1_000_000)
    # rows: x, z over +-2,896 * scale^(1/3), y over +-1,024: 362 x 8 x 362 = ~1M regions at scale 1
    half_xz, half_y = 2896.0 * a.scale ** (1.0 / 3.0), 1024.0
    g = torch.Generator(device=dev)
    g.manual_seed(1234)

    def rand_pos(n):
        p = torch.rand((n, 3), dtype=torch.float64, device=dev, generator=g) * 2.0 - 1.0
        p[:, 0] *= half_xz
        p[:, 1] *= half_y
        p[:, 2] *= half_xz
        return p

    r = Router(16, 0)
    store = R.GpuRecordStore(r, *CFG)
    sample_every = 100
    ref = R.RecordStoreRef(*CFG)
    sampled = []
    loaded_pos = torch.empty((n_rows, 3), dtype=torch.float64, device=dev)  # the caller's side of the payload
    t0 = time.perf_counter()
    for base in range(0, n_rows, chunk):
        n = min(chunk, n_rows - base)
        pos = rand_pos(n)
        loaded_pos[base:base + n] = pos
        idx = torch.arange(base, base + n, dtype=torch.int64, device=dev)
        # 5%: the uuid of an earlier row (of this chunk's range shifted down), so two rows share it
        dup = torch.rand(n, device=dev, generator=g) < 0.05
        uuid = torch.where(dup, idx // 2, idx)
        ts = 1_000_000 + idx
        ops = ops_tensor(torch, dev, R.CREATE, pos, uuid, ts, idx)
        sync()
        store.apply_device(ops.data_ptr(), n)
        sync()
        s = ops[::sample_every].cpu().numpy().view(R.REC_OP_DTYPE).reshape(-1)
        sampled.append(s.copy())
        ref.apply(s)
    load_s = time.perf_counter() - t0
    live, stored, seen = store.stats()
    out = {"tool": "tools/records_bench.py", "scale": a.scale, "reps": a.reps, "warmup": a.warmup,
           "timing": "host clock, a device synchronise on both sides of every repeat",
           "budget": "read: 36 n_queries in + 4 (n_queries + 1) out + 28 scanned + 12 returned bytes; share of 8 TB/s",
           "store": {"rows": int(stored), "rows_live": int(live), "region_sizes": CFG[:3], "table_size": CFG[3],
                     "load_seconds": round(load_s, 2)}, "forms": {}}

    # queries at C5's entity positions
    c5 = synth_ext.config_c5(scale=a.scale)
    q_pos = torch.from_numpy(np.ascontiguousarray(c5.pos[:n_q], dtype=np.float64)).to(dev)
    q_world = torch.zeros(n_q, dtype=torch.int32, device=dev)
    cap = int(min(4 * n_rows + 1024, 200_000_000))
    off = torch.zeros(n_q + 1, dtype=torch.int32, device=dev)
    hd = torch.zeros(cap, dtype=torch.int32, device=dev)
    ts_out = torch.zeros(cap, dtype=torch.int64, device=dev)
    sync()

    def read(dedupe, n=n_q):
        return store.read_device(n, q_world.data_ptr(), q_pos.data_ptr(), None, dedupe, off.data_ptr(), hd.data_ptr(),
                                 ts_out.data_ptr(), cap)

    # check: a store of the sampled rows alone, read on the GPU, equals RecordStoreRef on the same rows
    chk_router = Router(16, 0)
    chk = R.GpuRecordStore(chk_router, *CFG)
    chk.apply(np.concatenate(sampled))
    n_chk = min(n_q, 20_000)
    qp = np.ascontiguousarray(c5.pos[:n_chk], dtype=np.float64)
    want = ref.read([(0, p, None) for p in qp])
    got = chk.read(np.zeros(n_chk, np.uint32), qp, capacity=int(want["returned"]))
    out["checks"] = {"sample_rows": len(ref.rows), "sample_queries": n_chk, "sample_returned": int(want["returned"]),
                     "gpu_equals_reference_on_sample": bool(
                         all(np.array_equal(got[f], want[f]) for f in ("offsets", "handles", "ts_us"))
                         and got["rejected"] == 0)}
    chk.close()
    chk_router.close()
    if not out["checks"]["gpu_equals_reference_on_sample"]:
        print("the GPU store and RecordStoreRef differ on the sample", flush=True)
        return 1

    res = read(False)
    sync()
    out["read_shape"] = {"queries": n_q, **{k: int(v) for k, v in res.items()}}
    if res["overflow"] or res["error"] or res["rejected"]:
        print("the read overflowed, was cut or rejected queries:", res, flush=True)
        return 1
    # determinism: the same bytes twice
    k = res["returned"]
    first = (off.clone(), hd[:k].clone(), ts_out[:k].clone())
    read(False)
    sync()
    out["checks"]["read_deterministic"] = bool(torch.equal(first[0], off) and torch.equal(first[1], hd[:k])
                                               and torch.equal(first[2], ts_out[:k]))
    del first

    def budget(n, x):
        return 36 * n + 4 * (n + 1) + 28 * x["scanned"] + 12 * x["returned"]

    next_handle = [n_rows]

    def fresh_duplicates():
        """1M newer copies of rows the last read returned, each up to 12 units from its row's stored
        position: the same region or a neighbouring one, nearly always the same table, so the next
        deduping read has about as many rows to kill."""
        n = n_create
        got = hd[torch.randint(0, max(k, 1), (n,), device=dev, generator=g)].to(torch.int64) & 0xFFFFFFFF
        got = got % n_rows  # (a row a previous repeat added stands in for a loaded one)
        pos = loaded_pos[got] + (torch.rand((n, 3), dtype=torch.float64, device=dev, generator=g) - 0.5) * 24.0
        uuid = got  # the handle of a loaded row is its uuid (95% of them)
        idx = torch.arange(next_handle[0], next_handle[0] + n, dtype=torch.int64, device=dev)
        next_handle[0] += n
        ops = ops_tensor(torch, dev, R.CREATE, pos, uuid, 10_000_000_000 + idx, idx)
        sync()
        store.apply_device(ops.data_ptr(), n)
        sync()

    def churn_ops():
        n = n_create + n_delete
        pos = rand_pos(n)
        idx = torch.arange(next_handle[0], next_handle[0] + n, dtype=torch.int64, device=dev)
        next_handle[0] += n
        kind = torch.zeros(n, dtype=torch.int64, device=dev)
        kind[torch.randperm(n, device=dev, generator=g)[:n_delete]] = R.DELETE
        # a delete names a loaded row's uuid at a random position: few hit (the region must match)
        uuid = torch.where(kind == R.DELETE, torch.randint(0, n_rows, (n,), device=dev, generator=g), idx)
        return ops_tensor(torch, dev, kind, pos, uuid, 20_000_000_000 + idx, idx), n

    times = {"read": [], "read_dedupe": [], "apply": []}
    extra = {"read": None, "read_dedupe": [], "apply": []}
    for rep in range(a.warmup + a.reps):
        timed = rep >= a.warmup
        # read
        sync()
        t = time.perf_counter()
        x = read(False)
        sync()
        if timed:
            times["read"].append((time.perf_counter() - t) * 1e3)
            extra["read"] = x
        # read with dedupe on fresh duplicates; the compaction of the views is part of neither: the
        # apply left them merged, and the rows this read kills leave at the next read
        fresh_duplicates()
        read(False, 1)  # compacts what the previous repeat's dedupe and deletes killed
        sync()
        t = time.perf_counter()
        x = read(True)
        sync()
        if timed:
            times["read_dedupe"].append((time.perf_counter() - t) * 1e3)
            extra["read_dedupe"].append(x)
        read(False, 1)
        # apply
        ops, n = churn_ops()
        sync()
        t = time.perf_counter()
        store.apply_device(ops.data_ptr(), n)
        sync()
        if timed:
            times["apply"].append((time.perf_counter() - t) * 1e3)
            extra["apply"].append(n)
        read(False, 1)
        sync()

    x = extra["read"]
    ms = statistics.fmean(times["read"])
    out["forms"]["read"] = {"times": summary(times["read"]), **{k_: int(v) for k_, v in x.items()},
                            "rows_per_s": round(x["returned"] / (ms * 1e-3)), "queries_per_s": round(n_q / (ms * 1e-3)),
                            "budget_bytes": budget(n_q, x),
                            "share_of_8TBs": round(budget(n_q, x) / (ms * 1e-3) / HBM_PEAK, 4)}
    xs = extra["read_dedupe"]
    ms = statistics.fmean(times["read_dedupe"])
    ret = statistics.fmean(v["returned"] for v in xs)
    out["forms"]["read_dedupe"] = {"times": summary(times["read_dedupe"]), "returned_mean": round(ret),
                                   "deduped_rows": [int(v["deduped_rows"]) for v in xs],
                                   "scanned_mean": round(statistics.fmean(v["scanned"] for v in xs)),
                                   "rows_per_s": round(ret / (ms * 1e-3)),
                                   "budget_bytes": round(statistics.fmean(budget(n_q, v) for v in xs)),
                                   "share_of_8TBs": round(statistics.fmean(budget(n_q, v) for v in xs) / (ms * 1e-3)
                                                          / HBM_PEAK, 4)}
    ms = statistics.fmean(times["apply"])
    n_ops = n_create + n_delete
    live, stored, seen = store.stats()
    out["forms"]["apply"] = {"times": summary(times["apply"]), "ops": n_ops, "creates": n_create, "deletes": n_delete,
                             "ops_per_s": round(n_ops / (ms * 1e-3)), "rows_stored_after": int(stored),
                             "rows_live_after": int(live),
                             "budget_bytes": 64 * n_ops + 2 * 4 * 2 * int(stored) + 60 * n_create,
                             "share_of_8TBs": round((64 * n_ops + 16 * int(stored) + 60 * n_create) / (ms * 1e-3)
                                                    / HBM_PEAK, 4)}
    store.close()
    r.close()

    # the CPU baseline: RecordStoreRef on the 1/100 sample of the loaded rows and of the queries
    qs = [(0, p, None) for p in c5.pos[:n_q:sample_every]]
    cpu = []
    for _ in range(3):
        t = time.perf_counter()
        y = ref.read(qs)
        cpu.append((time.perf_counter() - t) * 1e3)
    ms = statistics.fmean(cpu)
    out["forms"]["cpu"] = {"what": "RecordStoreRef (plain Python) on a 1/100 sample: rows and queries",
                           "rows": len(ref.rows), "queries": len(qs), "times": summary(cpu), "returned": int(y["returned"]),
                           "rows_per_s": round(y["returned"] / (ms * 1e-3)) if ms else 0,
                           "queries_per_s": round(len(qs) / (ms * 1e-3)) if ms else 0}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k_: (v.get("times", {}).get("mean_ms"), v.get("share_of_8TBs")) for k_, v in out["forms"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
