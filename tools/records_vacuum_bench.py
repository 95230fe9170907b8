#!/usr/bin/env python3
"""Vacuum, export and import of the record store (wq_records_vacuum / _export_device /
_import_device, csrc/wq_records.hip) in one process, the forms alternating:

  vacuum        wq_records_vacuum of a store whose stored rows are about half dead
  export        wq_records_export_device of the same store (before its vacuum) into a device buffer
  import        wq_records_import_device of that snapshot into a fresh store on another handle
  reapply       the baseline, what there was before: a fresh store filled by wq_records_apply_device with
                one create per live row in batches of 1M (the ops are built before the clock starts)
  read_before / read_after   wq_records_read_device, 1M queries at C5's entity positions, on the store
                before and after its vacuum (the views compacted before either is timed)

The store, at --scale 1: 16M rows over ~1M regions of 16 x 256 x 16 (table 1,024), then deletes of a
random half of them. A vacuumed store has nothing left to vacuum, so every repeat loads and churns a
store of its own from the same ops (untimed). --warmup untimed and --reps timed repeats per form, a
synchronise on both sides of each; min / mean / max are reported with every number. Before anything
is timed the repeat checks itself: the read after the vacuum returns the bytes of the read before
it, the imported store exports the bytes it was given, and its read equals the source's.

Byte budget, S stored and L live rows: S live bytes read and 4 S map bytes written,
60 L in and 60 L out for the move (64 L out for an export) and, for the vacuum, 12 L per view: vacuum
5 S + 144 L, export 5 S + 124 L.

    python tools/records_vacuum_bench.py [--scale 1.0] [--reps 5] [--out profiles/records_vacuum_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12  # bytes/s
CFG = (16, 256, 16, 1024)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records_vacuum_bench.json"))
    a = ap.parse_args()
    import torch
    from records_bench import ops_tensor, summary
    from worldql_server_amd import records as R, synth_ext
    from worldql_server_amd.router import Router

    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)
    n_rows = max(1024, int(16_000_000 * a.scale))
    n_q = max(64, int(1_000_000 * a.scale))
    chunk = min(n_rows, 1_000_000)
    half_xz, half_y = 2896.0 * a.scale ** (1.0 / 3.0), 1024.0
    g = torch.Generator(device=dev)
    g.manual_seed(4321)

    # the ops of every repeat: the load (one create per row) and the churn (a delete of a random half)
    pos = torch.rand((n_rows, 3), dtype=torch.float64, device=dev, generator=g) * 2.0 - 1.0
    pos[:, 0] *= half_xz
    pos[:, 1] *= half_y
    pos[:, 2] *= half_xz
    idx = torch.arange(n_rows, dtype=torch.int64, device=dev)
    creates = ops_tensor(torch, dev, R.CREATE, pos, idx, 1_000_000 + idx, idx)
    dead = torch.rand(n_rows, device=dev, generator=g) < 0.5
    kill = idx[dead]
    deletes = ops_tensor(torch, dev, R.DELETE, pos[kill], kill, 0, 0)
    survivors = creates[~dead].contiguous()  # the baseline's ops: one create per live row
    n_live = int(survivors.shape[0])
    sync()

    def batches(store, ops):
        for base in range(0, int(ops.shape[0]), chunk):
            part = ops[base:base + chunk]
            store.apply_device(part.data_ptr(), int(part.shape[0]))

    c5 = synth_ext.config_c5(scale=a.scale)
    q_pos = torch.from_numpy(np.ascontiguousarray(c5.pos[:n_q], dtype=np.float64)).to(dev)
    q_world = torch.zeros(n_q, dtype=torch.int32, device=dev)
    cap = int(min(4 * n_rows + 1024, 200_000_000))
    off = torch.zeros(n_q + 1, dtype=torch.int32, device=dev)
    hd = torch.zeros(cap, dtype=torch.int32, device=dev)
    ts_out = torch.zeros(cap, dtype=torch.int64, device=dev)
    snap = torch.zeros((n_live, 8), dtype=torch.int64, device=dev)
    sync()

    def read(store, n=n_q):
        return store.read_device(n, q_world.data_ptr(), q_pos.data_ptr(), None, False, off.data_ptr(), hd.data_ptr(),
                                 ts_out.data_ptr(), cap)

    def clock(fn):
        sync()
        t = time.perf_counter()
        x = fn()
        sync()
        return (time.perf_counter() - t) * 1e3, x

    src_router, dst_router = Router(16, 0), Router(16, 0)
    names = ("read_before", "export", "vacuum", "read_after", "import", "reapply")
    times = {k: [] for k in names}
    checks = {"read_after_equals_read_before": True, "import_exports_the_same_bytes": True,
              "read_of_imported_equals_source": True, "reapplied_live_rows": True}
    shape = {}
    for rep in range(a.warmup + a.reps):
        timed = rep >= a.warmup
        src = R.GpuRecordStore(src_router, *CFG)
        batches(src, creates)
        batches(src, deletes)
        read(src, 1)  # compacts the views: no form below pays for it
        live, stored, ops_seen = src.stats()
        if live != n_live or stored != n_rows:
            print("the churned store is not the expected one:", live, stored, flush=True)
            return 1
        t_rb, x = clock(lambda: read(src))
        if x["overflow"] or x["error"] or x["rejected"]:
            print("the read overflowed, was cut or rejected queries:", x, flush=True)
            return 1
        k = x["returned"]
        before = (off.clone(), hd[:k].clone(), ts_out[:k].clone())
        t_ex, n_ops = clock(lambda: src.export_device(snap.data_ptr(), n_live))
        t_va, v = clock(src.vacuum)
        t_ra, y = clock(lambda: read(src))
        same_read = lambda: bool(torch.equal(before[0], off) and torch.equal(before[1], hd[:k])
                                 and torch.equal(before[2], ts_out[:k]))
        checks["read_after_equals_read_before"] &= y == x and same_read()
        if n_ops != (n_live, ops_seen) or v["rows_before"] != n_rows or v["rows_after"] != n_live:
            print("export or vacuum did not report the store:", n_ops, v, flush=True)
            return 1
        src.close()
        dst = R.GpuRecordStore(dst_router, *CFG)
        t_im, imp = clock(lambda: dst.import_device(snap.data_ptr(), n_live, ops_seen))
        if imp != {"imported": n_live, "rejected": 0}:
            print("the import did not take the snapshot:", imp, flush=True)
            return 1
        if rep == 0:
            again = torch.zeros_like(snap)
            dst.export_device(again.data_ptr(), n_live)
            sync()
            checks["import_exports_the_same_bytes"] &= bool(torch.equal(again, snap))
            del again
            z = read(dst)
            sync()
            checks["read_of_imported_equals_source"] &= z == x and same_read()
        dst.close()
        base = R.GpuRecordStore(dst_router, *CFG)
        t_re, _ = clock(lambda: batches(base, survivors))
        checks["reapplied_live_rows"] &= base.stats()[:2] == (n_live, n_live)
        base.close()
        del before
        if timed:
            for name, t in zip(names, (t_rb, t_ex, t_va, t_ra, t_im, t_re)):
                times[name].append(t)
            shape = {"rows_stored": n_rows, "rows_live": n_live, "ops_seen": int(ops_seen), "vacuum": v,
                     "read": {"queries": n_q, **{k_: int(v_) for k_, v_ in x.items()}}}
    src_router.close()
    dst_router.close()
    if not all(checks.values()):
        print("a check failed:", checks, flush=True)
        return 1

    S, L = n_rows, n_live
    budget = {"vacuum": S + 4 * S + 120 * L + 2 * 12 * L, "export": S + 4 * S + 60 * L + 64 * L}
    out = {"tool": "tools/records_vacuum_bench.py", "scale": a.scale, "reps": a.reps, "warmup": a.warmup,
           "timing": "host clock, a device synchronise on both sides of every repeat",
           "budget": "S stored, L live rows: S live bytes read + 4 S map bytes written, 60 L in and 60 L out "
                     "(64 L out for the export), for the vacuum 2 x 12 L for the two views; share of 8 TB/s",
           "store": {**shape, "region_sizes": CFG[:3], "table_size": CFG[3]}, "checks": checks, "forms": {}}
    for name in names:
        ms = statistics.fmean(times[name])
        f = {"times": summary(times[name])}
        if name in budget:
            f["budget_bytes"] = budget[name]
            f["share_of_8TBs"] = round(budget[name] / (ms * 1e-3) / HBM_PEAK, 4)
        if name in ("vacuum", "export", "import", "reapply"):
            f["live_rows_per_s"] = round(L / (ms * 1e-3))
        out["forms"][name] = f
    re_ms = out["forms"]["reapply"]["times"]["mean_ms"]
    out["against_reapply"] = {k: round(re_ms / out["forms"][k]["times"]["mean_ms"], 2) for k in ("vacuum", "import")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k_: (v_["times"]["mean_ms"], v_.get("share_of_8TBs")) for k_, v_ in out["forms"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
