#!/usr/bin/env python3
"""The table export (wq_table_export*, csrc/wq_table_export.hip) on C3's and C5's built tables, in
one process, the forms alternating:

  export_device   wq_table_export_device, unfiltered, into a device buffer
  export_peers    the same with a filter of 1,000 random peers
  export_host     wq_table_export into pinned host memory
  import          wq_apply_ops_device of export_device's rows into a fresh handle (the first-batch
                  rebuild), timed to completion with a following stats() call

The tables come from the generators bench.py uses (synth_ext.config_c3 / config_c5 at --scale).
--warmup untimed and --reps timed repeats per form, a synchronise on both sides of each; min / mean /
max are reported with every number. Before anything is timed the run checks itself: the imported
handle exports the bytes it was given and reports the same stats.

Byte budget of export_device: 128 B per live record + 4 B per list word of the cubes
above 24 peers + 40 B per row, and its share of 8 TB/s.

    python tools/table_export_bench.py [--scale 1.0] [--reps 5] [--out profiles/table_export_bench.json]
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


def summary(v):
    return {"mean_ms": round(statistics.fmean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "reps_ms": [round(x, 4) for x in v]}


def run_config(name, cube_size, ops, n_peers, a, torch, dev):
    from worldql_server_amd import abi
    from worldql_server_amd.router import PinnedArray, Router

    sync = lambda: torch.cuda.synchronize(dev)

    def clock(fn):
        sync()
        t = time.perf_counter()
        x = fn()
        sync()
        return (time.perf_counter() - t) * 1e3, x

    r = Router(cube_size, 0)
    t0 = time.perf_counter()
    r.apply_ops(ops)
    build_s = time.perf_counter() - t0
    del ops
    st = r.stats()
    n = st["n_entries"]
    rows = torch.zeros((n, 5), dtype=torch.int64, device=dev)
    some = torch.zeros((n, 5), dtype=torch.int64, device=dev)
    pinned = PinnedArray((n,), abi.OP_DTYPE)
    peers = np.random.default_rng(17).choice(n_peers, min(1000, n_peers), replace=False).astype(np.uint32)
    sync()

    names = ("export_device", "export_peers", "export_host", "import")
    times = {k: [] for k in names}
    checks = {"import_exports_the_same_bytes": True, "import_stats_agree": True, "host_rows_equal_device_rows": True}
    n_some = 0
    for rep in range(a.warmup + a.reps):
        t_a, got = clock(lambda: r.export_table_device(rows.data_ptr(), n))
        if got != (0, n):
            print("the export did not return the table:", got, n, flush=True)
            return None
        t_b, got = clock(lambda: r.export_table_device(some.data_ptr(), n, peers=peers))
        n_some = got[1]
        t_c, host = clock(lambda: r.export_table(out=pinned.array))
        fresh = Router(cube_size, 0)
        sync()

        def imp():
            fresh.apply_ops_device(rows.data_ptr(), n)
            return fresh.stats()

        t_d, st2 = clock(imp)
        if rep == 0:
            checks["import_stats_agree"] &= all(st2[k] == st[k] for k in ("n_entries", "n_cubes", "n_any"))
            again = torch.zeros_like(rows)
            checks["import_exports_the_same_bytes"] &= fresh.export_table_device(again.data_ptr(), n) == (0, n)
            sync()
            checks["import_exports_the_same_bytes"] &= bool(torch.equal(again, rows))
            del again
            checks["host_rows_equal_device_rows"] &= len(host) == n and bool(
                torch.equal(torch.from_numpy(host.view(np.int64).reshape(n, 5)), rows.cpu()))
        fresh.close()
        if rep >= a.warmup:
            for k, t in zip(names, (t_a, t_b, t_c, t_d)):
                times[k].append(t)
    # the budget's terms from the rows themselves: cube boundaries, then the lists above 24 peers
    key = rows[:, [0, 2, 3, 4]].clone()
    key[:, 0] &= 0xFFFFFFFF
    first = torch.ones(n, dtype=torch.bool, device=dev)
    first[1:] = (key[1:] != key[:-1]).any(1)
    starts = first.nonzero().flatten()
    counts = torch.diff(starts, append=torch.tensor([n], device=dev))
    n_cubes = int(starts.numel())
    list_words = int((counts[counts > 24] + 1).sum())
    budget = 128 * n_cubes + 4 * list_words + 40 * n
    out = {"table": {"entries": n, "cubes": n_cubes, "stats_cubes": st["n_cubes"], "cubes_above_24_peers": int((counts > 24).sum()),
                     "list_words_above_24": list_words, "longest_list": int(counts.max()), "build_s": round(build_s, 3)},
           "checks": checks, "filtered_rows": n_some, "forms": {k: {"times": summary(times[k])} for k in names}}
    ms = out["forms"]["export_device"]["times"]["mean_ms"]
    out["forms"]["export_device"].update(budget_bytes=budget, share_of_8TBs=round(budget / (ms * 1e-3) / HBM_PEAK, 4),
                                         rows_per_s=round(n / (ms * 1e-3)))
    out["export_over_import"] = round(ms / out["forms"]["import"]["times"]["mean_ms"], 4)
    out["export_below_import"] = all(x < y for x, y in zip(times["export_device"], times["import"]))
    pinned.close()
    r.close()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default="c3,c5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_export_bench.json"))
    a = ap.parse_args()
    import torch
    from worldql_server_amd import synth_ext

    dev = torch.device("cuda:0")
    out = {"tool": "tools/table_export_bench.py", "scale": a.scale, "reps": a.reps, "warmup": a.warmup,
           "timing": "host clock, a device synchronise on both sides of every repeat; the forms alternate in one process",
           "budget": "export_device: 128 B x live records + 4 B x list words of the cubes above 24 peers + 40 B x rows; "
                     "share of 8 TB/s", "configs": {}}
    ok = True
    for name in a.configs.split(","):
        if name == "c3":
            w = synth_ext.config_c3(scale=a.scale)
            res = run_config("c3", w.cube_size, w.ops, w.n_peers, a, torch, dev)
        elif name == "c5":
            c5 = synth_ext.config_c5(scale=a.scale)
            res = run_config("c5", 16, c5.initial_ops(), c5.n, a, torch, dev)
        else:
            raise SystemExit(f"unknown config {name}")
        if res is None:
            return 1
        out["configs"][name] = res
        ok &= all(res["checks"].values())
        print(json.dumps({name: {k: v["times"]["mean_ms"] for k, v in res["forms"].items()},
                          "export_over_import": res["export_over_import"],
                          "share_of_8TBs": res["forms"]["export_device"]["share_of_8TBs"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    if not ok:
        print("a check failed", flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
