#!/usr/bin/env python3
"""C5 ticks with the subscription deltas produced three ways, in one process, alternating:

  (a) device ops   the tick's ops pre-uploaded (outside every timed region), wq_apply_ops_device —
                   what `bench.py --config c5` times;
  (b) host ops     the tick's ops in a pinned (wq_host_alloc) buffer, uploaded by wq_apply_ops — what
                   a host that computes the ops itself pays (their computation is NOT timed);
  (c) follow       wq_follow_peers_device on positions already on the device: the ops are generated
                   on the GPU (csrc/wq_follow.hip).

Three routers hold the same table and see the same ticks; a tick is update + positions + radius
route. After a warm-up, `--ticks` whole ticks are timed per form (one synchronise before, one after),
then `--split` ticks with a synchronise between the update and the rest, which gives the update time
of each form and, through wq_profile_read, the generator kernels' time of (c). One JSON result under
profiles/.

    python tools/follow_bench.py [--scale 1.0] [--ticks 5] [--split 3] [--warmup 2] [--out profiles/follow_bench.json]
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--split", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "follow_bench.json"))
    a = ap.parse_args()

    import torch
    from worldql_server_amd import abi, synth_ext
    from worldql_server_amd.router import PinnedArray, Router

    dev = torch.device("cuda:0")
    c5 = synth_ext.config_c5(scale=a.scale)
    M = c5.n
    t0 = time.perf_counter()
    init = c5.initial_ops()
    init_pos = c5.pos.copy()
    n_ticks = a.warmup + a.ticks + a.split
    ticks = []
    for _ in range(n_ticks):
        ops = c5.step()
        ticks.append((ops, c5.pos.copy()))
    gen_s = time.perf_counter() - t0

    stream = torch.cuda.Stream(device=dev)
    forms = ("device_ops", "host_ops", "follow")
    R = {f: Router(16, 0) for f in forms}
    zeros_w = np.zeros(M, np.uint32)
    for f, r in R.items():
        r.set_stream(stream.cuda_stream)
        if f == "follow":
            res0 = r.follow_peers(zeros_w, init_pos)
            assert res0["n_subscribe"] == len(init) and res0["n_followed"] == M
        else:
            r.apply_ops(init)
        r.set_peer_positions(init_pos)
        r.set_radius(c5.radius)
    S0 = R["device_ops"].stats()["n_entries"]

    max_ops = max(len(t[0]) for t in ticks)
    pinned = PinnedArray((max_ops,), abi.OP_DTYPE)
    ops_d = [torch.from_numpy(np.ascontiguousarray(t[0]).view(np.uint8).copy()).to(dev) for t in ticks]
    pos_d = [torch.from_numpy(t[1]).to(dev) for t in ticks]
    world_t = torch.zeros(M, dtype=torch.int32, device=dev)
    sender_t = torch.from_numpy(np.arange(M, dtype=np.int32)).to(dev)
    repl_t = torch.zeros(M, dtype=torch.uint8, device=dev)
    cap = 80 * M + 1024
    offs = torch.empty(M + 1, dtype=torch.int32, device=dev)
    peers = torch.empty(cap, dtype=torch.int32, device=dev)
    msgs = torch.empty(cap, dtype=torch.int32, device=dev)
    cnt = {f: torch.zeros((n_ticks, 24), dtype=torch.uint8, device=dev) for f in forms}
    follow_ops = []
    torch.cuda.synchronize(dev)

    def update(f, i):
        r = R[f]
        if f == "device_ops":
            r.apply_ops_device(ops_d[i].data_ptr(), len(ticks[i][0]))
        elif f == "host_ops":
            r._check(r.lib.wq_apply_ops(r.h, pinned.ptr, len(ticks[i][0])))
        else:
            res = r.follow_peers_device(world_t.data_ptr(), pos_d[i].data_ptr(), M)
            follow_ops.append(res["n_unsubscribe"] + res["n_subscribe"])

    def rest(f, i):
        r = R[f]
        r.set_peer_positions_device(pos_d[i].data_ptr(), M)
        r.route_device(pos_d[i].data_ptr(), world_t.data_ptr(), sender_t.data_ptr(), repl_t.data_ptr(), M,
                       offs.data_ptr(), peers.data_ptr(), msgs.data_ptr(), cap, cnt[f][i].data_ptr())

    tick_ms = {f: [] for f in forms}
    upd_ms = {f: [] for f in forms}
    rest_ms = {f: [] for f in forms}
    gen_kernel_ms, gen_ops = [], []
    for i in range(n_ticks):
        pinned.array[: len(ticks[i][0])] = ticks[i][0]  # (b)'s host-side op production: not timed
        split = i >= a.warmup + a.ticks
        for f in forms:
            r = R[f]
            torch.cuda.synchronize(dev)
            if not split:
                t0 = time.perf_counter()
                update(f, i)
                rest(f, i)
                torch.cuda.synchronize(dev)
                if i >= a.warmup:
                    tick_ms[f].append((time.perf_counter() - t0) * 1e3)
                continue
            if f == "follow":
                r.profile_enable(True)
            t0 = time.perf_counter()
            update(f, i)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            if f == "follow":
                k_ms, _ = r.profile_read()  # the count + scan and the emit intervals of this call
                r.profile_enable(False)
                gen_kernel_ms.append(k_ms)
                gen_ops.append(follow_ops[-1])
            t1b = time.perf_counter()
            rest(f, i)
            torch.cuda.synchronize(dev)
            upd_ms[f].append((t1 - t0) * 1e3)
            rest_ms[f].append((time.perf_counter() - t1b) * 1e3)

    # correctness at full size: the three tables agree, every tick routed the same pairs, no error
    stats = {f: R[f].stats() for f in forms}
    counters = {f: cnt[f].cpu().numpy().reshape(-1).view(abi.COUNTERS_DTYPE) for f in forms}
    for f in forms:
        c = counters[f]
        assert (c["overflow"] == 0).all() and (c["error"] == 0).all(), f
        assert (c["n_pairs"] == counters["device_ops"]["n_pairs"]).all(), f
        assert R[f].route_health() == (0, 0), f
    tables_equal = all(stats[f]["n_entries"] == stats["device_ops"]["n_entries"] and
                       stats[f]["n_cubes"] == stats["device_ops"]["n_cubes"] for f in forms)
    upd = {f: R[f].update_counts() for f in forms}

    def summary(v):
        return {"mean_ms": round(statistics.fmean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "ticks_ms": [round(x, 4) for x in v]} if v else None

    mean = {f: statistics.fmean(tick_ms[f]) for f in forms}
    spread_b = max(tick_ms["host_ops"]) - min(tick_ms["host_ops"])
    ops_tick = [len(t[0]) for t in ticks[a.warmup:]]
    out = {
        "tool": "tools/follow_bench.py", "config": "C5", "scale": a.scale, "entities": M, "subscriptions": int(S0),
        "warmup": a.warmup, "ticks": a.ticks, "split_ticks": a.split, "host_generate_s": round(gen_s, 1),
        "ops_per_tick": int(statistics.fmean(ops_tick)), "op_bytes_per_tick": int(40 * statistics.fmean(ops_tick)),
        "follow_ops_per_tick": int(statistics.fmean(follow_ops[a.warmup:])),
        "follow_ops_equal_generator": follow_ops == [len(t[0]) for t in ticks],
        "tick": {f: summary(tick_ms[f]) for f in forms},
        "split": {f: {"update": summary(upd_ms[f]), "positions_route": summary(rest_ms[f])} for f in forms},
        "incremental_batches_fallbacks": {f: list(upd[f]) for f in forms},
        "tables_equal": bool(tables_equal),
        "final_table": {f: {"n_entries": stats[f]["n_entries"], "n_cubes": stats[f]["n_cubes"]} for f in forms},
    }
    if gen_kernel_ms:
        g = statistics.fmean(gen_kernel_ms)
        nbytes = statistics.fmean([56 * M + 40 * k + 28 * M for k in gen_ops])
        ua, uc = statistics.fmean(upd_ms["device_ops"]), statistics.fmean(upd_ms["follow"])
        out["generator"] = {
            "kernels_ms": round(g, 4), "kernels_ticks_ms": [round(x, 4) for x in gen_kernel_ms],
            "budget_bytes": int(nbytes), "achieved_bytes_per_s": round(nbytes / (g / 1e3), 0),
            "peak_bytes_per_s": HBM_PEAK, "frac_of_peak": round(nbytes / (g / 1e3) / HBM_PEAK, 4),
            "what": "count + scan and emit (events around the launches); budget = 56 B read and 28 B written per "
                    "peer, 40 B written per op",
        }
        out["bars"] = {
            "follow_vs_host_ops": {"host_minus_follow_ms": round(mean["host_ops"] - mean["follow"], 4),
                                   "host_ops_spread_ms": round(spread_b, 4),
                                   "pass": bool(mean["host_ops"] - mean["follow"] > spread_b)},
            "follow_vs_device_ops": {"tick_extra_ms": round(mean["follow"] - mean["device_ops"], 4),
                                     "update_extra_ms": round(uc - ua, 4), "device_ops_update_ms": round(ua, 4),
                                     "within_quarter_of_update": bool(uc - ua <= ua / 4)},
        }
    for r in R.values():
        r.close()
    pinned.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0 if tables_equal else 1


if __name__ == "__main__":
    sys.exit(main())
