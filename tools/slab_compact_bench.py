#!/usr/bin/env python3
"""The slab's compaction (wq_slab_compact_device, csrc/wq_slab_compact.hip) against the floor of its copy, against
the other ways to fill an arena and against per-record Python, in one process, the forms alternating:

  hip      Router.slab_compact_device from a source slab in device memory into a destination that is exactly
           large enough, with the counters, asynchronous, no read-back;
  d2d      one device-to-device copy of the bytes the call writes, the live payload plus 64 bytes per
           destination entry: the floor;
  store    wq_slab_store_device of the same live records from frames (the live payloads back to back, 100
           records a frame) into an empty slab: today's other way to fill an arena;
  torch    a composite on the same device arrays: masks, cumsum, a byte gather by repeat_interleave;
  python   per record DeviceRecordSlab.get and put_host into a second slab, on the first 1/100 of the live
           entries, scaled by the live entries.

Shapes (payloads are random bytes; the source arena holds them in a random handle order, dead ones included;
--arena handle lays them out in ascending handle order instead, which separates the cost of the gather):
  half_dead_1m     1M entries of 100 - 200 bytes, every fourth with a 16-byte flex, half of them dead at random;
  none_dead_1m     the same, nothing dead;
  dead99_1m        the same, 99% dead;
  big_256x1m       256 live entries of 1 MiB;
  one_big          one 64 MiB payload among 100,000 small ones;
  one_big_spread   the same bytes spread evenly over the same number of entries;
  dead_run         100,000 live small entries whose handles surround one run of 1M dead handles;
  dead_run_dense   the same entries with dense handles.

hip's result on the first 2,000 source entries is checked equal to records.slab_compact_np's, and a second call
byte-identical, before anything is timed. Then --warmup untimed and --reps timed repeats per form, a device
synchronise on both sides of each; min / mean / max with every number.

    python tools/slab_compact_bench.py [--scale 1.0] [--only half_dead_1m,...] [--reps 7] [--warmup 3]
                                       [--arena random|handle] [--out profiles/slab_compact_bench.json]
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

SHAPES = "half_dead_1m,none_dead_1m,dead99_1m,big_256x1m,one_big,one_big_spread,dead_run,dead_run_dense"
PAIRS = (("one_big", "one_big_spread"), ("dead_run", "dead_run_dense"))


def summary(v):
    return {"mean_ms": round(statistics.fmean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "reps_ms": [round(x, 4) for x in v]}


def shape(name, scale, rng, arena="random"):
    """(entries, payload) of a shape's source slab; arena: the payloads' order in the source arena, a random
    permutation of the handles or ("handle") ascending handles."""
    from worldql_server_amd import abi
    small = lambda n: (rng.integers(100, 201, n), np.where(np.arange(n) % 4 == 0, 16, 0))   # noqa: E731
    if name in ("half_dead_1m", "none_dead_1m", "dead99_1m"):
        n = max(int(1_000_000 * scale), 100)
        dl, fl = small(n)
        live = rng.random(n) >= {"half_dead_1m": 0.5, "none_dead_1m": 0.0, "dead99_1m": 0.99}[name]
    elif name == "big_256x1m":
        n = max(int(256 * scale), 2)
        dl, fl, live = np.zeros(n, np.int64), np.full(n, 1 << 20), np.ones(n, bool)
    elif name in ("one_big", "one_big_spread"):
        n = max(int(100_000 * scale), 10) + 1
        dl, fl = small(n)
        big = max(int((64 << 20) * scale), 1 << 20)
        dl[n // 2], fl[n // 2] = 0, big
        if name == "one_big_spread":
            total = int(dl.sum() + fl.sum())
            dl, fl = np.full(n, total // n), np.zeros(n, np.int64)
            dl[:total - int(dl.sum())] += 1
        live = np.ones(n, bool)
    else:
        k = max(int(100_000 * scale), 10)
        run = max(int(1_000_000 * scale), 100) if name == "dead_run" else 0
        n = k + run
        live = np.ones(n, bool)
        live[k // 2:k // 2 + run] = False
        dl, fl = small(n)
        dl[~live], fl[~live] = 0, 0       # the dead run holds no bytes: both shapes read the same arena
    order = rng.permutation(n) if arena == "random" else np.arange(n)
    size = (dl + fl).astype(np.int64)
    start = np.zeros(n, np.int64)
    start[order] = np.cumsum(size[order]) - size[order]
    ent = np.zeros(n, abi.SLAB_ENTRY_DTYPE)
    ent["uuid"] = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    ent["pos"] = rng.uniform(-4000, 4000, (n, 3))
    ent["world"] = rng.integers(0, 4, n)
    ent["bits"] = ((dl > 0) * abi.SLAB_DATA | (fl > 0) * abi.SLAB_FLEX | abi.SLAB_POSITION | np.where(live, abi.SLAB_LIVE, 0)).astype(np.uint32)
    ent["off"], ent["data_len"], ent["flex_len"] = start, dl, fl
    return ent, rng.integers(0, 256, int(size.sum()), dtype=np.uint8)


def canonical(ent, payload):
    """(offsets of the live entries in handle order, the live payloads back to back), vectorized."""
    from worldql_server_amd import abi
    live = np.flatnonzero(ent["bits"] & np.uint32(abi.SLAB_LIVE))
    size = ent["data_len"][live].astype(np.int64) + ent["flex_len"][live]
    to = np.cumsum(size) - size
    idx = np.repeat(ent["off"][live].astype(np.int64) - to, size) + np.arange(int(size.sum()))
    return live, to, size, payload[idx]


def store_inputs(ent, live, to, size, canon):
    """The live records as creates whose payloads lie in frames of 100 records: the canonical bytes."""
    from worldql_server_amd import abi, records
    n = len(live)
    frame = np.arange(n) // 100
    fo = np.r_[to[::100], int(size.sum())].astype(np.uint64)
    ops = np.zeros(n, dtype=records.REC_OP_DTYPE)
    ops["kind"], ops["world"], ops["handle"], ops["pos"] = records.CREATE, ent["world"][live], live, ent["pos"][live]
    u = ent["uuid"][live].astype(np.uint64)
    w = (np.uint64(1) << (np.uint64(8) * np.arange(7, -1, -1, dtype=np.uint64)))
    ops["uuid_hi"], ops["uuid_lo"] = (u[:, :8] * w).sum(1, dtype=np.uint64), (u[:, 8:] * w).sum(1, dtype=np.uint64)
    refs = np.zeros(n, dtype=abi.REC_OP_REF_DTYPE)
    refs["frame"], refs["record"] = frame, np.arange(n) % 100
    start = to - fo[frame].astype(np.int64)
    refs["data_off"], refs["data_len"] = start, ent["data_len"][live]
    refs["flex_off"], refs["flex_len"] = start + ent["data_len"][live], ent["flex_len"][live]
    refs["bits"] = ent["bits"][live] & 3
    return ops, refs, canon, fo


def run_shape(name, a, r, rng):
    import torch
    from worldql_server_amd import abi, records
    ent, payload = shape(name, a.scale, rng, a.arena)
    live, to, size, canon = canonical(ent, payload)
    n, n_live, total = len(ent), len(live), int(size.sum())
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    s_ent, s_pay = up(ent), up(payload if len(payload) else np.zeros(16, np.uint8))
    d_ent = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
    d_pay = torch.zeros(max(total, 16), dtype=torch.uint8, device=dev)
    ctrl = torch.zeros(8 + abi.SLAB_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    src = abi.SlabView(entries=s_ent.data_ptr(), n_entries=n, payload=s_pay.data_ptr(), n_payload_bytes=len(payload))
    dst = abi.SlabView(entries=d_ent.data_ptr(), n_entries=n, payload=d_pay.data_ptr(), n_payload_bytes=d_pay.numel())
    torch.cuda.synchronize()

    def hip(view=src):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.slab_compact_device(view, dst, ctrl.data_ptr(), ctrl.data_ptr() + 8)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # a prefix against the definition, and a second call byte-identical
    k = min(n, 2000)
    prefix = abi.SlabView(entries=s_ent.data_ptr(), n_entries=k, payload=s_pay.data_ptr(), n_payload_bytes=len(payload))
    hip(prefix)
    csize = abi.SLAB_COMPACT_COUNTERS_DTYPE.itemsize
    got = (d_ent.cpu().numpy().copy(), d_pay.cpu().numpy().copy(), records.slab_compact_counters(ctrl[8:8 + csize].cpu().numpy()))
    w_ent, w_pay, w_cur, w_cnt = records.slab_compact_np(ent[:k], payload, n, d_pay.numel())
    assert got[0].tobytes() == w_ent.tobytes() and np.array_equal(got[1][:w_cur], w_pay[:w_cur]) and got[2] == w_cnt, name
    hip(prefix)
    assert d_ent.cpu().numpy().tobytes() == got[0].tobytes() and np.array_equal(d_pay.cpu().numpy(), got[1]), name

    floor_src = torch.zeros(total + 64 * n, dtype=torch.uint8, device=dev)
    floor_dst = torch.empty_like(floor_src)

    def d2d():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        floor_dst.copy_(floor_src)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ops, refs, frames, fo = store_inputs(ent, live, to, size, canon)
    st = [up(x) for x in (ops, refs, frames if len(frames) else np.zeros(16, np.uint8), fo)]
    st_ent = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
    st_pay = torch.zeros(max(total, 16), dtype=torch.uint8, device=dev)
    st_ctrl = torch.zeros(8 + abi.SLAB_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    st_view = abi.SlabView(entries=st_ent.data_ptr(), n_entries=n, payload=st_pay.data_ptr(), n_payload_bytes=st_pay.numel())

    def store():
        st_ctrl[:8].zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.slab_store_device(st[0].data_ptr(), st[1].data_ptr(), n_live, st[2].data_ptr(), st[3].data_ptr(), len(fo) - 1, st_view,
                            st_ctrl.data_ptr(), st_ctrl.data_ptr() + 8)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    e64 = s_ent.view(torch.int64).view(n, 8)
    t_out = {}

    def torch_form():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        alive = e64[:, 5] < 0                                  # bit 31 of `bits` is the word's sign
        w7 = e64[:, 7]
        sz = torch.where(alive, (w7 & 0xFFFFFFFF) + ((w7 >> 32) & 0xFFFFFFFF), torch.zeros_like(w7))
        at = torch.cumsum(sz, 0) - sz
        new = torch.where(alive[:, None], e64, torch.zeros_like(e64))
        new[:, 6] = torch.where(alive, at, torch.zeros_like(at))
        idx = torch.repeat_interleave(e64[:, 6] - at, sz) + torch.arange(total, device=dev)
        t_out["ent"], t_out["pay"] = new, s_pay[idx]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    forms = {"hip": hip, "d2d": d2d, "store": store, "torch": torch_form}
    times = {f: [] for f in forms}
    for i in range(a.warmup + a.reps):
        for f, fn in forms.items():
            t = fn()
            if i >= a.warmup:
                times[f].append(t)
    cnt = records.slab_compact_counters(ctrl[8:8 + csize].cpu().numpy())
    assert cnt == dict(n_entries=n, n_live=n_live, bytes_live=total, entries_need=int(live[-1]) + 1, overflow=0, error=0), cnt
    # the three ways agree: the arena is the canonical bytes, the entries equal
    assert np.array_equal(d_pay[:total].cpu().numpy(), canon) and np.array_equal(t_out["pay"].cpu().numpy(), canon), name
    assert np.array_equal(st_pay[:total].cpu().numpy(), canon), name
    assert d_ent.cpu().numpy().tobytes() == t_out["ent"].cpu().numpy().tobytes() == st_ent.cpu().numpy().tobytes(), name

    # per-record Python: get from one slab, put_host into another
    s = max(n_live // 100, 1)
    a_slab = records.DeviceRecordSlab(r, dev, n_entries=n, n_payload_bytes=max(total, 16))
    a_slab.load(ent, payload)
    b_slab = records.DeviceRecordSlab(r, dev, n_entries=n, n_payload_bytes=max(total, 16))
    t0 = time.perf_counter()
    for hd in live[:s]:
        rec = a_slab.get(int(hd), raw_data=True)
        rec["data"], rec["flex"] = None, (rec["data"] or b"") + (rec["flex"] or b"")   # random bytes are no text
        b_slab.put_host(int(hd), rec, rec["world"])
    py_ms = (time.perf_counter() - t0) * 1e3 * n_live / s
    mean = {f: statistics.fmean(times[f]) for f in forms}
    res = {"entries": n, "live": n_live, "bytes_live": total, "bytes_written": total + 64 * n,
           **{f: summary(times[f]) for f in forms}, "python_scaled_ms": round(py_ms, 1), "python_sample_entries": s,
           "hip_over_d2d": round(mean["hip"] / mean["d2d"], 3), "hip_over_store": round(mean["hip"] / mean["store"], 3),
           "torch_over_hip": round(mean["torch"] / mean["hip"], 3), "python_over_hip": round(py_ms / mean["hip"], 1)}
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default=SHAPES)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slab_compact_bench.json"))
    ap.add_argument("--arena", choices=("random", "handle"), default="random",
                    help="the payloads' order in the source arena: a random permutation of the handles, or ascending handles")
    ap.add_argument("--dry", action="store_true", help="build the shapes and check the host arithmetic only (no device)")
    a = ap.parse_args()
    rng = np.random.default_rng(13)
    if a.dry:
        from worldql_server_amd import abi, records
        for name in a.only.split(","):
            ent, payload = shape(name, a.scale, rng, a.arena)
            live, to, size, canon = canonical(ent, payload)
            k = min(len(ent), 2000)
            w_ent, w_pay, cur, cnt = records.slab_compact_np(ent[:k], payload, k, int(size.sum()))
            assert np.array_equal(w_pay[:cur], canon[:cur]) and np.array_equal(w_ent["off"][live[live < k]], to[live < k])
            ops, refs, frames, fo = store_inputs(ent, live, to, size, canon)
            j = min(len(ops), 500)
            s_ent, s_pay, s_cur, s_cnt = records.slab_store_np(ops[:j], refs[:j], frames, fo, np.zeros(len(ent), abi.SLAB_ENTRY_DTYPE),
                                                               np.zeros(int(size.sum()), np.uint8), 0)
            assert s_cnt["error"] == 0 and np.array_equal(s_pay[:s_cur], canon[:s_cur])
            full = records.slab_compact_np(ent[:int(live[j - 1]) + 1], payload, len(ent), int(size.sum()))
            assert full[0].tobytes() == s_ent.tobytes()
            print(name, len(ent), len(live), int(size.sum()), cnt)
        return
    import torch
    from worldql_server_amd.router import Router
    if not torch.cuda.is_available():
        raise SystemExit("slab_compact_bench needs a GPU")
    r = Router(16, 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "scale": a.scale, "arena": a.arena, "shapes": {}}
    for name in a.only.split(","):
        out["shapes"][name] = run_shape(name, a, r, rng)
    out["pairs"] = {}
    for one, spread in PAIRS:
        if one in out["shapes"] and spread in out["shapes"]:
            out["pairs"][f"{one}_over_{spread}"] = round(out["shapes"][one]["hip"]["mean_ms"] / out["shapes"][spread]["hip"]["mean_ms"], 3)
    r.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
