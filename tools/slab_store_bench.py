#!/usr/bin/env python3
"""The record payload slab's store call (wq_slab_store_device, csrc/wq_slab.hip) against the floor of its copy and
against the per-record Python it replaces, in one process, the forms alternating:

  hip      Router.slab_store_device on ops, references and frames already in device memory, into a slab that
           is large enough, from cursor 0, with the counters, asynchronous, no read-back;
  d2d      one device-to-device copy of bytes_stored + 64 bytes per create: the floor, what a plain copy of
           the same output bytes costs;
  python   the leg it replaces, DeviceRecordProcessor.process's loop: per create one slice of the frame bytes
           per payload and one dict, on the first 1/100 of the ops, scaled by ops. A statement about
           per-record Python (the read-back of ops and references before it is not included).

Shapes (frames are random bytes, the references point into them; the call never parses a frame):
  records_1m     1M creates in 10,000 frames of 100, data 100 - 200 bytes, every fourth with a flex of 16;
  empty_1m       1M creates without payloads: the entries alone;
  flex_256x1m    256 creates with a flex of 1 MiB each, one per frame;
  one_big        one create with a flex of 64 MiB among 100,000 of 100 - 200 bytes.

hip's slab on the first 2,000 ops is checked equal to records.slab_store_np's, and a second call
byte-identical, before anything is timed. Then --warmup untimed and --reps timed repeats per form, a device
synchronise on both sides of each; min / mean / max with every number. bytes_moved is what the call must read
and write once: 96 bytes per op in, the payload bytes in and out, 64 bytes per create out.

    python tools/slab_store_bench.py [--scale 1.0] [--only records_1m,...] [--reps 7] [--warmup 3]
                                     [--out profiles/slab_store_bench.json]
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

HBM_BYTES_PER_S = 8e12


def summary(v):
    return {"mean_ms": round(statistics.fmean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "reps_ms": [round(x, 4) for x in v]}


def shape(name, scale, rng):
    """(ops, refs, frames, offsets) of a shape."""
    from worldql_server_amd import abi, records
    if name in ("records_1m", "empty_1m"):
        n, per = max(int(1_000_000 * scale) // 100 * 100, 100), 100
        dl = rng.integers(100, 201, n) if name == "records_1m" else np.zeros(n, np.int64)
        fl = np.where(np.arange(n) % 4 == 0, 16, 0) if name == "records_1m" else np.zeros(n, np.int64)
        frame = np.arange(n) // per
    elif name == "flex_256x1m":
        n = max(int(256 * scale), 2)
        dl, fl, frame = np.zeros(n, np.int64), np.full(n, 1 << 20), np.arange(n)
    else:
        n = max(int(100_000 * scale), 10) + 1
        dl, fl = rng.integers(100, 201, n), np.zeros(n, np.int64)
        dl[n // 2], fl[n // 2] = 0, max(int((64 << 20) * scale), 1 << 20)
        frame = np.arange(n) // 100
        frame[n // 2:] += 1
        frame[n // 2 + 1:] += 1
    size = dl + fl
    n_frames = int(frame[-1]) + 1
    fsize = np.bincount(frame, weights=size, minlength=n_frames).astype(np.int64) + 24
    fo = np.zeros(n_frames + 1, np.uint64)
    np.cumsum(fsize, out=fo[1:].view(np.int64))
    start = np.zeros(n, np.int64)   # where each op's data starts inside its frame: behind the ops before it
    first = np.r_[True, frame[1:] != frame[:-1]]
    run = np.cumsum(size) - size
    start = run - np.maximum.accumulate(np.where(first, run, 0)) + 24
    frames = rng.integers(0, 256, int(fo[-1]), dtype=np.uint8)
    ops = np.zeros(n, dtype=records.REC_OP_DTYPE)
    ops["kind"], ops["world"], ops["handle"] = records.CREATE, rng.integers(0, 4, n), rng.permutation(n)
    ops["pos"] = rng.uniform(-4000, 4000, (n, 3))
    ops["uuid_hi"], ops["uuid_lo"] = rng.integers(0, 1 << 62, n), rng.integers(0, 1 << 62, n)
    refs = np.zeros(n, dtype=abi.REC_OP_REF_DTYPE)
    refs["frame"], refs["record"] = frame, np.arange(n) % 100
    refs["data_off"], refs["data_len"], refs["flex_off"], refs["flex_len"] = start, dl, start + dl, fl
    refs["bits"] = (dl > 0) | 2 * (fl > 0)
    return ops, refs, frames, fo


def python_leg(ops, refs, frames, fo):
    """DeviceRecordProcessor.process's loop over the creates: slices and dicts."""
    off = [int(v) for v in fo]
    slab, cache = {}, (-1, b"")
    for op, ref in zip(ops, refs):
        if cache[0] != ref["frame"]:
            f = int(ref["frame"])
            cache = (f, frames[off[f]:off[f + 1]].tobytes())
        b = cache[1]
        slab[int(op["handle"])] = {
            "uuid": (int(op["uuid_hi"]), int(op["uuid_lo"])), "world_name": int(op["world"]),
            "position": tuple(float(c) for c in op["pos"]),
            "data": b[ref["data_off"]:ref["data_off"] + ref["data_len"]] if ref["bits"] & 1 else None,
            "flex": b[ref["flex_off"]:ref["flex_off"] + ref["flex_len"]] if ref["bits"] & 2 else None}
    return slab


def run_shape(name, a, r, rng):
    import torch
    from worldql_server_amd import abi, records
    ops, refs, frames, fo = shape(name, a.scale, rng)
    n, total = len(ops), int(refs["data_len"].sum() + refs["flex_len"].sum())
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    d_ops, d_refs, d_frames, d_fo = up(ops), up(refs), up(frames), up(fo)
    ent = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
    pay = torch.zeros(max(total, 16), dtype=torch.uint8, device=dev)
    ctrl = torch.zeros(8 + abi.SLAB_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    view = abi.SlabView(entries=ent.data_ptr(), n_entries=n, payload=pay.data_ptr(), n_payload_bytes=pay.numel())
    torch.cuda.synchronize()

    def hip(k=n):
        ctrl[:8].zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.slab_store_device(d_ops.data_ptr(), d_refs.data_ptr(), k, d_frames.data_ptr(), d_fo.data_ptr(), len(fo) - 1, view,
                            ctrl.data_ptr(), ctrl.data_ptr() + 8)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # the sample against the definition, and a second call byte-identical
    k = min(n, 2000)
    hip(k)
    got = (ent.cpu().numpy().copy(), pay.cpu().numpy().copy(), records.slab_counters(ctrl[8:].cpu().numpy()))
    w_ent, w_pay, _, w_cnt = records.slab_store_np(ops[:k], refs[:k], frames, fo, np.zeros(n, abi.SLAB_ENTRY_DTYPE),
                                                   np.zeros(pay.numel(), np.uint8), 0)
    assert got[0].tobytes() == w_ent.tobytes() and np.array_equal(got[1], w_pay) and got[2] == w_cnt, name
    hip(k)
    assert ent.cpu().numpy().tobytes() == got[0].tobytes() and np.array_equal(pay.cpu().numpy(), got[1]), name

    floor_src = torch.zeros(total + 64 * n, dtype=torch.uint8, device=dev)
    floor_dst = torch.empty_like(floor_src)

    def d2d():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        floor_dst.copy_(floor_src)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    forms = {"hip": hip, "d2d": d2d}
    times = {f: [] for f in forms}
    for i in range(a.warmup + a.reps):
        for f, fn in forms.items():
            t = fn()
            if i >= a.warmup:
                times[f].append(t)
    cnt = records.slab_counters(ctrl[8:].cpu().numpy())
    assert cnt["overflow"] == 0 and cnt["error"] == 0 and cnt["bytes_stored"] == total and cnt["n_creates"] == n, cnt
    s = max(n // 100, 1)
    t0 = time.perf_counter()
    python_leg(ops[:s], refs[:s], frames, fo)
    py_ms = (time.perf_counter() - t0) * 1e3 * n / s
    moved = 96 * n + 2 * total + 64 * n
    res = {"ops": n, "frames": len(fo) - 1, "bytes_stored": total, "bytes_moved": moved,
           "hip": summary(times["hip"]), "d2d": summary(times["d2d"]),
           "python_scaled_ms": round(py_ms, 1), "python_sample_ops": s,
           "hip_over_d2d": round(statistics.fmean(times["hip"]) / statistics.fmean(times["d2d"]), 3),
           "fraction_of_hbm": round(moved / HBM_BYTES_PER_S / (statistics.fmean(times["hip"]) * 1e-3), 4)}
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default="records_1m,empty_1m,flex_256x1m,one_big")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slab_store_bench.json"))
    ap.add_argument("--dry", action="store_true", help="build the shapes and time the Python leg only (no device)")
    a = ap.parse_args()
    rng = np.random.default_rng(11)
    if a.dry:
        from worldql_server_amd import abi, records
        for name in a.only.split(","):
            ops, refs, frames, fo = shape(name, a.scale, rng)
            k = min(len(ops), 2000)
            _, _, cur, cnt = records.slab_store_np(ops[:k], refs[:k], frames, fo, np.zeros(len(ops), abi.SLAB_ENTRY_DTYPE),
                                                   np.zeros(int(refs["data_len"].sum() + refs["flex_len"].sum()), np.uint8), 0)
            print(name, len(ops), len(fo) - 1, cnt)
        return
    import torch
    from worldql_server_amd.router import Router
    if not torch.cuda.is_available():
        raise SystemExit("slab_store_bench needs a GPU")
    r = Router(16, 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "scale": a.scale, "shapes": {}}
    for name in a.only.split(","):
        out["shapes"][name] = run_shape(name, a, r, rng)
    r.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
