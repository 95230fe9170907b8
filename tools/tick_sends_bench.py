#!/usr/bin/env python3
"""The tick sends (wq_tick_sends_device, csrc/wq_sends.hip) against their yardsticks, in one process, the
forms alternating. The CSRs are synthetic with the shapes named below (peer ids uniform below n_peers, rows
ascending); nothing is routed.

  sends       Router.tick_sends_device on the regions: asynchronous, no read-back; the host's check and
              upload of the region table is inside the timed call;
  peer_major  Router.peer_major_device on the same CSR, where the shape is one identity region: the floor
              (a 32-bit sort by peer alone, no region search, no frame map);
  composite   torch on the same device arrays: the rows expanded with repeat_interleave from the regions'
              offsets, the frames gathered, one stable sort of (peer * n_frames + frame) as int64, a
              searchsorted for the offsets. It reads no `connected` bitmap and checks no bound.

Shapes
  a_identity    C5's tick as one identity region: 1M rows, about 1.98M pairs, 1M peers
  b_10k_regions the same rows as about 10,000 read regions of 100 rows (C5 with 1% subscribes spread evenly),
                every region's frames through a src array
  c_mix_1m      random_events' run shape at 1M frames (not 10M): about 640,000 regions of one or two rows,
                each padded to 4 pairs per row
  d_one_row     one region of 16M elements in one row
  d_1m_rows     the same 16M elements in one region of 1M rows of 16

Before anything is timed the call's kept frames and offsets are checked against the composite's. Then
--warmup untimed and --reps timed repeats per form, the forms alternating, a synchronise on both sides of
each; mean, min and max with every number. min_bytes is what the call must read and write once: 4 B per
element in, 4 B per element out, 4 B per offset and src entry, 4 B per peer offset, 44 B per region;
share_of_hbm is min_bytes over the mean time over 8 TB/s.

    python tools/tick_sends_bench.py [--scale 1.0] [--only a_identity,...] [--reps 7] [--warmup 3]
                                     [--out profiles/tick_sends_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from peer_budget_bench import summary  # noqa: E402

HBM_BYTES_PER_S = 8e12
SHAPES = ("a_identity", "b_10k_regions", "c_mix_1m", "d_one_row", "d_1m_rows")


def shape(name, scale):
    """(regions, offsets, peers, src, n_peers, n_frames) of a shape, numpy arrays."""
    from worldql_server_amd import abi
    rng = np.random.default_rng(7)
    M = max(1000, int(round(1_000_000 * scale)))
    n_peers = M
    if name in ("a_identity", "b_10k_regions"):
        lens = rng.poisson(1.98, M).astype(np.int64)
        peers = rng.integers(0, n_peers, int(lens.sum()), dtype=np.uint32)
        off = np.concatenate([[0], np.cumsum(lens)])
        if name == "a_identity":
            reg = [abi.send_region(off_at=0, peers_at=0, n_rows=M, capacity=len(peers))]
            return reg, off, peers, np.zeros(0, np.uint32), n_peers, M
        per, offs, reg = 100, [], []
        for lo in range(0, M, per):
            hi = min(lo + per, M)
            reg.append(abi.send_region(off_at=lo + len(reg), peers_at=int(off[lo]), n_rows=hi - lo,
                                       capacity=int(off[hi] - off[lo]), src_at=lo, src_sel=0))
            offs.append(off[lo:hi + 1] - off[lo])
        return reg, np.concatenate(offs), peers, np.arange(M, dtype=np.uint32), n_peers, M
    if name == "c_mix_1m":
        rows_of = rng.integers(1, 3, M)                       # regions of one or two rows until the frames run out
        rows_of = rows_of[:int(np.searchsorted(np.cumsum(rows_of), int(0.96 * M)))]
        R = int(rows_of.sum())
        lens = rng.integers(0, 4, R).astype(np.int64)
        first = np.concatenate([[0], np.cumsum(rows_of)])[:-1]
        reg, offs = [], []
        starts = np.concatenate([[0], np.cumsum(lens)])
        for g, (r0, k) in enumerate(zip(first.tolist(), rows_of.tolist())):
            o = starts[r0:r0 + k + 1] - starts[r0]
            reg.append(abi.send_region(off_at=r0 + g, peers_at=4 * r0, n_rows=k, capacity=4 * k, src_at=r0, src_sel=g % 2))
            offs.append(o)
        peers = rng.integers(0, n_peers, 4 * R, dtype=np.uint32)
        src = np.sort(rng.choice(M, R, replace=False)).astype(np.uint32)
        return reg, np.concatenate(offs), peers, src, n_peers, M
    E = 16 * M
    peers = rng.integers(0, n_peers, E, dtype=np.uint32)
    if name == "d_one_row":
        return [abi.send_region(off_at=0, peers_at=0, n_rows=1, capacity=E)], np.array([0, E]), peers, np.zeros(0, np.uint32), n_peers, 1
    return ([abi.send_region(off_at=0, peers_at=0, n_rows=M, capacity=E)], np.arange(M + 1, dtype=np.int64) * 16, peers,
            np.zeros(0, np.uint32), n_peers, M)


def run(name, a, torch, r):
    from worldql_server_amd import abi
    dev = torch.device("cuda:0")
    reg, off, peers, src, n_peers, n_frames = shape(name, a.scale)
    reg = np.array(reg, abi.SEND_REGION_DTYPE)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(dev)
    t_off, t_peers, t_src = up(off), up(peers), up(src)
    n_elems = int(reg["capacity"].astype(np.int64).sum())
    po = torch.empty(n_peers + 1, dtype=torch.int32, device=dev)
    fo = torch.empty(max(n_elems, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(64, dtype=torch.uint8, device=dev)
    sync = lambda: torch.cuda.synchronize(dev)

    def sends():
        r.tick_sends_device(reg, t_off.data_ptr(), len(off), t_peers.data_ptr(), len(peers),
                            [t_src.data_ptr() if len(src) else None] * 2, [len(src)] * 2, None, n_peers, n_frames, po.data_ptr(),
                            fo.data_ptr(), n_elems, cnt.data_ptr())

    # the composite's view of the regions, on the device once (untimed, like the call's arrays)
    rows_reg = np.repeat(np.arange(len(reg)), reg["n_rows"])
    local = np.arange(len(rows_reg)) - np.repeat(np.cumsum(reg["n_rows"].astype(np.int64)) - reg["n_rows"], reg["n_rows"])
    at = reg["off_at"].astype(np.int64)[rows_reg] + local
    t_at = torch.from_numpy(at).to(dev)
    t_start = torch.from_numpy(reg["peers_at"].astype(np.int64)[rows_reg]).to(dev)
    has_src = bool(len(src))
    t_frame_of_row = torch.from_numpy((reg["src_at"].astype(np.int64)[rows_reg] + local) if has_src else local).to(dev)

    def composite():
        o = t_off.long()
        lens = o[t_at + 1] - o[t_at]
        total = int(lens.sum().item())
        row = torch.repeat_interleave(torch.arange(lens.numel(), device=dev), lens, output_size=total)
        excl = torch.cumsum(lens, 0) - lens
        idx = (t_start + o[t_at] - excl)[row] + torch.arange(total, device=dev)
        frame = (t_src.long()[t_frame_of_row] if has_src else t_frame_of_row)[row]
        key = t_peers.long()[idx] * n_frames + frame
        skey, order = torch.sort(key, stable=True)
        offs = torch.searchsorted(skey, torch.arange(n_peers + 1, device=dev) * n_frames)
        return offs, frame[order]

    def peer_major():
        r.peer_major_device(t_off.data_ptr(), t_peers.data_ptr(), len(off) - 1, n_elems, None, n_peers, po.data_ptr(), fo.data_ptr())

    forms = {"sends": sends, "composite": composite}
    if name in ("a_identity", "d_1m_rows", "d_one_row"):
        forms["peer_major"] = peer_major
    sync()
    sends()
    sync()
    c = cnt.cpu().numpy().view(abi.TICK_SENDS_COUNTERS_DTYPE)[0]
    w_off, w_frames = composite()
    kept = int(c["n_kept"])
    assert int(c["error"]) == 0 and kept == int(w_off[-1].item()) == w_frames.numel(), (int(c["error"]), kept)
    assert torch.equal(po.long(), w_off) and torch.equal(fo[:kept].long(), w_frames), "the call and the composite differ"
    res = {"regions": len(reg), "rows": int(reg["n_rows"].astype(np.int64).sum()), "elements": n_elems, "kept": kept,
           "n_peers": n_peers, "n_frames": n_frames,
           "key_bits": max(n_peers.bit_length(), 1) + max(n_frames - 1, 0).bit_length()}
    times = {k: [] for k in forms}
    for rep in range(a.warmup + a.reps):
        for k, fn in forms.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rep >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    for k, v in times.items():
        res[k] = summary(v)
    res["min_bytes"] = 8 * n_elems + 4 * (len(off) + len(src)) + 4 * (n_peers + 1) + 44 * len(reg)
    res["share_of_hbm"] = round(res["min_bytes"] / (res["sends"]["mean_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
    for k in forms:
        if k != "sends":
            res["sends_over_" + k] = round(res["sends"]["mean_ms"] / res[k]["mean_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tick_sends_bench.json"))
    a = ap.parse_args()
    import torch
    from worldql_server_amd.router import Router
    if not torch.cuda.is_available():
        sys.exit("tick_sends_bench: no GPU (there is no CPU form of this measurement)")
    out = {"scale": a.scale, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "shapes": {}}
    r = Router(16, 0)
    for name in a.only.split(","):
        print(f"[{name}]", flush=True)
        out["shapes"][name] = run(name, a, torch, r)
        print(json.dumps({name: out["shapes"][name]}), flush=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
