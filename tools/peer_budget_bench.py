#!/usr/bin/env python3
"""The send budgets (wq_peer_budget_device, csrc/wq_budget.hip) against a torch composite on the same
device arrays, in one process, the forms alternating:

  hip        Router.peer_budget_device: rows / keys / radix select / flags / scans / emit, asynchronous,
             no read-back;
  composite  the key of every element (two gathers and the f64 expression, op by op), a stable sort by
             key, a stable sort of that order by peer, rank in row from the sorted position, the mask
             rank < B scattered back so the kept elements come out in input order, offsets from the
             per-row minimum of budget and length.

Shapes, at full size with --scale 1:
  i    C5: one radius tick of 1M entities, wq_peer_major_device, then K = 32
  ii   C3: one tick of 10M messages transposed (about 417M pairs), K = 256
  iii  P elements in one row among 1M empty rows, against the same P spread evenly over the rows,
       both with K = P / 2 (the skew line), and the spread rows again with K = half a row

Every form's outputs are checked equal to each other (and to interest.peer_budget_np where the
elements fit --host-check-elements) before anything is timed. Then --warmup untimed and --reps timed
repeats per form, a synchronise on both sides of each; min / mean / max are reported with every
number.

    python tools/peer_budget_bench.py [--scale 1.0] [--only i,ii,iii] [--forms hip,composite] [--reps 7] [--append]
                                      [--out profiles/peer_budget_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes/s


def summary(v):
    return {"mean_ms": round(statistics.fmean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "reps_ms": [round(x, 4) for x in v]}


class Bench:
    def __init__(self, a):
        import torch
        from worldql_server_amd import abi, interest
        self.torch, self.abi, self.interest, self.a = torch, abi, interest, a
        self.dev = torch.device("cuda:0")
        self.forms = a.forms.split(",")

    def i32(self, n):
        return self.torch.empty(max(int(n), 1), dtype=self.torch.int32, device=self.dev)

    def dev_u32(self, x):
        return self.torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(self.dev)

    def host_u32(self, t, n=None):
        t = t if n is None else t[:n]
        return t.cpu().numpy().view(np.uint32)

    def sync(self):
        self.torch.cuda.synchronize(self.dev)

    def timed(self, fn, reps):
        out = []
        for _ in range(reps):
            self.sync()
            t0 = time.perf_counter()
            fn()
            self.sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def tick_transposed(self, r, pos, world, sender, repl, M, n_peers, cap):
        """One tick on device arrays, grown until it fits, then wq_peer_major_device:
        (peer_offsets, rows[:P], P)."""
        cnt = self.torch.zeros(24, dtype=self.torch.uint8, device=self.dev)
        while True:
            offs, peers = self.i32(M + 1), self.i32(cap)
            self.sync()
            r.route_device(pos.data_ptr(), world.data_ptr(), sender.data_ptr(), repl.data_ptr(), M, offs.data_ptr(),
                           peers.data_ptr(), None, cap, cnt.data_ptr())
            self.sync()
            c = cnt.cpu().numpy().view(self.abi.COUNTERS_DTYPE)[0]
            assert c["error"] == 0, int(c["error"])
            if not c["overflow"]:
                break
            r.route_health()
            cap = int(c["n_pairs"]) + 1024
        P = int(c["n_pairs"])
        po, rows = self.i32(n_peers + 1), self.i32(P)
        r.peer_major_device(offs.data_ptr(), peers.data_ptr(), M, P, None, n_peers, po.data_ptr(), rows.data_ptr())
        self.sync()
        del offs, peers
        self.torch.cuda.empty_cache()
        return po, rows[:P], P

    def composite(self, po, msgs, n, mpos, ppos, k):
        """The torch baseline; int32 tensors holding u32 bits (values below 2^31). Returns (offsets, kept)."""
        torch = self.torch
        n_peers = po.numel() - 1
        lens = (po[1:] - po[:-1]).long()
        out_off = torch.zeros(n_peers + 1, dtype=torch.int32, device=self.dev)
        torch.cumsum(lens.clamp(max=k), 0, dtype=torch.int32, out=out_off[1:])
        if n == 0:
            return out_off, msgs[:0]
        row = torch.repeat_interleave(torch.arange(n_peers, device=self.dev), lens, output_size=n)
        d = mpos[msgs[:n].long()] - ppos[row]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        d2 = torch.where(torch.isnan(d2), torch.full_like(d2, float("inf")), d2)
        by_key = torch.argsort(d2, stable=True)
        order = by_key[torch.argsort(row[by_key], stable=True)]
        rank = torch.arange(n, device=self.dev) - po.long()[row[order]]
        keep = torch.zeros(n, dtype=torch.bool, device=self.dev)
        keep[order[rank < k]] = True
        return out_off, msgs[:n][keep]

    def run(self, r, name, po, msgs, n, mpos, ppos, k, composite_ok=True):
        """po[n_peers + 1], msgs[n] (int32 device tensors), mpos / ppos f64 [*, 3]. The shape's result."""
        torch, abi = self.torch, self.abi
        n_peers = po.numel() - 1
        oo, om = self.i32(n_peers + 1), self.i32(n)
        cnt = torch.zeros(24, dtype=torch.uint8, device=self.dev)

        def hip():
            r.peer_budget_device(po.data_ptr(), msgs.data_ptr() if n else None, n_peers, n, mpos.data_ptr(),
                                 mpos.shape[0], ppos.data_ptr(), ppos.shape[0], k, None, oo.data_ptr(),
                                 om.data_ptr() if n else None, cnt.data_ptr())

        self.sync()
        hip()
        self.sync()
        c = cnt.cpu().numpy().view(abi.BUDGET_COUNTERS_DTYPE)[0]
        assert c["error"] == 0 and int(c["n_in"]) == n, (int(c["error"]), int(c["n_in"]), n)
        kept = int(c["n_kept"])
        res = {"peers": n_peers, "elements": n, "k": k, "kept": kept, "rows_cut": int(c["rows_cut"]),
               "longest_row": int((po[1:] - po[:-1]).max().item()) if n_peers else 0}
        checks = {}
        with_composite = "composite" in self.forms and composite_ok
        if with_composite:
            t_oo, t_om = self.composite(po, msgs, n, mpos, ppos, k)
            checks["hip_equals_composite"] = bool(len(t_om) == kept and torch.equal(t_oo, oo)
                                                  and torch.equal(t_om, om[:kept]))
            del t_oo, t_om
        elif "composite" in self.forms:
            res["composite"] = "not measured at this size (see composite_scale)"
        if n <= self.a.host_check_elements:
            w_oo, w_om, w_cnt = self.interest.peer_budget_np(self.host_u32(po), self.host_u32(msgs, n),
                                                             mpos.cpu().numpy(), ppos.cpu().numpy(), k=k)
            checks["hip_equals_peer_budget_np"] = bool(self.host_u32(oo).tobytes() == w_oo.tobytes()
                                                       and self.host_u32(om, kept).tobytes() == w_om.tobytes())
        first = (oo.clone(), om[:kept].clone())
        hip()
        self.sync()
        checks["hip_deterministic"] = bool(torch.equal(first[0], oo) and torch.equal(first[1], om[:kept]))
        del first
        res["checks"] = checks
        assert all(checks.values()), checks
        fns = {"hip": hip}
        if with_composite:
            fns["composite"] = lambda: self.composite(po, msgs, n, mpos, ppos, k)
        for fn in fns.values():
            for _ in range(self.a.warmup):
                fn()
        times = {f: [] for f in fns}
        for _ in range(self.a.reps):  # alternating
            for f, fn in fns.items():
                times[f] += self.timed(fn, 1)
        res["times"] = {f: summary(v) for f, v in times.items()}
        # what the call must move: the list, two 24-byte position gathers per element, the offsets in
        # and out, the kept list
        nbytes = 4 * n + 48 * n + 8 * (n_peers + 1) + 4 * kept
        res["must_move_bytes"] = nbytes
        res["hip_frac_of_8TBps"] = round(nbytes / (statistics.fmean(times["hip"]) / 1e3) / HBM_PEAK, 4)
        if "composite" in times:
            res["composite_over_hip"] = round(statistics.fmean(times["composite"]) / statistics.fmean(times["hip"]), 3)
        print(f"[{name}] " + json.dumps(res), flush=True)
        torch.cuda.empty_cache()
        return res

    # ---- shapes ----
    def shape_i(self):
        from worldql_server_amd import synth_ext
        from worldql_server_amd.router import Router
        torch = self.torch
        c5 = synth_ext.config_c5(scale=self.a.scale)
        M = c5.n
        r = Router(16, 0)
        r.set_radius(c5.radius)
        pos = torch.from_numpy(c5.pos.copy()).to(self.dev)
        world = torch.zeros(M, dtype=torch.int32, device=self.dev)
        sender = torch.from_numpy(np.arange(M, dtype=np.int32)).to(self.dev)
        repl = torch.zeros(M, dtype=torch.uint8, device=self.dev)
        self.sync()
        r.follow_peers_device(world.data_ptr(), pos.data_ptr(), M)
        r.set_peer_positions_device(pos.data_ptr(), M)
        po, rows, P = self.tick_transposed(r, pos, world, sender, repl, M, M, 16 * M + 1024)
        out = {"k32": self.run(r, "i_k32", po, rows, P, pos, pos, 32),
               "k1": self.run(r, "i_k1", po, rows, P, pos, pos, 1)}   # K = 32 cuts no C5 row; K = 1 does
        r.close()
        return out

    def shape_ii(self):
        from worldql_server_amd import synth, synth_ext
        from worldql_server_amd.router import Router
        torch = self.torch

        def at(s, composite_ok):
            n_peers = max(1, int(round(1_000_000 * s)))
            M = max(1, int(round(10_000_000 * s)))
            print(f"[ii] building the C3 table and tick at scale {s}", flush=True)
            half, sig = 4096.0 * (s ** (1.0 / 3.0)), 128.0 * (s ** (1.0 / 3.0))
            peer_pos = synth_ext.hotspot_positions(3, 1, n_peers, half, 256, sig)
            r = Router(16, 0)
            r.follow_peers(np.zeros(n_peers, np.uint32), peer_pos)  # the C3 table: every peer's 3x3x3
            pos = torch.from_numpy(synth_ext.hotspot_positions(3, 2, M, half, 256, sig)).to(self.dev)
            sender = self.dev_u32(synth.stream(3, 3).below(n_peers, M))
            world = torch.zeros(M, dtype=torch.int32, device=self.dev)
            repl = torch.zeros(M, dtype=torch.uint8, device=self.dev)
            ppos = torch.from_numpy(peer_pos).to(self.dev)
            self.sync()
            po, rows, P = self.tick_transposed(r, pos, world, sender, repl, M, n_peers, 48 * M + 1024)
            print(f"[ii] {P} pairs transposed", flush=True)
            res = self.run(r, f"ii_scale_{s}", po, rows, P, pos, ppos, 256, composite_ok)
            res["scale"] = s
            r.close()
            return res

        cs = min(self.a.scale, self.a.composite_scale)
        out = {"full": at(self.a.scale, cs >= self.a.scale)}
        if cs < self.a.scale:   # the composite's buffers do not fit at full size: both forms at the largest that do
            out["composite_scale"] = at(cs, True)
        return out

    def shape_iii(self):
        from worldql_server_amd.router import Router
        torch = self.torch
        n_rows = max(2, int(round(1_000_000 * self.a.scale))) + 1
        per = 16
        P = per * (n_rows - 1)
        rng = np.random.default_rng(5)
        n_msgs = n_rows
        mpos = torch.from_numpy(rng.uniform(-1024.0, 1024.0, (n_msgs, 3))).to(self.dev)
        ppos = torch.from_numpy(rng.uniform(-1024.0, 1024.0, (n_rows, 3))).to(self.dev)
        msgs = self.dev_u32(rng.integers(0, n_msgs, size=P))
        one = np.zeros(n_rows + 1, np.uint32)
        one[n_rows // 2 + 1:] = P                                  # all of it in row n_rows / 2
        even = np.zeros(n_rows + 1, np.uint32)
        even[1:n_rows] = per * np.arange(1, n_rows, dtype=np.uint32)   # 16 per row, the last row empty
        even[n_rows] = P
        r = Router(16, 0)
        d_one, d_even = self.dev_u32(one), self.dev_u32(even)
        self.sync()
        res_one = self.run(r, "iii_one_row", d_one, msgs, P, mpos, ppos, P // 2)
        res_even = self.run(r, "iii_spread", d_even, msgs, P, mpos, ppos, P // 2)
        res_cut = self.run(r, "iii_spread_half_rows", d_even, msgs, P, mpos, ppos, per // 2)
        r.close()
        ratio = res_one["times"]["hip"]["mean_ms"] / res_even["times"]["hip"]["mean_ms"]
        ratio_cut = res_one["times"]["hip"]["mean_ms"] / res_cut["times"]["hip"]["mean_ms"]
        return {"one_row": res_one, "spread": res_even, "spread_half_rows": res_cut,
                "hip_one_row_over_spread": round(ratio, 3), "hip_one_row_over_spread_half_rows": round(ratio_cut, 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--composite-scale", type=float, default=1.0,
                    help="shape ii: the largest scale at which the composite's buffers fit")
    ap.add_argument("--only", default="i,ii,iii")
    ap.add_argument("--forms", default="hip,composite")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-check-elements", type=int, default=3_000_000)
    ap.add_argument("--append", action="store_true", help="keep the shapes an earlier run wrote to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peer_budget_bench.json"))
    a = ap.parse_args()
    b = Bench(a)
    only = a.only.split(",")
    out = {"tool": "tools/peer_budget_bench.py", "scale": a.scale, "composite_scale": a.composite_scale,
           "reps": a.reps, "warmup": a.warmup, "forms": b.forms,
           "timing": "host clock, a device synchronise on both sides of every repeat",
           "must_move": "reads 4 n (the list) + 48 n (two position gathers) + 4 (n_peers + 1), writes "
                        "4 (n_peers + 1) + 4 kept bytes; share of 8 TB/s",
           "shapes": {}}
    if a.append and os.path.exists(a.out):
        with open(a.out) as fh:
            out["shapes"] = json.load(fh).get("shapes", {})
    ok = True

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    for name, fn in (("i", b.shape_i), ("ii", b.shape_ii), ("iii", b.shape_iii)):
        if name not in only:
            continue
        try:
            out["shapes"][name] = fn()
        except Exception:  # noqa: BLE001 — the other shapes still run; the failure is in the result
            ok = False
            out["shapes"][name] = {"failed": traceback.format_exc()}
            print(out["shapes"][name]["failed"], flush=True)
        b.torch.cuda.empty_cache()
        save()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
