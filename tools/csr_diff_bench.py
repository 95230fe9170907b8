#!/usr/bin/env python3
"""The interest diff (wq_csr_diff_device, csrc/wq_csr_diff.hip) against a torch composite on the same
device arrays, in one process, the forms alternating:

  hip        Router.csr_diff_device: rows / scan / flag / scan / emit, asynchronous, no read-back;
  composite  `row << 32 | peer` keys of both sides (torch.repeat_interleave, given P by the host),
             membership by torch.searchsorted (both key arrays are globally sorted), compaction by a
             boolean mask, row offsets from a cumulative sum sampled at the row starts.

Shapes, at full size with --scale 1:
  i    C5, consecutive ticks (follow + positions + radius route, then the diff): 1M short rows
  ii   C3 table and messages, the tick before and after one churn step that moves 5% of the peers
  iii  two independent C3 message draws against the same table (output about as large as the input)
  iv   P pairs in one row among 1M empty rows, against the same P spread evenly over the rows

Every form's outputs are checked equal to each other (and to interest.csr_diff_np where the pairs
fit --host-check-pairs) before anything is timed. Then --warmup untimed and --reps timed repeats per
form, a synchronise on both sides of each; min / mean / max are reported with every number.

    python tools/csr_diff_bench.py [--scale 1.0] [--only i,ii,iii,iv] [--forms hip,composite] [--reps 7]
                                   [--out profiles/csr_diff_bench.json]
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

    # ---- helpers ----
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

    def route(self, r, pos, world, sender, repl, M, cap):
        """One tick on device arrays into fresh tensors; grows until it fits. Returns (offsets, peers, P)."""
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
                return offs, peers, int(c["n_pairs"])
            r.route_health()
            cap = int(c["n_pairs"]) + 1024

    def composite(self, oo, op, Po, no, npr, Pn, M, with_left=True):
        """The torch baseline; int32 tensors holding u32 bits (offsets below 2^31)."""
        torch = self.torch
        rows_ar = torch.arange(M, device=self.dev)

        def keys(off, peers, P):
            counts = (off[1:] - off[:-1]).long()
            rows = torch.repeat_interleave(rows_ar, counts, output_size=P)
            return (rows << 32) | (peers[:P].long() & 0xFFFFFFFF)

        ko, kn = keys(oo, op, Po), keys(no, npr, Pn)

        def side(k, other, off, peers, P):
            if P == 0:
                return torch.zeros(M + 1, dtype=torch.int32, device=self.dev), peers[:0]
            if len(other):
                at = torch.searchsorted(other, k).clamp_(max=len(other) - 1)
                keep = other[at] != k
            else:
                keep = torch.ones(P, dtype=torch.bool, device=self.dev)
            out = peers[:P][keep]
            cs = torch.zeros(P + 1, dtype=torch.int32, device=self.dev)
            torch.cumsum(keep, 0, dtype=torch.int32, out=cs[1:])
            return cs[off.long()], out

        eo, ep = side(kn, ko, no, npr, Pn)
        if not with_left:
            return eo, ep, None, None
        lo, lp = side(ko, kn, oo, op, Po)
        return eo, ep, lo, lp

    # ---- one shape: check, then time every form ----
    def run_pair(self, r, name, M, old, new, extra=None):
        """old / new: (offsets, peers, P) device tensors. Returns the shape's result dict."""
        torch, abi = self.torch, self.abi
        (oo, op, Po), (no, npr, Pn) = old, new
        eo, lo = self.i32(M + 1), self.i32(M + 1)
        ep, lp = self.i32(Pn), self.i32(Po)
        cnt = torch.zeros(24, dtype=torch.uint8, device=self.dev)

        def hip():
            r.csr_diff_device(M, oo.data_ptr(), op.data_ptr(), op.numel(), no.data_ptr(), npr.data_ptr(), npr.numel(),
                              eo.data_ptr(), ep.data_ptr(), ep.numel(), lo.data_ptr(), lp.data_ptr(), lp.numel(),
                              cnt.data_ptr())

        self.sync()
        hip()
        self.sync()
        c = cnt.cpu().numpy().view(abi.DIFF_COUNTERS_DTYPE)[0]
        assert c["error"] == 0 and c["overflow"] == 0, (int(c["error"]), int(c["overflow"]))
        E, L = int(c["n_entered"]), int(c["n_left"])
        res = {"rows": M, "pairs_old": Po, "pairs_new": Pn, "entered": E, "left": L}
        checks = {}
        if "composite" in self.forms:
            t_eo, t_ep, t_lo, t_lp = self.composite(oo, op, Po, no, npr, Pn, M)
            checks["hip_equals_composite"] = bool(
                len(t_ep) == E and len(t_lp) == L and torch.equal(t_eo, eo) and torch.equal(t_lo, lo)
                and torch.equal(t_ep, ep[:E]) and torch.equal(t_lp, lp[:L]))
            del t_eo, t_ep, t_lo, t_lp
        if max(Po, Pn) <= self.a.host_check_pairs:
            want = self.interest.csr_diff_np(self.host_u32(oo), self.host_u32(op, Po), self.host_u32(no),
                                             self.host_u32(npr, Pn))
            got = (self.host_u32(eo), self.host_u32(ep, E), self.host_u32(lo), self.host_u32(lp, L))
            checks["hip_equals_csr_diff_np"] = all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        # twice the same bytes
        first = (eo.clone(), ep[:E].clone(), lo.clone(), lp[:L].clone())
        hip()
        self.sync()
        checks["hip_deterministic"] = all(torch.equal(x, y) for x, y in zip(first, (eo, ep[:E], lo, lp[:L])))
        del first
        res["checks"] = checks
        assert all(checks.values()), checks
        fns = {"hip": hip}
        if "composite" in self.forms:
            fns["composite"] = lambda: self.composite(oo, op, Po, no, npr, Pn, M)
        for fn in fns.values():
            for _ in range(self.a.warmup):
                fn()
        times = {f: [] for f in fns}
        for _ in range(self.a.reps):  # alternating
            for f, fn in fns.items():
                times[f] += self.timed(fn, 1)
        res["times"] = {f: summary(v) for f, v in times.items()}
        nbytes = 8 * (M + 1) + 4 * (Po + Pn) + 8 * (M + 1) + 4 * (E + L)
        hip_s = statistics.fmean(times["hip"]) / 1e3
        res["budget_bytes"] = nbytes
        res["hip_frac_of_8TBps"] = round(nbytes / hip_s / HBM_PEAK, 4)
        if "composite" in times:
            th, tc = times["hip"], times["composite"]
            spread = max(max(th) - min(th), max(tc) - min(tc))
            res["bar"] = {"hip_minus_composite_ms": round(statistics.fmean(th) - statistics.fmean(tc), 4),
                          "spread_ms": round(spread, 4),
                          "hip_not_slower": bool(statistics.fmean(th) - statistics.fmean(tc) <= spread)}
        if extra:
            res.update(extra(hip, cnt, res))
        print(f"[{name}] " + json.dumps(res), flush=True)
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
        world = torch.zeros(M, dtype=torch.int32, device=self.dev)
        sender = torch.from_numpy(np.arange(M, dtype=np.int32)).to(self.dev)
        repl = torch.zeros(M, dtype=torch.uint8, device=self.dev)
        cap = 16 * M + 1024
        ticks = []
        pos_d = []
        for _ in range(3):
            pos_d.append(torch.from_numpy(c5.pos.copy()).to(self.dev))
            c5.step()
        self.sync()

        def table(i):
            r.follow_peers_device(world.data_ptr(), pos_d[i].data_ptr(), M)
            r.set_peer_positions_device(pos_d[i].data_ptr(), M)

        for i in range(2):
            table(i)
            ticks.append(self.route(r, pos_d[i], world, sender, repl, M, cap))
        offs, peers = self.i32(M + 1), self.i32(cap)
        rcnt = torch.zeros(24, dtype=torch.uint8, device=self.dev)
        state = {"i": 0}

        def whole_tick():  # follow + positions + radius route (alternating between two positions)
            i = 1 + (state["i"] & 1)
            state["i"] += 1
            table(i)
            r.route_device(pos_d[i].data_ptr(), world.data_ptr(), sender.data_ptr(), repl.data_ptr(), M,
                           offs.data_ptr(), peers.data_ptr(), None, cap, rcnt.data_ptr())

        def extra(hip, cnt, res):
            for _ in range(self.a.warmup):
                whole_tick()
            tick = self.timed(whole_tick, self.a.reps)
            # launch floor: the same launches on one empty row; read-back: the counters to the host
            one = torch.zeros(2, dtype=torch.int32, device=self.dev)
            o1, o2 = self.i32(2), self.i32(2)

            def floor():
                r.csr_diff_device(1, one.data_ptr(), None, 0, one.data_ptr(), None, 0, o1.data_ptr(), None, 0,
                                  o2.data_ptr(), None, 0, cnt.data_ptr())

            def with_read():
                hip()
                cnt.cpu()

            for _ in range(self.a.warmup):
                floor()
            fl = self.timed(floor, self.a.reps)
            rd = self.timed(with_read, self.a.reps)
            hip_ms = res["times"]["hip"]["mean_ms"]
            tick_ms = statistics.fmean(tick)
            return {"whole_tick": summary(tick), "diff_share_of_tick_plus_diff": round(hip_ms / (tick_ms + hip_ms), 4),
                    "launch_floor_one_empty_row": summary(fl), "diff_plus_counter_read": summary(rd),
                    "launch_share_of_diff": round(statistics.fmean(fl) / hip_ms, 4),
                    "read_back_extra_ms": round(statistics.fmean(rd) - hip_ms, 4)}

        out = self.run_pair(r, "i", M, ticks[0], ticks[1], extra)
        r.close()
        return out

    def c3_setup(self):
        from worldql_server_amd import synth, synth_ext
        from worldql_server_amd.router import Router
        torch, s = self.torch, self.a.scale
        n_peers = max(1, int(round(1_000_000 * s)))
        M = max(1, int(round(10_000_000 * s)))
        half, sig = 4096.0 * (s ** (1.0 / 3.0)), 128.0 * (s ** (1.0 / 3.0))
        peer_pos = synth_ext.hotspot_positions(3, 1, n_peers, half, 256, sig)
        r = Router(16, 0)
        pworld = np.zeros(n_peers, np.uint32)
        r.follow_peers(pworld, peer_pos)  # the C3 table: every peer's 3x3x3
        pos = torch.from_numpy(synth_ext.hotspot_positions(3, 2, M, half, 256, sig)).to(self.dev)
        sender = self.dev_u32(synth.stream(3, 3).below(n_peers, M))
        world = torch.zeros(M, dtype=torch.int32, device=self.dev)
        repl = torch.zeros(M, dtype=torch.uint8, device=self.dev)
        self.sync()
        return r, M, n_peers, half, sig, peer_pos, pworld, pos, world, sender, repl

    def shape_ii_iii(self, which):
        from worldql_server_amd import synth, synth_ext
        torch = self.torch
        r, M, n_peers, half, sig, peer_pos, pworld, pos, world, sender, repl = self.c3_setup()
        cap = 48 * M + 1024
        out = {}
        a = self.route(r, pos, world, sender, repl, M, cap)
        if "iii" in which:
            pos2 = torch.from_numpy(synth_ext.hotspot_positions(3, 12, M, half, 256, sig)).to(self.dev)
            sender2 = self.dev_u32(synth.stream(3, 13).below(n_peers, M))
            b = self.route(r, pos2, world, sender2, repl, M, a[2] + a[2] // 8 + 1024)
            out["iii"] = self.run_pair(r, "iii", M, a, b)
            del b, pos2, sender2
            torch.cuda.empty_cache()
        if "ii" in which:
            g = synth.stream(3, 21)
            moved = np.flatnonzero(g.uniform(0.0, 1.0, n_peers) < 0.05)
            new = peer_pos.copy()
            new[moved] += np.stack([g.normal(len(moved)) for _ in range(3)], 1) * 16.0
            new = np.clip(new, -half, np.nextafter(half, -np.inf))
            r.follow_peers(pworld, new)  # one churn step
            b = self.route(r, pos, world, sender, repl, M, a[2] + a[2] // 8 + 1024)
            out["ii"] = self.run_pair(r, "ii", M, a, b)
            out["ii"]["peers_moved"] = int(len(moved))
        r.close()
        return out

    def shape_iv(self):
        from worldql_server_amd.router import Router
        torch = self.torch
        M = max(2, int(round(1_000_000 * self.a.scale))) + 1
        per = 16
        P = per * (M - 1)
        idx = np.arange(P, dtype=np.uint32)
        old_p, new_p = self.dev_u32(2 * idx), self.dev_u32(2 * idx + (idx & 1))  # every other peer changes
        one = np.zeros(M + 1, np.uint32)
        one[M // 2 + 1:] = P                                 # all of it in row M / 2
        even = np.zeros(M + 1, np.uint32)
        even[1:M] = per * np.arange(1, M, dtype=np.uint32)   # 16 per row, the last row empty
        even[M] = P
        r = Router(16, 0)
        d_one, d_even = self.dev_u32(one), self.dev_u32(even)
        self.sync()
        res_one = self.run_pair(r, "iv_one_row", M, (d_one, old_p, P), (d_one, new_p, P))
        res_even = self.run_pair(r, "iv_spread", M, (d_even, old_p, P), (d_even, new_p, P))
        r.close()
        ratio = res_one["times"]["hip"]["mean_ms"] / res_even["times"]["hip"]["mean_ms"]
        return {"one_row": res_one, "spread": res_even, "hip_one_row_over_spread": round(ratio, 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default="i,ii,iii,iv")
    ap.add_argument("--forms", default="hip,composite")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-check-pairs", type=int, default=40_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_diff_bench.json"))
    a = ap.parse_args()
    b = Bench(a)
    only = a.only.split(",")
    out = {"tool": "tools/csr_diff_bench.py", "scale": a.scale, "reps": a.reps, "warmup": a.warmup,
           "forms": b.forms, "timing": "host clock, a device synchronise on both sides of every repeat",
           "budget": "reads 8(M+1) + 4(P_old + P_new), writes 8(M+1) + 4(E + L) bytes; share of 8 TB/s",
           "shapes": {}}
    ok = True

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    steps = []
    if "i" in only:
        steps.append(("i", b.shape_i))
    if "ii" in only or "iii" in only:
        steps.append(("c3", lambda: b.shape_ii_iii([x for x in only if x in ("ii", "iii")])))
    if "iv" in only:
        steps.append(("iv", b.shape_iv))
    for name, fn in steps:
        try:
            res = fn()
            if name == "c3":
                out["shapes"].update(res)
            else:
                out["shapes"][name] = res
        except Exception:  # noqa: BLE001 — the other shapes still run; the failure is in the result
            ok = False
            out["shapes"][name] = {"failed": traceback.format_exc()}
            print(out["shapes"][name]["failed"], flush=True)
        b.torch.cuda.empty_cache()
        save()
    print(json.dumps({k: (v.get("times") or v.get("failed") or "see file") for k, v in out["shapes"].items()}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
