#!/usr/bin/env python3
"""The ingest dispatch (wq_ingest_dispatch_device, csrc/wq_dispatch.hip) against a torch composite and
against the host path it replaces, in one process, the forms alternating:

  hip    Router.dispatch_device on the decode's arrays in device memory: every output, the run table and
         the counters, asynchronous, no read-back;
  torch  a composite on the same device arrays: the class of every frame from masks, nonzero per class,
         gathers of the rows, the 40-byte ops assembled from five 8-byte columns, the runs from the
         effective frames' kinds and cumulative sums. nonzero reads sizes back;
  host   the path it replaces: the classification part of processing.SubscriptionProcessor — the Python
         loop over the messages with its drop rules and its flush-on-reorder batching, filling the lists
         a run hands to the router, the router calls left out — over the decode's arrays on the host.
         Measured on a 1/100 sample of the frames (a contiguous prefix) and scaled by 100: said so in the
         output.

Shapes:
  c5        C5's 1M frames, all LocalMessage: one run;
  c5_subs   the same with 1% subscribes spread evenly: about 20,000 runs, what the run table costs;
  mix_10m   10M frames of the instruction, world and position mix of tests/seq_reference.random_events
            (its disconnects left out).

hip's rows, ops and run table are checked equal to the torch form's and a second call byte-identical
before anything is timed. Then --warmup untimed and --reps timed repeats per form, a synchronise on both
sides of each; min / mean / max with every number. bytes_moved is what the call must read and write once:
10 B per frame read, 1 B class written, 24 + 37 B per LocalMessage row, 13 B per GlobalMessage row,
24 + 44 B per op, 4 B per listed frame, 20 B per run.

One shape per process keeps every GPU step under a time limit of its own; a run with --only adds its
shapes to the file the earlier runs wrote.

    python tools/ingest_dispatch_bench.py [--scale 1.0] [--only c5,c5_subs,mix_10m] [--forms hip,torch,host]
                                          [--reps 7] [--warmup 3] [--out profiles/ingest_dispatch_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from peer_budget_bench import Bench, summary  # noqa: E402

HBM_BYTES_PER_S = 8e12
HOST_SAMPLE = 100
OK, POS, ATG, WK, SK = 1, 2, 16, 32, 64
FULL = OK | POS | WK | SK
HB, SUB, UNSUB, GLOBAL, LOCAL = 0, 4, 5, 6, 7


def host_classify(ins, flags, world, sender, repl, pos):
    """process_tick's loop without the router: per message the handlers' drop rules, consecutive table
    events into one op batch, consecutive read events into the lists of one route and one route_global."""
    from worldql_server_amd import abi
    runs = 0
    n = len(ins)
    i = 0
    while i < n:
        is_read = ins[i] in (LOCAL, GLOBAL)
        if not is_read and ins[i] not in (SUB, UNSUB):
            i += 1                                       # not a subscription-task event: another channel
            continue
        l_idx, l_pos, l_world, l_sender, l_repl = [], [], [], [], []
        g_idx, g_world, g_sender, g_repl = [], [], [], []
        ops = []
        j = i
        while j < n and ((ins[j] in (LOCAL, GLOBAL)) == is_read) and ins[j] in (LOCAL, GLOBAL, SUB, UNSUB):
            f = flags[j]
            if f & OK:
                if ins[j] == GLOBAL:
                    if not f & ATG and f & WK:
                        g_idx.append(j), g_world.append(world[j]), g_sender.append(sender[j]), g_repl.append(repl[j])
                elif not f & ATG and f & POS and f & WK:
                    if ins[j] == LOCAL:
                        l_idx.append(j), l_pos.append((pos[j, 0], pos[j, 1], pos[j, 2])), l_world.append(world[j])
                        l_sender.append(sender[j]), l_repl.append(repl[j])
                    elif f & SK:
                        ops.append(abi.make_op(world[j], sender[j], abi.OP_SUBSCRIBE if ins[j] == SUB else abi.OP_UNSUBSCRIBE,
                                               pos=(pos[j, 0], pos[j, 1], pos[j, 2])))
            j += 1
        if l_idx:
            np.array(l_pos, np.float64), np.array(l_world, np.uint32), np.array(l_sender, np.uint32), np.array(l_repl, np.uint8)
        if g_idx:
            np.array(g_world, np.uint32), np.array(g_sender, np.uint32), np.array(g_repl, np.uint8)
        if ops:
            np.array(ops, dtype=abi.OP_DTYPE)
        runs += 1
        i = j
    return runs


class DispatchBench(Bench):
    def torch_form(self, t):
        """The composite: a dict of the same arrays (ops as [k, 5] int64 words)."""
        torch = self.torch
        ins, fl, world, sender = t["instruction"], t["flags"], t["world"], t["sender"]
        ok = (fl & OK) != 0
        atg, has_pos = (fl & ATG) != 0, (fl & POS) != 0
        world_ok = ((fl & WK) != 0) & (world >= 0) & (world < 0xFFFFFFFE)      # int64 views of the u32 values
        sender_ok = ((fl & SK) != 0) & (sender != 0xFFFFFFFF)
        full = ~atg & has_pos & world_ok
        cls = torch.full_like(ins, 8)                                          # other
        cls = torch.where((ins == 8) | (ins == 9) | (ins == 11), 7, cls)
        cls = torch.where(ins == HB, 1, cls)
        cls = torch.where(ins == LOCAL, torch.where(full, 2, 9), cls)
        cls = torch.where(ins == GLOBAL, torch.where(atg, 4, torch.where(world_ok, 3, 9)), cls)
        cls = torch.where(ins == SUB, torch.where(atg | ~has_pos, 9, torch.where(world_ok & sender_ok, 5, 6)), cls)
        cls = torch.where(ins == UNSUB, torch.where(full & sender_ok, 5, 9), cls)
        cls = torch.where(ok, cls, 0).to(torch.uint8)
        li, gi, oi = (torch.nonzero(cls == c).flatten() for c in (2, 3, 5))
        row_sender = torch.where(sender_ok, sender, 0xFFFFFFFF)
        out = dict(cls=cls, l_src=li, l_pos=t["pos_bits"][li], l_world=world[li], l_sender=row_sender[li], l_repl=t["repl"][li],
                   g_src=gi, g_world=world[gi], g_sender=row_sender[gi], g_repl=t["repl"][gi], op_src=oi)
        out["ops"] = torch.cat([(world[oi] | (sender[oi] << 32)).unsqueeze(1), (ins[oi] == UNSUB).to(torch.int64).unsqueeze(1),
                                t["pos_bits"][oi]], dim=1)
        out["side_src"] = torch.cat([torch.nonzero(cls == c).flatten() for c in (1, 4, 7, 8, 6)])
        kind = torch.where(cls == 5, 1, torch.where((cls == 2) | (cls == 3), 2, 0))
        eff = torch.nonzero(kind).flatten()
        k = kind[eff]
        start = torch.ones_like(k, dtype=torch.bool)
        start[1:] = k[1:] != k[:-1]
        first = eff[start]
        before = lambda c: torch.cumsum(cls == c, 0)[first] - (cls[first] == c).to(torch.int64)   # noqa: E731
        out["runs"] = torch.stack([k[start], first, before(2), before(3), before(5)], dim=1)
        return out

    def run(self, name, d):
        from worldql_server_amd import ingest
        from worldql_server_amd.router import Router
        torch, abi = self.torch, self.abi
        n = len(d["instruction"])
        r = Router(16, 0)
        stream = torch.cuda.Stream(device=self.dev)
        self.sync()
        r.set_stream(stream.cuda_stream)
        dev = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if v.dtype == np.uint32 else np.ascontiguousarray(v)).to(self.dev)
               for k, v in d.items()}
        src = abi.DispatchIn(**{k: dev[k].data_ptr() for k in ("instruction", "flags", "world", "sender", "repl", "pos")})
        widths = dict(cls=1, l_src=4, l_pos=24, l_world=4, l_sender=4, l_repl=1, g_src=4, g_world=4, g_sender=4, g_repl=1,
                      ops=40, op_src=4, side_src=4, runs=20)
        cap = n + 1
        outs = {k: torch.zeros(max(n * w, 8) + (20 if k == "runs" else 0), dtype=torch.uint8, device=self.dev)
                for k, w in widths.items()}
        out = abi.DispatchOut(**{k: v.data_ptr() for k, v in outs.items()}, runs_capacity=cap)
        cnt = torch.zeros(abi.DISPATCH_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        # the torch form's inputs: the same arrays, the u32 values widened once (not timed) so masks and ors are plain
        t_in = dict(instruction=dev["instruction"].to(torch.int64), flags=dev["flags"].to(torch.int64),
                    world=dev["world"].to(torch.int64) & 0xFFFFFFFF, sender=dev["sender"].to(torch.int64) & 0xFFFFFFFF, repl=dev["repl"],
                    pos_bits=dev["pos"].view(torch.int64).reshape(n, 3))

        def hip():
            r.dispatch_device(src, n, out, cnt.data_ptr())

        def torch_form():
            with torch.cuda.stream(stream):
                return self.torch_form(t_in)

        self.sync()
        hip()
        self.sync()
        c = ingest.dispatch_counters(cnt.cpu().numpy())
        first = {k: v.clone() for k, v in outs.items()}
        res = {"frames": n, "counters": c}
        moved = (n * 11 + c["n_local"] * 61 + c["n_global"] * 13 + c["n_op"] * 68 + c["side_begin"][5] * 4 + (c["n_runs"] + 1) * 20)
        res["bytes_moved"] = moved
        checks = {}
        if "torch" in self.forms:
            tf = torch_form()
            self.sync()
            rows = dict(l_src=c["n_local"], g_src=c["n_global"], op_src=c["n_op"], side_src=c["side_begin"][5])
            u32 = lambda k, m: outs[k][:4 * m].view(torch.int32).to(torch.int64) & 0xFFFFFFFF   # noqa: E731
            for k, m in rows.items():
                checks["hip_" + k + "_equals_torch"] = bool(torch.equal(u32(k, m), tf[k]))
            checks["hip_cls_equals_torch"] = bool(torch.equal(outs["cls"][:n], tf["cls"]))
            checks["hip_ops_equal_torch"] = bool(torch.equal(outs["ops"][:40 * c["n_op"]].view(torch.int64).reshape(-1, 5), tf["ops"]))
            checks["hip_l_pos_equals_torch"] = bool(torch.equal(outs["l_pos"][:24 * c["n_local"]].view(torch.int64).reshape(-1, 3),
                                                                tf["l_pos"]))
            runs = outs["runs"][:20 * c["n_runs"]].view(torch.int32).to(torch.int64).reshape(-1, 5)
            checks["hip_runs_equal_torch"] = bool(torch.equal(runs, tf["runs"]))
            del tf
        hip()
        self.sync()
        checks["hip_deterministic"] = all(torch.equal(outs[k], first[k]) for k in outs)
        res["checks"] = checks
        assert all(checks.values()), checks
        del first
        fns = {"hip": hip}
        if "torch" in self.forms:
            fns["torch"] = torch_form
        for fn in fns.values():
            for _ in range(self.a.warmup):
                fn()
        times = {f: [] for f in fns}
        for _ in range(self.a.reps):  # alternating
            for f, fn in fns.items():
                times[f] += self.timed(fn, 1)
        if "host" in self.forms:
            m = max(n // HOST_SAMPLE, 1)
            h = {k: np.ascontiguousarray(v[:m]) for k, v in d.items()}
            h = {k: (v.tolist() if v.ndim == 1 else v) for k, v in h.items()}      # Python values, as Message fields are
            host_times = []
            for _ in range(max(self.a.host_reps, 1)):
                t0 = time.perf_counter()
                host_classify(h["instruction"], h["flags"], h["world"], h["sender"], h["repl"], h["pos"])
                host_times.append((time.perf_counter() - t0) * 1e3 * (n / m))
            times["host"] = host_times
            res["host_note"] = (f"measured on the first {m} frames (1/{HOST_SAMPLE} of the shape) and scaled by {n / m:.1f}; "
                                "the router calls are left out")
        res["times"] = {f: summary(v) for f, v in times.items()}
        hip_ms = statistics.fmean(times["hip"])
        res["hip_fraction_of_8TBps"] = round(moved / (hip_ms / 1e3) / HBM_BYTES_PER_S, 4)
        res["hip_ns_per_frame"] = round(hip_ms * 1e6 / n, 3)
        for f in ("torch", "host"):
            if f in times:
                res[f + "_over_hip"] = round(statistics.fmean(times[f]) / hip_ms, 3)
        print(f"[{name}] " + json.dumps(res), flush=True)
        self.sync()
        r.set_stream(None)
        r.close()
        del outs, dev, t_in
        torch.cuda.empty_cache()
        return res

    # ---- shapes ----
    def scaled(self, n):
        return max(200, int(round(n * self.a.scale)))

    def all_local(self, n):
        rng = np.random.default_rng(5)
        return dict(instruction=np.full(n, LOCAL, np.uint8), flags=np.full(n, FULL, np.uint8),
                    world=rng.integers(0, 3, n).astype(np.uint32), sender=rng.integers(0, 100_000, n).astype(np.uint32),
                    repl=np.zeros(n, np.uint8), pos=rng.uniform(-5000, 5000, (n, 3)))

    def shape_c5(self):
        return self.run("c5", self.all_local(self.scaled(1_000_000)))

    def shape_c5_subs(self):
        d = self.all_local(self.scaled(1_000_000))
        d["instruction"][50::100] = SUB
        return self.run("c5_subs", d)

    def shape_mix_10m(self):
        """random_events' mix: subscribe 33, unsubscribe 14, LocalMessage 36, GlobalMessage 14 (its 3% of
        disconnects left out); 5% of the names "@global", 9% refused or unknown, 2% without a position."""
        n = self.scaled(10_000_000)
        rng = np.random.default_rng(7)
        ins = rng.choice(np.array([SUB, UNSUB, LOCAL, GLOBAL], np.uint8), size=n, p=np.array([33, 14, 36, 14]) / 97)
        kind_w = rng.choice(3, size=n, p=[0.86, 0.05, 0.09])
        world = np.where(kind_w == 0, rng.integers(0, 6, n), np.where(kind_w == 1, 0xFFFFFFFE, 0xFFFFFFFF)).astype(np.uint32)
        flags = (OK | SK | np.where(rng.random(n) < 0.98, POS, 0) | np.where(kind_w == 0, WK, 0) |
                 np.where(kind_w == 1, ATG, 0)).astype(np.uint8)
        return self.run("mix_10m", dict(instruction=ins, flags=flags, world=world, sender=rng.integers(0, 300, n).astype(np.uint32),
                                        repl=rng.integers(0, 3, n).astype(np.uint8), pos=rng.uniform(-40, 40, (n, 3))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default="c5,c5_subs,mix_10m")
    ap.add_argument("--forms", default="hip,torch,host")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_dispatch_bench.json"))
    a = ap.parse_args()
    b = DispatchBench(a)
    only = a.only.split(",")
    out = {"tool": "tools/ingest_dispatch_bench.py", "scale": a.scale, "reps": a.reps, "warmup": a.warmup, "host_reps": a.host_reps,
           "forms": b.forms, "timing": "host clock, a device synchronise on both sides of every repeat",
           "torch": "masks, nonzero per class, gathers, cumulative sums on the same device arrays (u32 inputs widened once, untimed); "
                    "nonzero reads sizes back",
           "host": f"the classification and batching loop of processing.SubscriptionProcessor over the decode's arrays on the host, "
                   f"router calls left out, on 1/{HOST_SAMPLE} of the frames, scaled", "shapes": {}}
    if os.path.exists(a.out):   # one shape per process, each under its own time limit: keep the other shapes' results
        with open(a.out) as fh:
            prev = json.load(fh)
        if all(prev.get(k) == out[k] for k in ("tool", "scale", "reps", "warmup")):
            out["shapes"] = {k: v for k, v in prev.get("shapes", {}).items() if k not in only}
    ok = True
    for name in ("c5", "c5_subs", "mix_10m"):
        if name not in only:
            continue
        try:
            out["shapes"][name] = getattr(b, "shape_" + name)()
        except Exception:  # noqa: BLE001 — the other shapes still run; the failure is in the result
            ok = False
            out["shapes"][name] = {"failed": traceback.format_exc()}
            print(out["shapes"][name]["failed"], flush=True)
        b.torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
