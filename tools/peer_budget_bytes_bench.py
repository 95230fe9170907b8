#!/usr/bin/env python3
"""The byte budgets (wq_peer_budget_bytes_device, csrc/wq_budget.hip) against a torch composite on the
same device arrays and against the count budget itself, in one process, the forms alternating:

  hip        Router.peer_budget_bytes_device with d_out_bytes and the counters: rows / keys and sizes /
             three u64 scans / weighted radix select / flags / offsets / emit, asynchronous, no read-back;
  composite  the key of every element, a stable sort by key, a stable sort of that order by peer, the
             cumulative sum of the sizes in that order less its value at the row's start, the mask
             cum <= W scattered back so the kept elements come out in input order, offsets and per-row
             bytes from segment sums of the mask;
  count      Router.peer_budget_device on the same lists with K, the baseline of the parent commit.

Shapes: the three of tools/peer_budget_bench.py (whose set-up this tool reuses): i the C5 tick
transposed, ii the C3 tick transposed, iii one 16M-element row against the same elements spread out.
Sizes are a fixed-seed mix per message: 96% 100 - 200 B, 4% 2 - 16 KB (mean about 510 B). W is K times
the mean size, so a row keeps about as many elements as under the count bench's K and about the same
rows are cut.

The hip and composite outputs are checked equal (and equal to interest.peer_budget_bytes_np where the
elements fit --host-check-elements) before anything is timed. Then --warmup untimed and --reps timed
repeats per form, a synchronise on both sides of each; min / mean / max are reported with every number.

    python tools/peer_budget_bytes_bench.py [--scale 1.0] [--only i,ii,iii] [--forms hip,composite,count]
                                            [--reps 7] [--append] [--out profiles/peer_budget_bytes_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from peer_budget_bench import HBM_PEAK, Bench, summary  # noqa: E402


def frame_mix(n, seed=11):
    rng = np.random.default_rng(seed)
    s = rng.integers(100, 201, size=n)
    big = rng.random(n) < 0.04
    s[big] = rng.integers(2048, 16385, size=int(big.sum()))
    return s.astype(np.uint32)


class BytesBench(Bench):
    def composite_bytes(self, po, msgs, n, mpos, msize, ppos, w):
        """The torch baseline: (offsets, kept, bytes per row)."""
        torch = self.torch
        n_peers = po.numel() - 1
        lens = (po[1:] - po[:-1]).long()
        out_off = torch.zeros(n_peers + 1, dtype=torch.int32, device=self.dev)
        out_bytes = torch.zeros(n_peers, dtype=torch.int64, device=self.dev)
        if n == 0:
            return out_off, msgs[:0], out_bytes
        row = torch.repeat_interleave(torch.arange(n_peers, device=self.dev), lens, output_size=n)
        m = msgs[:n].long()
        d = mpos[m] - ppos[row]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        d2 = torch.where(torch.isnan(d2), torch.full_like(d2, float("inf")), d2)
        by_key = torch.argsort(d2, stable=True)
        order = by_key[torch.argsort(row[by_key], stable=True)]
        sz = msize[m[order]]
        incl = torch.cumsum(sz, 0)
        first = po.long()[row[order]]                      # the row's first position in `order`
        cum = incl - (incl - sz)[first]
        keep = torch.zeros(n, dtype=torch.bool, device=self.dev)
        keep[order[cum <= w]] = True
        kept_per_row = torch.zeros(n_peers, dtype=torch.int64, device=self.dev).index_add_(0, row, keep.long())
        torch.cumsum(kept_per_row, 0, dtype=torch.int32, out=out_off[1:])
        out_bytes.index_add_(0, row, torch.where(keep, msize[m], torch.zeros_like(m)))
        return out_off, msgs[:n][keep], out_bytes

    def run(self, r, name, po, msgs, n, mpos, ppos, k, composite_ok=True):
        """The count bench's shape with sizes: po[n_peers + 1], msgs[n], K as the count bench sets it."""
        torch, abi = self.torch, self.abi
        n_peers = po.numel() - 1
        sizes = frame_mix(mpos.shape[0])
        msize32 = self.dev_u32(sizes)
        msize = msize32.long()
        w = int(round(k * float(sizes.mean())))
        oo, om = self.i32(n_peers + 1), self.i32(n)
        ob = torch.empty(max(n_peers, 1), dtype=torch.int64, device=self.dev)
        cnt = torch.zeros(40, dtype=torch.uint8, device=self.dev)
        koo, kom = self.i32(n_peers + 1), self.i32(n)
        kcnt = torch.zeros(24, dtype=torch.uint8, device=self.dev)

        def hip():
            r.peer_budget_bytes_device(po.data_ptr(), msgs.data_ptr() if n else None, n_peers, n, mpos.data_ptr(),
                                       msize32.data_ptr(), mpos.shape[0], ppos.data_ptr(), ppos.shape[0], w, None,
                                       oo.data_ptr(), om.data_ptr() if n else None, ob.data_ptr(), cnt.data_ptr())

        def count():
            r.peer_budget_device(po.data_ptr(), msgs.data_ptr() if n else None, n_peers, n, mpos.data_ptr(),
                                 mpos.shape[0], ppos.data_ptr(), ppos.shape[0], k, None, koo.data_ptr(),
                                 kom.data_ptr() if n else None, kcnt.data_ptr())

        self.sync()
        hip()
        self.sync()
        c = cnt.cpu().numpy().view(abi.BUDGET_BYTES_COUNTERS_DTYPE)[0]
        assert c["error"] == 0 and int(c["n_in"]) == n, (int(c["error"]), int(c["n_in"]), n)
        kept = int(c["n_kept"])
        res = {"peers": n_peers, "elements": n, "k": k, "w": w, "kept": kept, "rows_cut": int(c["rows_cut"]),
               "bytes_in": int(c["bytes_in"]), "bytes_kept": int(c["bytes_kept"]),
               "longest_row": int((po[1:] - po[:-1]).max().item()) if n_peers else 0}
        checks = {}
        with_composite = "composite" in self.forms and composite_ok
        if with_composite:
            t_oo, t_om, t_ob = self.composite_bytes(po, msgs, n, mpos, msize, ppos, w)
            checks["hip_equals_composite"] = bool(len(t_om) == kept and torch.equal(t_oo, oo)
                                                  and torch.equal(t_om, om[:kept]) and torch.equal(t_ob, ob[:n_peers]))
            del t_oo, t_om, t_ob
        elif "composite" in self.forms:
            res["composite"] = "not measured at this size (see composite_scale)"
        if n <= self.a.host_check_elements:
            w_oo, w_om, w_ob, w_cnt = self.interest.peer_budget_bytes_np(
                self.host_u32(po), self.host_u32(msgs, n), mpos.cpu().numpy(), sizes, ppos.cpu().numpy(), w=w)
            checks["hip_equals_peer_budget_bytes_np"] = bool(
                self.host_u32(oo).tobytes() == w_oo.tobytes() and self.host_u32(om, kept).tobytes() == w_om.tobytes()
                and ob[:n_peers].cpu().numpy().view(np.uint64).tobytes() == w_ob.tobytes()
                and {f: int(c[f]) for f in w_cnt} == w_cnt)
        first = (oo.clone(), om[:kept].clone(), ob.clone())
        fns = {"hip": hip}
        if "count" in self.forms:
            count()                                          # between two byte-budget calls on the handle
            self.sync()
            kc = kcnt.cpu().numpy().view(abi.BUDGET_COUNTERS_DTYPE)[0]
            res["count_kept"], res["count_rows_cut"] = int(kc["n_kept"]), int(kc["rows_cut"])
            fns["count"] = count
        hip()
        self.sync()
        checks["hip_deterministic"] = bool(torch.equal(first[0], oo) and torch.equal(first[1], om[:kept])
                                           and torch.equal(first[2], ob))
        del first
        res["checks"] = checks
        assert all(checks.values()), checks
        if with_composite:
            fns["composite"] = lambda: self.composite_bytes(po, msgs, n, mpos, msize, ppos, w)
        for fn in fns.values():
            for _ in range(self.a.warmup):
                fn()
        times = {f: [] for f in fns}
        for _ in range(self.a.reps):  # alternating
            for f, fn in fns.items():
                times[f] += self.timed(fn, 1)
        res["times"] = {f: summary(v) for f, v in times.items()}
        # what the call must move: the list, two 24-byte position gathers and a 4-byte size gather per
        # element, the offsets in and out, the kept list, the per-row bytes
        nbytes = 4 * n + 52 * n + 8 * (n_peers + 1) + 4 * kept + 8 * n_peers
        res["must_move_bytes"] = nbytes
        hip_ms = statistics.fmean(times["hip"])
        res["hip_frac_of_8TBps"] = round(nbytes / (hip_ms / 1e3) / HBM_PEAK, 4)
        if "composite" in times:
            res["composite_over_hip"] = round(statistics.fmean(times["composite"]) / hip_ms, 3)
        if "count" in times:
            res["hip_over_count"] = round(hip_ms / statistics.fmean(times["count"]), 3)
        print(f"[{name}] " + json.dumps(res), flush=True)
        del msize, msize32, oo, om, ob, koo, kom
        torch.cuda.empty_cache()
        return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--composite-scale", type=float, default=1.0,
                    help="shape ii: the largest scale at which the composite's buffers fit")
    ap.add_argument("--only", default="i,ii,iii")
    ap.add_argument("--forms", default="hip,composite,count")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-check-elements", type=int, default=3_000_000)
    ap.add_argument("--append", action="store_true", help="keep the shapes an earlier run wrote to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peer_budget_bytes_bench.json"))
    a = ap.parse_args()
    b = BytesBench(a)
    only = a.only.split(",")
    out = {"tool": "tools/peer_budget_bytes_bench.py", "scale": a.scale, "composite_scale": a.composite_scale,
           "reps": a.reps, "warmup": a.warmup, "forms": b.forms,
           "timing": "host clock, a device synchronise on both sides of every repeat",
           "sizes": "per message, seed 11: 96% uniform 100 - 200 B, 4% uniform 2,048 - 16,384 B; W = K x the mean size",
           "must_move": "reads 4 n (the list) + 52 n (two position gathers, one size) + 4 (n_peers + 1), writes "
                        "4 (n_peers + 1) + 4 kept + 8 n_peers bytes; share of 8 TB/s",
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
