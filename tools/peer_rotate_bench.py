#!/usr/bin/env python3
"""The fair share (wq_peer_rotate_device, csrc/wq_rotate.hip) against a torch composite on the same
device arrays and against the count budget on the same input, in one process, the forms alternating:

  hip              Router.peer_rotate_device, count share only, with the counters: rows of both CSRs /
                   cut flags / scan / rows' terms / keep flags / scan / offsets / emit, asynchronous, no
                   read-back;
  hip_sizes        the same with d_msg_size, a byte share and d_out_bytes (two u64 scans more);
  composite        row << 32 | message keys of both CSRs, searchsorted of the full keys in the kept keys
                   for the matching, cumsum of the cut mask, searchsorted of row << 32 | cursor for the
                   start, the cyclic rank from gathers of that cumsum, masks, a boolean gather for the
                   output and a scatter for the cursors (rows hold a message once, which the shapes do);
  composite_sizes  the same with the cumsum of cut * size and the per-row bytes;
  count            Router.peer_budget_device on the same lists with the shape's K, which wrote the kept CSR.

Shapes: those of tools/peer_budget_bench.py (whose set-up this tool reuses): i the C5 tick transposed
after K = 1, ii the C3 tick transposed after K = 256, iii one 16M-element row against the same elements
spread over 1M rows (rows ascending here: message j is element j; K = half the row). R = 8 everywhere;
with sizes (the byte bench's mix, mean about 510 B) V = 8 x the mean size. The cursors start at
0xFFFFFFFF and move with every call, as they do in use.

Before anything is timed the hip outputs (offsets, messages, cursors, per-row bytes) are checked equal
to the composite's, equal to interest.peer_rotate_np where the elements fit --host-check-elements, and
byte-identical on a second call from the same cursors. Then --warmup untimed and --reps timed repeats
per form, a synchronise on both sides of each; min / mean / max are reported with every number.

    python tools/peer_rotate_bench.py [--scale 1.0] [--only i,ii,iii] [--reps 7] [--append]
                                      [--forms hip,hip_sizes,composite,composite_sizes,count]
                                      [--out profiles/peer_rotate_bench.json]
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
from peer_budget_bytes_bench import frame_mix  # noqa: E402

R = 8


class RotateBench(Bench):
    def composite_rotate(self, po, msgs, n, ko, km, cursor, r, msize=None, v=0):
        """The torch baseline on int32 tensors holding u32 bits (message indices below 2^31, a message
        at most once per row): (offsets, out, new cursors, bytes per row or None)."""
        torch = self.torch
        n_peers = po.numel() - 1
        dev = self.dev
        pol, kol = po.long(), ko.long()
        cur = cursor.long() & 0xFFFFFFFF
        out_off = torch.zeros(n_peers + 1, dtype=torch.int32, device=dev)
        if n == 0:
            return out_off, msgs[:0], cursor.clone(), (torch.zeros(n_peers, dtype=torch.int64, device=dev)
                                                       if msize is not None else None)
        ar = torch.arange(n_peers, device=dev)
        row = torch.repeat_interleave(ar, pol[1:] - pol[:-1], output_size=n)
        key = (row << 32) | msgs[:n].long()
        nk = int(kol[-1].item())
        krow = torch.repeat_interleave(ar, kol[1:] - kol[:-1], output_size=nk)
        kkey = (krow << 32) | km[:nk].long()
        if nk:
            at = torch.searchsorted(kkey, key)
            cut = kkey[at.clamp(max=nk - 1)] != key
        else:
            cut = torch.ones(n, dtype=torch.bool, device=dev)
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        C = torch.cat([zero, torch.cumsum(cut.long(), 0)])
        P = torch.searchsorted(key, (ar << 32) | cur, right=True)
        s, e = pol[:-1], pol[1:]
        x = torch.arange(n, device=dev)
        after = x >= P[row]
        rank = torch.where(after, C[:-1] - C[P][row], C[:-1] - C[s][row] + (C[e] - C[P])[row])
        chosen = cut & (rank < r)
        size = None
        if msize is not None:
            size = msize[msgs[:n].long()]
            B = torch.cat([zero, torch.cumsum(torch.where(cut, size, torch.zeros_like(size)), 0)])
            run = torch.where(after, B[:-1] - B[P][row], B[:-1] - B[s][row] + (B[e] - B[P])[row]) + size
            chosen &= (rank == 0) | (run <= v)
        keep = ~cut | chosen
        Kc = torch.cat([zero, torch.cumsum(keep.long(), 0)])
        out_off.copy_(Kc[pol].int())
        Ch = torch.cat([zero, torch.cumsum(chosen.long(), 0)])
        last = chosen & (rank == (Ch[e] - Ch[s])[row] - 1)
        new_cursor = cursor.clone()
        new_cursor[row[last]] = msgs[:n][last]
        out_bytes = None
        if size is not None:
            Bk = torch.cat([zero, torch.cumsum(torch.where(keep, size, torch.zeros_like(size)), 0)])
            out_bytes = Bk[e] - Bk[s]
        return out_off, msgs[:n][keep], new_cursor, out_bytes

    def run(self, r, name, po, msgs, n, mpos, ppos, k, composite_ok=True):
        """The count bench's shape: the count budget with K writes the kept CSR, then the forms."""
        torch, abi = self.torch, self.abi
        n_peers = po.numel() - 1
        n_msgs = mpos.shape[0]
        sizes = frame_mix(n_msgs)
        msize32 = self.dev_u32(sizes)
        msize = msize32.long()
        v = int(round(R * float(sizes.mean())))
        ko, km = self.i32(n_peers + 1), self.i32(n)
        kcnt = torch.zeros(24, dtype=torch.uint8, device=self.dev)
        oo, om = self.i32(n_peers + 1), self.i32(n)
        ob = torch.empty(max(n_peers, 1), dtype=torch.int64, device=self.dev)
        cnt = torch.zeros(64, dtype=torch.uint8, device=self.dev)
        start = torch.full((max(n_peers, 1),), -1, dtype=torch.int32, device=self.dev)
        cursor = start.clone()

        def count():
            r.peer_budget_device(po.data_ptr(), msgs.data_ptr() if n else None, n_peers, n, mpos.data_ptr(), n_msgs,
                                 ppos.data_ptr(), ppos.shape[0], k, None, ko.data_ptr(), km.data_ptr() if n else None,
                                 kcnt.data_ptr())

        def rotate(with_sizes):
            r.peer_rotate_device(po.data_ptr(), msgs.data_ptr() if n else None, n_peers, n, ko.data_ptr(),
                                 km.data_ptr() if n else None, n, msize32.data_ptr() if with_sizes else None,
                                 n_msgs if with_sizes else 0, R, None, v, None, cursor.data_ptr(), oo.data_ptr(),
                                 om.data_ptr() if n else None, ob.data_ptr() if with_sizes else None, cnt.data_ptr())

        self.sync()
        count()
        self.sync()
        kc = kcnt.cpu().numpy().view(abi.BUDGET_COUNTERS_DTYPE)[0]
        assert kc["error"] == 0 and int(kc["n_in"]) == n
        n_kept = int(kc["n_kept"])
        res = {"peers": n_peers, "elements": n, "k": k, "r": R, "v": v, "kept_in": n_kept,
               "rows_cut": int(kc["rows_cut"]), "longest_row": int((po[1:] - po[:-1]).max().item()) if n_peers else 0}
        checks = {}
        with_composite = "composite" in self.forms and composite_ok
        if "composite" in self.forms and not composite_ok:
            res["composite"] = "not measured at this size (see composite_scale)"
        host = None
        if n <= self.a.host_check_elements:
            host = (self.host_u32(po), self.host_u32(msgs, n), self.host_u32(ko), self.host_u32(km, n_kept))
        for with_sizes in (False, True):
            tag = "hip_sizes" if with_sizes else "hip"
            cursor.copy_(start)
            self.sync()
            rotate(with_sizes)
            self.sync()
            c = cnt.cpu().numpy().view(abi.ROTATE_COUNTERS_DTYPE)[0]
            assert c["error"] == 0 and int(c["n_in"]) == n and int(c["n_kept_in"]) == n_kept, (tag, c)
            n_out = int(c["n_out"])
            res[tag + "_counters"] = {f: int(c[f]) for f in abi.ROTATE_COUNTERS_DTYPE.names if f != "pad_"}
            first = (oo.clone(), om[:n_out].clone(), cursor.clone(), ob.clone() if with_sizes else None)
            if with_composite:
                t = self.composite_rotate(po, msgs, n, ko, km, start, R, msize if with_sizes else None, v)
                checks[tag + "_equals_composite"] = bool(
                    len(t[1]) == n_out and torch.equal(t[0], oo) and torch.equal(t[1], om[:n_out])
                    and torch.equal(t[2][:n_peers], cursor[:n_peers])
                    and (not with_sizes or torch.equal(t[3], ob[:n_peers])))
                del t
            if host is not None:
                h_cursor = np.full(n_peers, 0xFFFFFFFF, np.uint32)
                w_oo, w_om, w_ob, w_cnt = self.interest.peer_rotate_np(
                    host[0], host[1], host[2], host[3], h_cursor, r=R, msg_size=sizes if with_sizes else None, v=v)
                checks[tag + "_equals_peer_rotate_np"] = bool(
                    self.host_u32(oo).tobytes() == w_oo.tobytes() and self.host_u32(om, n_out).tobytes() == w_om.tobytes()
                    and self.host_u32(cursor, n_peers).tobytes() == h_cursor.tobytes()
                    and (not with_sizes or ob[:n_peers].cpu().numpy().view(np.uint64).tobytes() == w_ob.tobytes())
                    and {f: int(c[f]) for f in w_cnt} == {f: int(x) for f, x in w_cnt.items()})
            cursor.copy_(start)
            self.sync()
            rotate(with_sizes)
            self.sync()
            checks[tag + "_deterministic"] = bool(
                torch.equal(first[0], oo) and torch.equal(first[1], om[:n_out]) and torch.equal(first[2], cursor)
                and (not with_sizes or torch.equal(first[3], ob)))
            del first
        res["checks"] = checks
        assert all(checks.values()), checks
        fns = {}
        if "hip" in self.forms:
            fns["hip"] = lambda: rotate(False)
        if "hip_sizes" in self.forms:
            fns["hip_sizes"] = lambda: rotate(True)
        if "count" in self.forms:
            fns["count"] = count     # rewrites the same kept CSR between the rotate calls
        if with_composite:
            fns["composite"] = lambda: self.composite_rotate(po, msgs, n, ko, km, cursor, R)
            if "composite_sizes" in self.forms:
                fns["composite_sizes"] = lambda: self.composite_rotate(po, msgs, n, ko, km, cursor, R, msize, v)
        cursor.copy_(start)
        for fn in fns.values():
            for _ in range(self.a.warmup):
                fn()
        times = {f: [] for f in fns}
        for _ in range(self.a.reps):  # alternating
            for f, fn in fns.items():
                times[f] += self.timed(fn, 1)
        res["times"] = {f: summary(v_) for f, v_ in times.items()}
        # what the call must move: both lists, both offset arrays and the cursors in; the offsets, the
        # output list and the cursors out; with sizes a 4-byte gather per element and the per-row bytes
        n_out = res["hip_counters"]["n_out"]
        nbytes = 4 * n + 4 * n_kept + 8 * (n_peers + 1) + 4 * n_peers + 4 * (n_peers + 1) + 4 * n_out + 4 * n_peers
        res["must_move_bytes"] = nbytes
        res["must_move_bytes_sizes"] = nbytes + 4 * n + 8 * n_peers
        mean = {f: statistics.fmean(t) for f, t in times.items()}
        if "hip" in mean:
            res["hip_frac_of_8TBps"] = round(nbytes / (mean["hip"] / 1e3) / HBM_PEAK, 4)
        if "hip_sizes" in mean:
            res["hip_sizes_frac_of_8TBps"] = round(res["must_move_bytes_sizes"] / (mean["hip_sizes"] / 1e3) / HBM_PEAK, 4)
        for a_, b_ in (("hip", "count"), ("hip_sizes", "count"), ("composite", "hip"), ("composite_sizes", "hip_sizes")):
            if a_ in mean and b_ in mean:
                res[f"{a_}_over_{b_}"] = round(mean[a_] / mean[b_], 3)
        print(f"[{name}] " + json.dumps(res), flush=True)
        del msize, msize32, oo, om, ob, ko, km, cursor, start
        torch.cuda.empty_cache()
        return res

    def shape_i(self):
        """The count bench's shape i with K = 1 only (K = 32 cuts no C5 row: nothing to rotate)."""
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
        out = {"k1": self.run(r, "i_k1", po, rows, P, pos, pos, 1)}
        r.close()
        return out

    def shape_iii(self):
        """One 16M-element row against the same elements, 16 per row: message j is element j, so every
        row ascends. K is half the row in both."""
        from worldql_server_amd.router import Router
        torch = self.torch
        n_rows = max(2, int(round(1_000_000 * self.a.scale))) + 1
        per = 16
        P = per * (n_rows - 1)
        rng = np.random.default_rng(5)
        mpos = torch.from_numpy(rng.uniform(-1024.0, 1024.0, (P, 3))).to(self.dev)
        ppos = torch.from_numpy(rng.uniform(-1024.0, 1024.0, (n_rows, 3))).to(self.dev)
        msgs = self.dev_u32(np.arange(P, dtype=np.uint32))
        one = np.zeros(n_rows + 1, np.uint32)
        one[n_rows // 2 + 1:] = P                                  # all of it in row n_rows / 2
        even = np.zeros(n_rows + 1, np.uint32)
        even[1:n_rows] = per * np.arange(1, n_rows, dtype=np.uint32)   # 16 per row, the last row empty
        even[n_rows] = P
        r = Router(16, 0)
        d_one, d_even = self.dev_u32(one), self.dev_u32(even)
        self.sync()
        res_one = self.run(r, "iii_one_row", d_one, msgs, P, mpos, ppos, P // 2)
        res_even = self.run(r, "iii_spread", d_even, msgs, P, mpos, ppos, per // 2)
        r.close()
        out = {"one_row": res_one, "spread": res_even}
        for f in ("hip", "hip_sizes"):
            if f in res_one["times"] and f in res_even["times"]:
                out[f + "_one_row_over_spread"] = round(res_one["times"][f]["mean_ms"] / res_even["times"][f]["mean_ms"], 3)
        return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--composite-scale", type=float, default=1.0,
                    help="shape ii: the largest scale at which the composite's buffers fit")
    ap.add_argument("--only", default="i,ii,iii")
    ap.add_argument("--forms", default="hip,hip_sizes,composite,composite_sizes,count")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-check-elements", type=int, default=3_000_000)
    ap.add_argument("--append", action="store_true", help="keep the shapes an earlier run wrote to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peer_rotate_bench.json"))
    a = ap.parse_args()
    b = RotateBench(a)
    only = a.only.split(",")
    out = {"tool": "tools/peer_rotate_bench.py", "scale": a.scale, "composite_scale": a.composite_scale,
           "reps": a.reps, "warmup": a.warmup, "forms": b.forms, "r": R,
           "timing": "host clock, a device synchronise on both sides of every repeat",
           "sizes": "per message, seed 11: 96% uniform 100 - 200 B, 4% uniform 2,048 - 16,384 B; V = R x the mean size",
           "must_move": "reads 4 n (the list) + 4 kept_in (the kept list) + 8 (n_peers + 1) (both offsets) + "
                        "4 n_peers (cursors), writes 4 (n_peers + 1) + 4 n_out + 4 n_peers; with sizes 4 n "
                        "(a size gather) and 8 n_peers more; share of 8 TB/s",
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
