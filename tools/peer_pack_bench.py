#!/usr/bin/env python3
"""The send buffers (wq_peer_pack_device, csrc/wq_pack.hip) against two yardsticks in one process, the
forms alternating:

  hip        Router.peer_pack_device with d_out_elem_bytes and the counters: rows / sizes / one u64 scan /
             offsets / the copy over the output bytes, asynchronous, no read-back;
  copy       a device-to-device copy of bytes_written bytes on the same stream: the floor any pack can
             approach (it reads and writes every output byte once and does nothing else);
  composite  torch on the same device arrays: the record sizes of the list, their cumulative sum E, a
             searchsorted of every output byte's index over E, and one byte gather from the frames (the
             prefix bytes from the sizes). Its index alone is 8 bytes per output byte and the whole
             takes about 56, so it runs only where that fits in the device's free memory.

Shapes (the set-up of tools/peer_budget_bench.py; frames of tools/peer_budget_bytes_bench.py's mix,
96% 100 - 200 B and 4% 2 - 16 KB per message, contiguous as wq_serialize_messages leaves them):
  i    the C5 tick transposed, after wq_peer_budget_bytes_device at W = 16 KB;
  ii   the C3 tick transposed, after a byte budget with W = 16 KB per peer, so that the packed output
       of 1M peers is at most 16 GiB (W and bytes_need are recorded);
  iii  one 16M-element row against the same elements spread over 1M rows, packed as they are;
  iv   shape i with the length prefix on.

The hip output is checked equal to the composite's (and to interest.peer_pack_np where the elements
fit --host-check-elements) and byte-identical on a second call before anything is timed. Then --warmup
untimed and --reps timed repeats per form, a synchronise on both sides of each; min / mean / max are
reported with every number.

    python tools/peer_pack_bench.py [--scale 1.0] [--only i,ii,iii,iv] [--forms hip,copy,composite]
                                    [--reps 7] [--warmup 3] [--append] [--out profiles/peer_pack_bench.json]
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

from peer_budget_bench import Bench, summary  # noqa: E402
from peer_budget_bytes_bench import frame_mix  # noqa: E402

W_BYTES = 16384


class PackBench(Bench):
    prefix = False
    budget_w = W_BYTES   # None: pack the lists as they are

    def frames_for(self, n_msgs):
        """(frames u8, frame_offsets i64 holding the u64 values, sizes) on the device."""
        torch = self.torch
        sizes = frame_mix(n_msgs)
        fo = np.zeros(n_msgs + 1, np.uint64)
        np.cumsum(sizes.astype(np.uint64), out=fo[1:])
        total = int(fo[-1])
        block = torch.randint(0, 256, (min(max(total, 1), 1 << 26),), dtype=torch.uint8, device=self.dev,
                              generator=torch.Generator(device=self.dev).manual_seed(7))
        frames = block.repeat((total + block.numel() - 1) // block.numel())[:total].contiguous()
        return frames, torch.from_numpy(fo.view(np.int64)).to(self.dev), sizes

    def composite_pack(self, po, msgs, n, frames, fo, prefix):
        """The torch baseline: (out bytes, E[n + 1])."""
        torch = self.torch
        m = msgs[:n].long()
        size = fo[m + 1] - fo[m]
        pre = 4 if prefix else 0
        E = torch.zeros(n + 1, dtype=torch.int64, device=self.dev)
        torch.cumsum(size + pre, 0, out=E[1:])
        total = int(E[n].item())
        idx = torch.arange(total, dtype=torch.int64, device=self.dev)
        q = torch.searchsorted(E[1:], idx, right=True)
        within = idx - E[q]
        if not prefix:
            return frames[fo[m[q]] + within], E
        body = frames[(fo[m[q]] + (within - 4)).clamp_(min=0)]
        head = ((size[q] >> (8 * within.clamp(max=3))) & 255).to(torch.uint8)
        return torch.where(within < 4, head, body), E

    def run(self, r, name, po, msgs, n, mpos, ppos, k=None, composite_ok=True):
        """po[n_peers + 1], msgs[n] (int32 device tensors). With budget_w the lists first go through
        wq_peer_budget_bytes_device at that W; k is the count bench's K and is not used."""
        torch, abi = self.torch, self.abi
        n_peers, n_msgs = po.numel() - 1, mpos.shape[0]
        stream = torch.cuda.Stream(device=self.dev)      # the handle's stream, so that the copy runs on it too
        self.sync()
        r.set_stream(stream.cuda_stream)
        frames, fo, sizes = self.frames_for(n_msgs)
        n_frame_bytes = frames.numel()
        res = {"peers": n_peers, "elements_in": n, "prefix": self.prefix, "frame_bytes": n_frame_bytes}
        if self.budget_w is not None:
            msize = self.dev_u32(sizes)
            oo, om = self.i32(n_peers + 1), self.i32(n)
            bcnt = torch.zeros(40, dtype=torch.uint8, device=self.dev)
            self.sync()
            r.peer_budget_bytes_device(po.data_ptr(), msgs.data_ptr(), n_peers, n, mpos.data_ptr(), msize.data_ptr(), n_msgs,
                                       ppos.data_ptr(), ppos.shape[0], self.budget_w, None, oo.data_ptr(), om.data_ptr(),
                                       None, bcnt.data_ptr())
            self.sync()
            bc = bcnt.cpu().numpy().view(abi.BUDGET_BYTES_COUNTERS_DTYPE)[0]
            assert bc["error"] == 0
            n = int(bc["n_kept"])
            po, msgs = oo, om[:n].clone()
            res.update(w=self.budget_w, rows_cut=int(bc["rows_cut"]), budget_bytes_kept=int(bc["bytes_kept"]))
            del om, msize
            torch.cuda.empty_cache()
        res["elements"] = n
        flags = abi.PACK_LEN_PREFIX if self.prefix else 0
        pb = torch.empty(n_peers + 1, dtype=torch.int64, device=self.dev)
        eb = torch.empty(max(n, 1), dtype=torch.int64, device=self.dev)
        cnt = torch.zeros(40, dtype=torch.uint8, device=self.dev)

        def call(out, cap):
            r.peer_pack_device(po.data_ptr(), msgs.data_ptr() if n else None, n_peers, n, frames.data_ptr(), fo.data_ptr(),
                               n_msgs, n_frame_bytes, flags, out.data_ptr() if cap else None, cap, pb.data_ptr(),
                               eb.data_ptr() if n else None, cnt.data_ptr())

        self.sync()
        call(pb, 0)                                           # the sizing call
        self.sync()
        c = cnt.cpu().numpy().view(abi.PACK_COUNTERS_DTYPE)[0]
        assert c["error"] == 0 and int(c["n_in"]) == n, (int(c["error"]), int(c["n_in"]), n)
        need = int(c["bytes_need"])
        res.update(bytes_need=need, longest_row=int((po[1:] - po[:-1]).max().item()) if n_peers else 0)
        if self.budget_w is not None and not self.prefix:
            assert need == res["budget_bytes_kept"], "d_out_bytes sizes the send buffers"
        out = torch.empty(max(need, 16), dtype=torch.uint8, device=self.dev)
        dst = torch.empty(max(need, 16), dtype=torch.uint8, device=self.dev)

        def hip():
            call(out, need)

        def copy():
            with torch.cuda.stream(stream):
                dst[:need].copy_(out[:need], non_blocking=True)

        self.sync()
        hip()
        self.sync()
        c = cnt.cpu().numpy().view(abi.PACK_COUNTERS_DTYPE)[0]
        assert c["overflow"] == 0 and int(c["bytes_written"]) == need and int(c["n_complete"]) == n
        checks = {}
        free = torch.cuda.mem_get_info()[0]
        with_composite = "composite" in self.forms and composite_ok and 56 * need + 32 * n < 0.8 * free
        if with_composite:
            t_out, t_E = self.composite_pack(po, msgs, n, frames, fo, self.prefix)
            checks["hip_equals_composite"] = bool(torch.equal(t_out, out[:need]) and torch.equal(t_E[:n], eb[:n])
                                                  and torch.equal(t_E[po.long()], pb))
            del t_out, t_E
        elif "composite" in self.forms:
            res["composite"] = "not measured: its index and gather buffers (about 56 bytes per output byte) do not fit"
        if n <= self.a.host_check_elements and need <= 1 << 31:
            w = self.interest.peer_pack_np(self.host_u32(po), self.host_u32(msgs, n), frames.cpu().numpy(),
                                           fo.cpu().numpy().view(np.uint64), len_prefix=self.prefix)
            checks["hip_equals_peer_pack_np"] = bool(out[:need].cpu().numpy().tobytes() == w[0].tobytes()
                                                     and pb.cpu().numpy().view(np.uint64).tobytes() == w[1].tobytes()
                                                     and {f: int(c[f]) for f in w[3]} == w[3])
        first = out[:need].clone()
        out.zero_()
        self.sync()                                           # zero_ runs on torch's stream, the call on the handle's
        hip()
        self.sync()
        checks["hip_deterministic"] = bool(torch.equal(first, out[:need]))
        del first
        res["checks"] = checks
        assert all(checks.values()), checks
        fns = {"hip": hip}
        if "copy" in self.forms:
            fns["copy"] = copy
        if with_composite:
            fns["composite"] = lambda: self.composite_pack(po, msgs, n, frames, fo, self.prefix)
        for fn in fns.values():
            for _ in range(self.a.warmup):
                fn()
        times = {f: [] for f in fns}
        for _ in range(self.a.reps):  # alternating
            for f, fn in fns.items():
                times[f] += self.timed(fn, 1)
        res["times"] = {f: summary(v) for f, v in times.items()}
        hip_ms = statistics.fmean(times["hip"])
        res["hip_output_GBps"] = round(need / (hip_ms / 1e3) / 1e9, 1)
        if "copy" in times:
            res["hip_over_copy"] = round(hip_ms / statistics.fmean(times["copy"]), 3)
            res["copy_GBps"] = round(need / (statistics.fmean(times["copy"]) / 1e3) / 1e9, 1)
        if "composite" in times:
            res["composite_over_hip"] = round(statistics.fmean(times["composite"]) / hip_ms, 3)
            res["bar_hip_max_below_composite_min"] = bool(max(times["hip"]) < min(times["composite"]))
        print(f"[{name}] " + json.dumps(res), flush=True)
        self.sync()
        r.set_stream(None)
        del out, dst, frames, fo, pb, eb
        torch.cuda.empty_cache()
        return res

    # ---- shapes ----
    def shape_i(self, prefix=False):
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
        self.prefix, self.budget_w = prefix, W_BYTES
        out = self.run(r, "iv" if prefix else "i", po, rows, P, pos, pos)
        self.prefix = False
        r.close()
        return out

    def shape_iv(self):
        return self.shape_i(prefix=True)

    def shape_ii(self):
        self.prefix, self.budget_w = False, W_BYTES
        return super().shape_ii()          # the C3 set-up of tools/peer_budget_bench.py; run() is this class's

    def shape_iii(self):
        from worldql_server_amd.router import Router
        torch = self.torch
        n_rows = max(2, int(round(1_000_000 * self.a.scale))) + 1
        per = 16
        P = per * (n_rows - 1)
        rng = np.random.default_rng(5)
        mpos = torch.zeros(n_rows, 3, dtype=torch.float64, device=self.dev)     # only its length is used
        msgs = self.dev_u32(rng.integers(0, n_rows, size=P))
        one = np.zeros(n_rows + 1, np.uint32)
        one[n_rows // 2 + 1:] = P                                  # all of it in row n_rows / 2
        even = np.zeros(n_rows + 1, np.uint32)
        even[1:n_rows] = per * np.arange(1, n_rows, dtype=np.uint32)   # 16 per row, the last row empty
        even[n_rows] = P
        r = Router(16, 0)
        d_one, d_even = self.dev_u32(one), self.dev_u32(even)
        self.sync()
        self.prefix, self.budget_w = False, None
        res_one = self.run(r, "iii_one_row", d_one, msgs, P, mpos, mpos)
        res_even = self.run(r, "iii_spread", d_even, msgs, P, mpos, mpos)
        r.close()
        ratio = res_one["times"]["hip"]["mean_ms"] / res_even["times"]["hip"]["mean_ms"]
        return {"one_row": res_one, "spread": res_even, "hip_one_row_over_spread": round(ratio, 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--composite-scale", type=float, default=1.0, help="shape ii: as tools/peer_budget_bench.py")
    ap.add_argument("--only", default="i,ii,iii,iv")
    ap.add_argument("--forms", default="hip,copy,composite")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-check-elements", type=int, default=300_000)
    ap.add_argument("--append", action="store_true", help="keep the shapes an earlier run wrote to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peer_pack_bench.json"))
    a = ap.parse_args()
    b = PackBench(a)
    only = a.only.split(",")
    out = {"tool": "tools/peer_pack_bench.py", "scale": a.scale, "reps": a.reps, "warmup": a.warmup, "forms": b.forms,
           "timing": "host clock, a device synchronise on both sides of every repeat",
           "frames": "per message, seed 11: 96% uniform 100 - 200 B, 4% uniform 2,048 - 16,384 B, contiguous",
           "copy": "device-to-device copy of bytes_written bytes on the handle's stream",
           "composite": "sizes, cumsum, searchsorted of every output byte over E, one byte gather; only where "
                        "about 56 bytes per output byte fit in the free device memory",
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

    for name, fn in (("i", b.shape_i), ("iv", b.shape_iv), ("iii", b.shape_iii), ("ii", b.shape_ii)):
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
