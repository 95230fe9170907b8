#!/usr/bin/env python3
"""The frame builder (wq_frames_build_device, csrc/wq_frames.hip) against the path it replaces and
against a copy, in one process, the forms alternating:

  hip    Router.build_frames_device with d_frame_size and the counters: sizes / one u64 scan / the copy
         over the output bytes, asynchronous, no read-back;
  host   the path it replaces: wq_serialize_messages over a prepared wq_message_in array on --threads
         host threads straight into pinned memory, the sizes from the offsets (interest.frame_sizes),
         then the upload of frames, offsets and sizes on the handle's stream. Filling the
         wq_message_in array is not timed;
  copy   a device-to-device copy of bytes_need bytes on the same stream: the floor (it reads and writes
         every output byte once and does nothing else).

Shapes:
  c5        the C5 tick's entity updates: 1M messages with a position and a 5-byte world name,
            instruction 7, 136 bytes each;
  mix_1m    the pack bench's mix through flex: per message (seed 11) 96% 100 - 200 B and 4% 2 - 16 KB,
  mix_10m   the flex length chosen so that a frame without a position has that size (frames below 124
            bytes get an empty flex), at 1M and 10M messages; `host` only up to --host-messages;
  one_flex  one message with a 256 MiB flex against the same payload bytes spread over 1M messages.

The hip output is checked equal to the host serializer's (up to --host-messages messages) and
byte-identical on a second call before anything is timed. Then --warmup untimed and --reps timed repeats
per form, a synchronise on both sides of each; min / mean / max are reported with every number.
bytes_moved is what the call must read and write once: the frames, the payload bytes, per message the
uuid, the world id, the position, the payload offsets, and the offsets and sizes it writes.

    python tools/frames_build_bench.py [--scale 1.0] [--only c5,mix_1m,mix_10m,one_flex] [--forms hip,host,copy]
                                       [--reps 7] [--warmup 3] [--threads 16] [--out profiles/frames_build_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
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

HBM_BYTES_PER_S = 8e12
WORLD = b"world"
# struct wq_message_in (include/wq_codec.h), 128 bytes
MESSAGE_IN = np.dtype({"names": ["instruction", "replication", "has_position", "has_parameter", "has_flex", "sender_uuid",
                                 "position", "parameter", "parameter_len", "world_name", "world_len", "flex", "flex_len",
                                 "records", "n_records", "entities", "n_entities"],
                       "formats": [np.uint8] * 5 + [(np.uint8, 16), (np.float64, 3)] + [np.uint64] * 10,
                       "offsets": [0, 1, 2, 3, 4, 8, 24, 48, 56, 64, 72, 80, 88, 96, 104, 112, 120], "itemsize": 128})


class FramesBench(Bench):
    def run(self, name, n, pos, flex_lens, host=True):
        """n messages in world 0 ("world"), instruction 7; pos: n x 3 f64 or None; flex_lens: n lengths or None."""
        from worldql_server_amd import codec, interest
        from worldql_server_amd.router import Router
        torch, abi = self.torch, self.abi
        r = Router(16, 0)
        r.set_worlds([WORLD])
        stream = torch.cuda.Stream(device=self.dev)      # the handle's stream, so that the copies run on it too
        self.sync()
        r.set_stream(stream.cuda_stream)
        rng = np.random.default_rng(3)
        uuid = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        d_uuid = torch.from_numpy(uuid).to(self.dev)
        d_world = torch.zeros(n, dtype=torch.int32, device=self.dev)
        d_pos = torch.from_numpy(pos).to(self.dev) if pos is not None else None
        d_flex = d_fo = None
        n_flex = 0
        if flex_lens is not None:
            fo = np.zeros(n + 1, np.uint64)
            np.cumsum(flex_lens.astype(np.uint64), out=fo[1:])
            n_flex = int(fo[-1])
            block = torch.randint(0, 256, (min(max(n_flex, 1), 1 << 26),), dtype=torch.uint8, device=self.dev,
                                  generator=torch.Generator(device=self.dev).manual_seed(7))
            d_flex = block.repeat((n_flex + block.numel() - 1) // block.numel())[:max(n_flex, 1)].contiguous()
            d_fo = torch.from_numpy(fo.view(np.int64)).to(self.dev)
        src = abi.FramesSrc(instruction=None, instruction_all=7, replication=None, replication_all=0,
                            sender_uuid=d_uuid.data_ptr(), world=d_world.data_ptr(),
                            pos=d_pos.data_ptr() if d_pos is not None else None, param=None, param_offsets=None,
                            n_param_bytes=0, flex=d_flex.data_ptr() if d_flex is not None else None,
                            flex_offsets=d_fo.data_ptr() if d_fo is not None else None, n_flex_bytes=n_flex, msg_flags=None)
        off = torch.empty(n + 1, dtype=torch.int64, device=self.dev)
        size = torch.empty(n, dtype=torch.int32, device=self.dev)
        cnt = torch.zeros(40, dtype=torch.uint8, device=self.dev)

        def call(out, cap):
            r.build_frames_device(src, n, out.data_ptr() if cap else None, cap, off.data_ptr(), size.data_ptr(), cnt.data_ptr())

        self.sync()
        call(None, 0)                                         # the sizing call
        self.sync()
        c = cnt.cpu().numpy().view(abi.FRAMES_COUNTERS_DTYPE)[0]
        assert c["error"] == 0 and int(c["n_frames"]) == n
        need = int(c["bytes_need"])
        moved = need + n_flex + n * (16 + 4 + (24 if pos is not None else 0) + (8 if d_fo is not None else 0) + 8 + 4)
        res = {"messages": n, "bytes_need": need, "flex_bytes": n_flex, "bytes_moved": moved,
               "mean_frame": round(need / max(n, 1), 1), "largest_flex": int(flex_lens.max()) if flex_lens is not None else 0}
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
        c = cnt.cpu().numpy().view(abi.FRAMES_COUNTERS_DTYPE)[0]
        assert c["overflow"] == 0 and int(c["bytes_written"]) == need and int(c["n_complete"]) == n
        checks = {}
        fns = {"hip": hip}
        with_host = host and "host" in self.forms and n <= self.a.host_messages
        if with_host:
            lib = codec._lib()
            h_flex = d_flex.cpu().numpy() if d_flex is not None else None
            world_buf = ctypes.create_string_buffer(WORLD)
            m = np.zeros(n, MESSAGE_IN)
            m["instruction"], m["sender_uuid"] = 7, uuid
            m["world_name"], m["world_len"] = ctypes.addressof(world_buf), len(WORLD)
            if pos is not None:
                m["has_position"], m["position"] = 1, pos
            if h_flex is not None:
                m["has_flex"], m["flex"], m["flex_len"] = 1, np.uint64(h_flex.ctypes.data) + fo[:-1], flex_lens
            cap = int(lib.wq_serialize_bound(m.ctypes.data, n))
            p_frames = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            p_off = torch.empty(n + 1, dtype=torch.int64, pin_memory=True)
            p_size = torch.empty(n, dtype=torch.int32, pin_memory=True)
            u_frames = torch.empty(max(need, 16), dtype=torch.uint8, device=self.dev)
            u_off, u_size = torch.empty_like(off), torch.empty_like(size)
            h_off = p_off.numpy().view(np.uint64)

            def host():
                rc = lib.wq_serialize_messages(m.ctypes.data, n, p_frames.data_ptr(), cap, p_off.data_ptr(), self.a.threads)
                assert rc == 0, rc
                p_size.numpy().view(np.uint32)[:] = interest.frame_sizes(h_off)
                with torch.cuda.stream(stream):
                    u_frames[:need].copy_(p_frames[:need], non_blocking=True)
                    u_off.copy_(p_off, non_blocking=True)
                    u_size.copy_(p_size, non_blocking=True)

            self.sync()
            host()
            self.sync()
            checks["hip_equals_host_serializer"] = bool(int(h_off[n]) == need and torch.equal(u_frames[:need], out[:need])
                                                        and torch.equal(u_off, off) and torch.equal(u_size, size))
            fns["host"] = host
        elif host and "host" in self.forms:
            res["host"] = f"not measured: more than --host-messages = {self.a.host_messages} messages"
        first = out[:need].clone()
        out.zero_()
        self.sync()                                           # zero_ runs on torch's stream, the call on the handle's
        hip()
        self.sync()
        checks["hip_deterministic"] = bool(torch.equal(first, out[:need]))
        del first
        res["checks"] = checks
        assert all(checks.values()), checks
        if "copy" in self.forms:
            fns["copy"] = copy
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
        res["hip_moved_GBps"] = round(moved / (hip_ms / 1e3) / 1e9, 1)
        res["hip_fraction_of_8TBps"] = round(moved / (hip_ms / 1e3) / HBM_BYTES_PER_S, 4)
        if "copy" in times:
            res["hip_over_copy"] = round(hip_ms / statistics.fmean(times["copy"]), 3)
            res["copy_GBps"] = round(need / (statistics.fmean(times["copy"]) / 1e3) / 1e9, 1)
        if "host" in times:
            res["host_over_hip"] = round(statistics.fmean(times["host"]) / hip_ms, 2)
            res["host_threads"] = self.a.threads
        print(f"[{name}] " + json.dumps(res), flush=True)
        self.sync()
        r.set_stream(None)
        r.close()
        torch.cuda.empty_cache()
        return res

    # ---- shapes ----
    def scaled(self, n):
        return max(2, int(round(n * self.a.scale)))

    def shape_c5(self):
        n = self.scaled(1_000_000)
        pos = np.random.default_rng(5).uniform(-5000, 5000, (n, 3))
        return self.run("c5", n, pos, None)

    def mix(self, name, n):
        lens = np.maximum(frame_mix(n).astype(np.int64) - 124, 0)
        return self.run(name, n, None, lens)

    def shape_mix_1m(self):
        return self.mix("mix_1m", self.scaled(1_000_000))

    def shape_mix_10m(self):
        return self.mix("mix_10m", self.scaled(10_000_000))

    def shape_one_flex(self):
        n = self.scaled(1_000_000)
        per = 256
        one = np.zeros(n, np.int64)
        one[n // 2] = per * n                                   # 256 MiB at full scale, all of it in one message
        res_one = self.run("one_flex", n, None, one, host=False)
        res_even = self.run("one_flex_spread", n, None, np.full(n, per, np.int64), host=False)
        ratio = res_one["times"]["hip"]["mean_ms"] / res_even["times"]["hip"]["mean_ms"]
        return {"one_message": res_one, "spread": res_even, "hip_one_message_over_spread": round(ratio, 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default="c5,mix_1m,mix_10m,one_flex")
    ap.add_argument("--forms", default="hip,host,copy")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-messages", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_build_bench.json"))
    a = ap.parse_args()
    b = FramesBench(a)
    only = a.only.split(",")
    out = {"tool": "tools/frames_build_bench.py", "scale": a.scale, "reps": a.reps, "warmup": a.warmup, "forms": b.forms,
           "timing": "host clock, a device synchronise on both sides of every repeat",
           "host": f"wq_serialize_messages on {a.threads} threads into pinned memory, sizes from the offsets, upload of "
                   "frames, offsets and sizes on the handle's stream; filling wq_message_in is not timed",
           "copy": "device-to-device copy of bytes_need bytes on the handle's stream",
           "shapes": {}}
    ok = True
    for name in ("c5", "mix_1m", "one_flex", "mix_10m"):
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
