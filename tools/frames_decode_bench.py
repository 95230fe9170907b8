#!/usr/bin/env python3
"""The ingest decoder (wq_frames_decode_device, csrc/wq_decode.hip) against the path it replaces and
against a copy, in one process, the forms alternating:

  hip          Router.decode_frames_device on frames already in device memory, every output and the
               counters, asynchronous, no read-back;
  hip_upload   the same behind the upload of the raw frames and their offsets from pinned memory;
  host         the path it replaces: wq_decode_messages on --threads host threads, then per message the
               world (sanitize + intern through a dict, as processing.py does) and the sender (a sorted
               table), then filling and uploading pos / world / sender / repl;
  host_decode  wq_decode_messages alone, the C part of `host`;
  copy         a device-to-device copy of the frame bytes on the same stream: the floor.

The frames are built on the device by wq_frames_build_device (flat shapes) or replicated from one
host-serialized frame (records). Shapes:
  c5           1M frames of 136 B (a position, a 5-byte world name);
  mix          the pack bench's mix through flex: 96% 100 - 200 B, 4% 2 - 16 KB; 1M frames;
  mix_corrupt  the same with one byte changed in 30% of the frames;
  one_flex     one 256 MiB flex among 1M small frames, against the same bytes spread;
  big_params   256 parameters of 1 MiB, against the same bytes as 256 B per message: the long-string ratio;
  records      10,000 frames of 100 records each;
  set_peers    wq_ingest_set_peers at 1M peers (host sort, upload, wait).

hip's msg array is checked equal to wq_decode_messages' and its world / sender arrays to the host
resolution, and a second call byte-identical, before anything is timed. Then --warmup untimed and --reps
timed repeats per form (host: --host-reps), a synchronise on both sides of each; min / mean / max with
every number. bytes_moved is what the call must read and write once: the frame bytes it has to look at
(structure and strings, not flex payloads), the offsets, and its outputs.

    python tools/frames_decode_bench.py [--scale 1.0] [--only c5,mix,...] [--forms hip,hip_upload,host,host_decode,copy]
                                        [--reps 7] [--warmup 3] [--threads 16] [--out profiles/frames_decode_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import traceback
import uuid

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from peer_budget_bench import Bench, summary  # noqa: E402
from peer_budget_bytes_bench import frame_mix  # noqa: E402

HBM_BYTES_PER_S = 8e12
WORLDS = ["world", "nether", "the_end"]
N_PEERS = 4096
OUT_BYTES = 72 + 24 + 4 + 4 + 1 + 1 + 16 + 8 + 1


class DecodeBench(Bench):
    def build(self, n, pos=None, param_lens=None, flex_lens=None):
        """n flat frames on the device through the builder: (frames u8, offsets i64)."""
        from worldql_server_amd.router import Router
        torch, abi = self.torch, self.abi
        r = Router(16, 0)
        r.set_worlds(WORLDS)
        rng = np.random.default_rng(3)
        uuids = self.peers[rng.integers(0, int(N_PEERS * 1.1), n) % len(self.peers)]   # a tenth are unknown senders
        keep = {"uuid": torch.from_numpy(uuids).to(self.dev),
                "world": torch.from_numpy(rng.integers(0, 3, n).astype(np.int32)).to(self.dev)}
        src = dict(instruction=None, instruction_all=7, replication=None, replication_all=0, sender_uuid=keep["uuid"].data_ptr(),
                   world=keep["world"].data_ptr(), pos=None, param=None, param_offsets=None, n_param_bytes=0, flex=None,
                   flex_offsets=None, n_flex_bytes=0, msg_flags=None)
        if pos is not None:
            keep["pos"] = torch.from_numpy(pos).to(self.dev)
            src["pos"] = keep["pos"].data_ptr()
        for key, lens, ascii_only in (("param", param_lens, True), ("flex", flex_lens, False)):
            if lens is None:
                continue
            off = np.zeros(n + 1, np.uint64)
            np.cumsum(lens.astype(np.uint64), out=off[1:])
            total = int(off[-1])
            block = torch.randint(97, 123, (1 << 22,), dtype=torch.uint8, device=self.dev) if ascii_only else \
                torch.randint(0, 256, (1 << 22,), dtype=torch.uint8, device=self.dev)
            keep[key] = block.repeat((total + block.numel() - 1) // block.numel() + 1)[:max(total, 1)].contiguous()
            keep[key + "_off"] = torch.from_numpy(off.view(np.int64)).to(self.dev)
            src[key], src[key + "_offsets"], src["n_" + key + "_bytes"] = keep[key].data_ptr(), keep[key + "_off"].data_ptr(), total
        s = abi.FramesSrc(**src)
        off = torch.empty(n + 1, dtype=torch.int64, device=self.dev)
        cnt = torch.zeros(40, dtype=torch.uint8, device=self.dev)
        self.sync()
        r.build_frames_device(s, n, None, 0, off.data_ptr(), None, cnt.data_ptr())
        self.sync()
        need = int(cnt.cpu().numpy().view(abi.FRAMES_COUNTERS_DTYPE)[0]["bytes_need"])
        frames = torch.empty(max(need, 16), dtype=torch.uint8, device=self.dev)
        r.build_frames_device(s, n, frames.data_ptr(), need, off.data_ptr(), None, cnt.data_ptr())
        self.sync()
        assert cnt.cpu().numpy().view(abi.FRAMES_COUNTERS_DTYPE)[0]["error"] == 0
        r.close()
        del keep
        torch.cuda.empty_cache()
        return frames[:need], off

    def run(self, name, frames, off, payload_bytes=0, host_form=True):
        """frames: u8 device tensor of exactly the frame bytes; off: i64 device tensor [n + 1]."""
        from worldql_server_amd import codec, ingest
        from worldql_server_amd.router import Router
        from worldql_server_amd.world_names import SanitizeError, sanitize_world_name
        torch, abi = self.torch, self.abi
        n, nb = off.numel() - 1, frames.numel()
        r = Router(16, 0)
        r.set_worlds(WORLDS)
        r.set_ingest_peers(self.peers[:N_PEERS])
        stream = torch.cuda.Stream(device=self.dev)
        self.sync()
        r.set_stream(stream.cuda_stream)
        tick = ingest.IngestTick(r, capacity=n)
        p_frames = torch.empty(max(nb, 1), dtype=torch.uint8, pin_memory=True)
        p_off = torch.empty(n + 1, dtype=torch.int64, pin_memory=True)
        p_frames[:nb].copy_(frames)
        p_off.copy_(off)
        self.sync()
        u_frames, u_off = torch.empty_like(frames), torch.empty_like(off)

        def hip():
            tick.decode(frames, off)

        def hip_upload():
            with torch.cuda.stream(stream):
                u_frames.copy_(p_frames[:nb], non_blocking=True)
                u_off.copy_(p_off, non_blocking=True)
            tick.decode(u_frames, u_off)

        dst = torch.empty_like(frames)

        def copy():
            with torch.cuda.stream(stream):
                dst.copy_(frames, non_blocking=True)

        h_data, h_off = p_frames.numpy()[:nb], p_off.numpy().view(np.uint64)
        h_msg = np.zeros(n, codec.DECODED_DTYPE)
        lib = codec._lib()

        def host_decode():
            assert lib.wq_decode_messages(h_data.ctypes.data, h_off.ctypes.data, n, h_msg.ctypes.data, self.a.threads) == 0

        world_ids = {w: i for i, w in reversed(list(enumerate(WORLDS)))}
        order = np.lexsort((self.peer_key[:N_PEERS, 1], self.peer_key[:N_PEERS, 0]))
        sorted_keys = self.peer_key[:N_PEERS][order]
        p_out = {k: torch.empty(s, dtype=t, pin_memory=True) for k, s, t in
                 (("pos", (n, 3), torch.float64), ("world", (n,), torch.int32), ("sender", (n,), torch.int32), ("repl", (n,), torch.uint8))}
        d_out = {k: torch.empty_like(v, device=self.dev) for k, v in p_out.items()}
        cache: dict = {}

        def resolve():
            ok = h_msg["status"] == 0
            world = np.full(n, abi.WORLD_INVALID, np.uint32)
            starts = h_off[:-1] + h_msg["world_off"]
            lens = h_msg["world_len"]
            for i in np.flatnonzero(ok):                          # per message, as processing.py: sanitize, intern
                key = h_data[int(starts[i]):int(starts[i]) + int(lens[i])].tobytes()
                w = cache.get(key)
                if w is None:
                    text = key.decode("utf-8")
                    try:
                        w = abi.WORLD_GLOBAL if text == "@global" else world_ids.get(sanitize_world_name(text), abi.WORLD_INVALID)
                    except SanitizeError:
                        w = abi.WORLD_INVALID
                    cache[key] = w
                world[i] = w
            be = h_msg["sender_uuid"].view(">u8").astype(np.uint64)       # n x 2: high, low
            at = np.searchsorted(sorted_keys[:, 0], be[:, 0])
            at = np.minimum(at, N_PEERS - 1)
            hit = ok & (sorted_keys[at, 0] == be[:, 0]) & (sorted_keys[at, 1] == be[:, 1])   # random uuids: no equal high halves
            sender = np.where(hit, order[at], abi.INGEST_NO_PEER).astype(np.uint32)
            return world, sender

        def host():
            cache.clear()
            host_decode()
            world, sender = resolve()
            p_out["pos"].numpy()[:] = h_msg["position"]
            p_out["world"].numpy().view(np.uint32)[:] = world
            p_out["sender"].numpy().view(np.uint32)[:] = sender
            p_out["repl"].numpy()[:] = h_msg["replication"]
            with torch.cuda.stream(stream):
                for k in p_out:
                    d_out[k].copy_(p_out[k], non_blocking=True)

        self.sync()
        hip()
        got = tick.read()
        c = got["counters"]
        first = {k: v.copy() for k, v in got.items() if k != "counters"}
        moved = n * (OUT_BYTES + 8) + nb - payload_bytes
        res = {"frames": n, "frame_bytes": nb, "mean_frame": round(nb / max(n, 1), 1), "bytes_moved": moved, "counters": c}
        checks = {}
        host_decode()
        checks["hip_msg_equals_wq_decode_messages"] = bool(got["msg"].tobytes() == h_msg.tobytes())
        with_host = host_form and "host" in self.forms
        if with_host:
            world, sender = resolve()
            ok = h_msg["status"] == 0
            checks["hip_world_equals_host"] = bool((got["world"][ok] == world[ok]).all())
            checks["hip_sender_equals_host"] = bool((got["sender"][ok] == sender[ok]).all())
        hip_upload()
        again = tick.read()
        checks["hip_deterministic"] = all(again[k].tobytes() == first[k].tobytes() for k in first) and again["counters"] == c
        res["checks"] = checks
        assert all(checks.values()), checks
        del first, again, got
        fns = {"hip": hip}
        for f, fn in (("hip_upload", hip_upload), ("host_decode", host_decode), ("copy", copy)):
            if f in self.forms:
                fns[f] = fn
        for fn in fns.values():
            for _ in range(self.a.warmup):
                fn()
        times = {f: [] for f in fns}
        for _ in range(self.a.reps):  # alternating
            for f, fn in fns.items():
                times[f] += self.timed(fn, 1)
        if with_host:
            host()
            times["host"] = self.timed(host, self.a.host_reps)
        res["times"] = {f: summary(v) for f, v in times.items()}
        hip_ms = statistics.fmean(times["hip"])
        res["hip_frames_GBps"] = round(nb / (hip_ms / 1e3) / 1e9, 1)
        res["hip_fraction_of_8TBps"] = round(moved / (hip_ms / 1e3) / HBM_BYTES_PER_S, 4)
        for f in ("copy", "host", "host_decode", "hip_upload"):
            if f in times:
                res[f + "_over_hip"] = round(statistics.fmean(times[f]) / hip_ms, 3)
        if "host" in times and "hip_upload" in times:
            res["host_over_hip_upload"] = round(statistics.fmean(times["host"]) / statistics.fmean(times["hip_upload"]), 3)
        res["host_threads"] = self.a.threads
        print(f"[{name}] " + json.dumps(res), flush=True)
        self.sync()
        r.set_stream(None)
        r.close()
        del tick
        torch.cuda.empty_cache()
        return res

    # ---- shapes ----
    def scaled(self, n):
        return max(2, int(round(n * self.a.scale)))

    def shape_c5(self):
        n = self.scaled(1_000_000)
        return self.run("c5", *self.build(n, pos=np.random.default_rng(5).uniform(-5000, 5000, (n, 3))))

    def mix_frames(self, n):
        lens = np.maximum(frame_mix(n).astype(np.int64) - 124, 0)
        return self.build(n, flex_lens=lens) + (int(lens.sum()),)

    def shape_mix(self):
        frames, off, payload = self.mix_frames(self.scaled(1_000_000))
        return self.run("mix", frames, off, payload)

    def shape_mix_corrupt(self):
        torch = self.torch
        frames, off, payload = self.mix_frames(self.scaled(1_000_000))
        n = off.numel() - 1
        g = torch.Generator(device=self.dev).manual_seed(9)
        hit = torch.nonzero(torch.rand(n, device=self.dev, generator=g) < 0.3).flatten()
        size = (off[1:] - off[:-1])[hit]
        at = off[:-1][hit] + torch.minimum((torch.rand(hit.numel(), device=self.dev, generator=g) * 120).long(), size - 1)
        frames[at] = frames[at] ^ 0x41                       # inside the structure and strings, not deep in the flex
        return self.run("mix_corrupt", frames, off, payload, host_form=False)

    def shape_one_flex(self):
        n, per = self.scaled(1_000_000), 256
        one = np.zeros(n, np.int64)
        one[n // 2] = per * n
        a = self.run("one_flex", *self.build(n, flex_lens=one), payload_bytes=per * n, host_form=False)
        b = self.run("one_flex_spread", *self.build(n, flex_lens=np.full(n, per, np.int64)), payload_bytes=per * n, host_form=False)
        return {"one_message": a, "spread": b, "hip_one_message_over_spread": round(a["times"]["hip"]["mean_ms"] / b["times"]["hip"]["mean_ms"], 3)}

    def shape_big_params(self):
        k = max(2, int(round(256 * self.a.scale)))
        a = self.run("big_params", *self.build(k, param_lens=np.full(k, 1 << 20, np.int64)), host_form=False)
        m = k * 4096
        b = self.run("big_params_spread", *self.build(m, param_lens=np.full(m, 256, np.int64)), host_form=False)
        return {"long": a, "spread": b, "hip_long_over_spread": round(a["times"]["hip"]["mean_ms"] / b["times"]["hip"]["mean_ms"], 3)}

    def shape_records(self):
        from worldql_server_amd import codec
        torch = self.torch
        n = self.scaled(10_000)
        rec = lambda i: dict(uuid=uuid.UUID(int=i + 1).bytes, world_name="world", position=(1.0 * i, 2.0, 3.0), data="d" * 20)
        one = np.frombuffer(codec.serialize_message(dict(instruction=8, sender_uuid=self.peers[0].tobytes(), world_name="world",
                                                          records=[rec(i) for i in range(100)])), np.uint8)
        frames = torch.from_numpy(np.tile(one, n)).to(self.dev)
        off = torch.arange(n + 1, dtype=torch.int64, device=self.dev) * len(one)
        return self.run("records", frames, off)

    def shape_set_peers(self):
        from worldql_server_amd.router import Router
        n = self.scaled(1_000_000)
        table = np.random.default_rng(12).integers(0, 256, (n, 16), dtype=np.uint8)
        r = Router(16, 0)
        times = []
        for _ in range(self.a.warmup + self.a.reps):
            t0 = time.perf_counter()
            r.set_ingest_peers(table)
            times.append((time.perf_counter() - t0) * 1e3)
        r.close()
        res = {"peers": n, "times": {"set_peers": summary(times[self.a.warmup:])}}
        print("[set_peers] " + json.dumps(res), flush=True)
        return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default="c5,mix,mix_corrupt,one_flex,big_params,records,set_peers")
    ap.add_argument("--forms", default="hip,hip_upload,host,host_decode,copy")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_decode_bench.json"))
    a = ap.parse_args()
    b = DecodeBench(a)
    b.peers = np.random.default_rng(2).integers(0, 256, (int(N_PEERS * 1.1) + 1, 16), dtype=np.uint8)
    b.peer_key = np.ascontiguousarray(b.peers).view(">u8").astype(np.uint64)
    only = a.only.split(",")
    out = {"tool": "tools/frames_decode_bench.py", "scale": a.scale, "reps": a.reps, "warmup": a.warmup, "host_reps": a.host_reps,
           "forms": b.forms, "timing": "host clock, a device synchronise on both sides of every repeat",
           "host": f"wq_decode_messages on {a.threads} threads over pinned frames, per-message world resolution (sanitize + "
                   "dict, cached by name bytes) and sender lookup (sorted table), fill and upload of pos / world / sender / repl",
           "copy": "device-to-device copy of the frame bytes on the handle's stream", "shapes": {}}
    ok = True
    for name in ("c5", "mix", "mix_corrupt", "one_flex", "big_params", "records", "set_peers"):
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
