#!/usr/bin/env python3
"""The ingest joins (wq_ingest_join_device, wq_ingest_drop_peers_device, csrc/wq_join.hip) against the host
leg they replace and against the dispatch alone, in one process, the forms alternating. Every shape has a
sender table of 1M uuids reserved to 2M; the frames are built on the device by the frame builder and decoded
by wq_frames_decode_device, so the arrays are the decoder's.

  join      Router.join_peers_device on the decode's arrays: ids assigned, sender / flags patched, the table
            merged, asynchronous, no read-back. Before every repeat (untimed) the tick is decoded again and
            the joined ids are dropped, so every repeat joins the same uuids into the same table;
  dispatch  Router.dispatch_device on the same arrays, for scale;
  host      the leg the join replaces in a tick with joins: the read-back of the dispatch's counters, the
            deferred list and its uuids, PeerIds.id per join, wq_ingest_set_peers of the whole table (a host
            sort of every uuid and an upload), and the second decode + dispatch of the tick. Before every
            repeat (untimed) the original table is set again and the tick decoded and dispatched;
  drop      Router.drop_peers_device of 10,000 ids (the table is set again before every repeat, untimed);
  rebuild   what the drop replaces: wq_ingest_set_peers of the table without those ids.

Shapes: c5 (1M LocalMessage frames, every sender known: the call's fixed cost), c5_subs (the same with 1%
subscribes, 1,000 of them from new uuids), subs_100k (100,000 subscribes from 100,000 distinct new uuids),
one_uuid (1M subscribes that all carry one new uuid), drop_10k.

Before anything is timed the join's counters are checked against the shape's construction, the dispatch
that follows must defer nothing, and a second join must be byte-identical. Then --warmup untimed and --reps
timed repeats per form, a synchronise on both sides of each; min / mean / max with every number.
bytes_moved is what the join must read and write once: 10 B per frame (instruction, flags, world, sender),
16 B per candidate, 21 B per patched frame, and with joins 40 B per live table entry and 20 B per join.

One shape per process keeps every GPU step under a time limit of its own; a run with --only adds its
shapes to the file the earlier runs wrote.

    python tools/ingest_join_bench.py [--scale 1.0] [--only c5,c5_subs,subs_100k,one_uuid,drop_10k]
                                      [--reps 7] [--warmup 3] [--host-reps 3] [--out profiles/ingest_join_bench.json]
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

HBM_BYTES_PER_S = 8e12
WORLDS = ["world", "nether", "the_end"]
SHAPES = ("c5", "c5_subs", "subs_100k", "one_uuid", "drop_10k")
SUB, LOCAL = 4, 7
ID_LIMIT = 1 << 22


class JoinBench(Bench):
    def table(self):
        n = max(1000, int(round(1_000_000 * self.a.scale)))
        rng = np.random.default_rng(1)
        return rng.integers(0, 256, (n, 16), dtype=np.uint8)       # distinct with overwhelming probability

    def new_uuids(self, k):
        return np.random.default_rng(2).integers(0, 256, (k, 16), dtype=np.uint8)

    def build(self, r, ins, uuids):
        """The frames of (instruction, uuid) messages in random worlds with positions, on the device."""
        torch, abi = self.torch, self.abi
        n = len(ins)
        rng = np.random.default_rng(3)
        keep = dict(ins=torch.from_numpy(ins).to(self.dev), uuid=torch.from_numpy(np.ascontiguousarray(uuids)).to(self.dev),
                    world=torch.from_numpy(rng.integers(0, 3, n).astype(np.int32)).to(self.dev),
                    pos=torch.from_numpy(rng.uniform(-5000, 5000, (n, 3))).to(self.dev))
        s = abi.FramesSrc(instruction=keep["ins"].data_ptr(), instruction_all=0, replication=None, replication_all=0,
                          sender_uuid=keep["uuid"].data_ptr(), world=keep["world"].data_ptr(), pos=keep["pos"].data_ptr(),
                          param=None, param_offsets=None, n_param_bytes=0, flex=None, flex_offsets=None, n_flex_bytes=0,
                          msg_flags=None)
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
        return frames[:need], off

    def router(self, table):
        from worldql_server_amd.router import Router
        r = Router(16, 0)
        r.set_worlds(WORLDS)
        r.set_ingest_peers(table)
        r.reserve_peers(2 * len(table))
        return r

    def run(self, name, ins, uuids, table, want_joined):
        from worldql_server_amd import ingest
        from worldql_server_amd.subscriptions import PeerIds
        torch, abi = self.torch, self.abi
        n, T = len(ins), len(table)
        r = self.router(table)
        frames, off = self.build(r, ins, uuids)
        tick = ingest.IngestTick(r, capacity=n)
        jcnt = torch.zeros(abi.JOIN_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        j_id = torch.zeros(max(n, 1), dtype=torch.int32, device=self.dev)
        j_frame, j_uuid = torch.zeros_like(j_id), torch.zeros(16 * max(n, 1), dtype=torch.uint8, device=self.dev)
        o = tick.out
        j_in = abi.JoinIn(instruction=o.instruction, world=o.world, sender_uuid=o.sender_uuid, flags=o.flags, sender=o.sender,
                          free_ids=None, n_free=0, id_next=T, id_limit=ID_LIMIT)
        j_out = abi.JoinOut(j_uuid=j_uuid.data_ptr(), j_id=j_id.data_ptr(), j_frame=j_frame.data_ptr(), joined_capacity=n)
        state = dict(k=0)

        def fresh():                      # untimed: the tick as the decode leaves it, the table as it was
            if state["k"]:
                r.drop_peers_device(j_id.data_ptr(), state["k"])
            tick.decode(frames, off)
            self.sync()

        def join():
            r.join_peers_device(j_in, n, j_out, jcnt.data_ptr())

        def read_join():
            self.sync()
            c = ingest.join_counters(jcnt.cpu().numpy())
            state["k"] = 0 if c["overflow"] else c["n_joined"]
            return c

        def dispatch():
            tick.dispatch()

        fresh()
        join()
        c = read_join()
        first = (j_id[:c["n_joined"]].clone(), tick.buf["sender"].clone(), tick.buf["flags"].clone())
        dispatch()
        self.sync()
        d = tick.read_dispatch()["counters"]
        checks = dict(joined_as_built=c["n_joined"] == want_joined, no_overflow=c["overflow"] == 0 and c["error"] == 0,
                      table_grew=c["n_table"] == T + want_joined, nothing_deferred=d["n_deferred"] == 0)
        fresh()
        join()
        c2 = read_join()
        checks["deterministic"] = c2 == c and torch.equal(j_id[:c["n_joined"]], first[0]) and \
            torch.equal(tick.buf["sender"], first[1]) and torch.equal(tick.buf["flags"], first[2])
        tu, _ = r.read_peers()
        key = np.ascontiguousarray(tu).view(">u8").reshape(-1, 2)
        up = (key[1:, 0] > key[:-1, 0]) | ((key[1:, 0] == key[:-1, 0]) & (key[1:, 1] > key[:-1, 1]))
        checks["table_ascending"] = len(tu) == T + want_joined and bool(up.all())
        assert all(checks.values()), (checks, c, d)
        moved = 10 * n + 16 * c["n_candidates"] + 21 * c["n_patched"] + (40 * T + 20 * c["n_joined"] if c["n_joined"] else 0)
        res = {"frames": n, "table": T, "join_counters": c, "bytes_moved": moved, "checks": checks}
        del first

        # the host leg: its state per repeat
        host = PeerIds()
        for k in range(T):
            host.id(k)                    # stand-ins for the 1M connected uuids; the joins' uuids are added and released
        table_ids = np.arange(T, dtype=np.uint32)

        def host_prepare():               # untimed: the original table, the tick decoded and dispatched with its joins deferred
            r.set_ingest_peers(table, table_ids)
            tick.decode(frames, off).dispatch()
            self.sync()

        def host_leg():
            cnt, _ = tick._read_ctrl()                                   # the tick's read-back
            lo, hi = cnt["side_begin"][4], cnt["side_begin"][5]
            idx = tick.dbuf["side_src"][4 * lo:4 * hi].view(torch.int32).to(torch.int64)
            uu = tick.buf["sender_uuid"][:16 * n].view(n, 16)[idx].cpu().numpy()   # the deferred frames' uuids
            new, ids = {}, []
            if len(uu):                                                  # the distinct uuids in arrival order
                _, at = np.unique(np.ascontiguousarray(uu).view("V16").reshape(-1), return_index=True)
                for row in uu[np.sort(at)]:
                    key = row.tobytes()
                    new[key] = host.id(key)
                    ids.append(new[key])
            if new:                                                      # the whole table again: host sort, upload
                all_u = np.concatenate([table, np.frombuffer(b"".join(new), np.uint8).reshape(-1, 16)])
                r.set_ingest_peers(all_u, np.concatenate([table_ids, np.array(ids, np.uint32)]))
                tick.decode(frames, off).dispatch()                      # and the tick again
                self.sync()
            for key in new:
                host.release(key)
            return len(new)

        fns = {"join": (fresh, join), "dispatch": (fresh, dispatch)}
        for prep, fn in fns.values():
            for _ in range(self.a.warmup):
                prep(), fn(), read_join()
        times = {f: [] for f in fns}
        for _ in range(self.a.reps):      # alternating
            for f, (prep, fn) in fns.items():
                prep()
                times[f] += self.timed(fn, 1)
                read_join()
        if "host" in self.forms:
            times["host"] = []
            for rep in range(self.a.host_reps + 1):
                host_prepare()
                t = self.timed(host_leg, 1)
                if rep:                   # the first one warms up
                    times["host"] += t
            r.set_ingest_peers(table, table_ids)
            res["host_note"] = "read-back of counters, deferred list and uuids; PeerIds.id per join; wq_ingest_set_peers of the " \
                               "whole table when a sender joined; second decode + dispatch"
        res["times"] = {f: summary(v) for f, v in times.items()}
        join_ms = statistics.fmean(times["join"])
        res["join_fraction_of_8TBps"] = round(moved / (join_ms / 1e3) / HBM_BYTES_PER_S, 5)
        res["join_ns_per_frame"] = round(join_ms * 1e6 / n, 3)
        res["join_over_dispatch"] = round(join_ms / statistics.fmean(times["dispatch"]), 3)
        if "host" in times:
            res["host_over_join"] = round(statistics.fmean(times["host"]) / join_ms, 3)
        print(f"[{name}] " + json.dumps(res), flush=True)
        r.close()
        return res

    # ---- shapes ----
    def frames_n(self, n):
        return max(2000, int(round(n * self.a.scale)))

    def known_senders(self, table, n):
        return table[np.random.default_rng(4).integers(0, len(table), n)]

    def shape_c5(self):
        table = self.table()
        n = self.frames_n(1_000_000)
        return self.run("c5", np.full(n, LOCAL, np.uint8), self.known_senders(table, n), table, 0)

    def shape_c5_subs(self):
        table = self.table()
        n = self.frames_n(1_000_000)
        ins, uu = np.full(n, LOCAL, np.uint8), self.known_senders(table, n)
        subs = np.arange(50, n, 100)
        ins[subs] = SUB
        k = max(1, len(subs) // 10)
        uu[subs[::10][:k]] = self.new_uuids(k)
        return self.run("c5_subs", ins, uu, table, k)

    def shape_subs_100k(self):
        table = self.table()
        n = self.frames_n(100_000)
        return self.run("subs_100k", np.full(n, SUB, np.uint8), self.new_uuids(n), table, n)

    def shape_one_uuid(self):
        table = self.table()
        n = self.frames_n(1_000_000)
        return self.run("one_uuid", np.full(n, SUB, np.uint8), np.repeat(self.new_uuids(1), n, axis=0), table, 1)

    def shape_drop_10k(self):
        from worldql_server_amd import ingest
        torch, abi = self.torch, self.abi
        table = self.table()
        T = len(table)
        ids = np.arange(T, dtype=np.uint32)
        k = max(10, int(round(10_000 * self.a.scale)))
        gone = np.random.default_rng(6).choice(T, k, replace=False).astype(np.uint32)
        d_gone = torch.from_numpy(gone.view(np.int32)).to(self.dev)
        keep = np.ones(T, bool)
        keep[gone] = False
        r = self.router(table)
        cnt = torch.zeros(abi.JOIN_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)

        def prepare():
            r.set_ingest_peers(table, ids)
            self.sync()

        def drop():
            r.drop_peers_device(d_gone.data_ptr(), k, cnt.data_ptr())

        def rebuild():
            r.set_ingest_peers(table[keep], ids[keep])

        prepare(), drop(), self.sync()
        c = ingest.join_counters(cnt.cpu().numpy())
        tu, ti = r.read_peers()
        order = np.lexsort(table[keep].T[::-1])
        checks = dict(removed=c["n_patched"] == k and c["n_table"] == T - k,
                      table_equals_rebuild=tu.tobytes() == table[keep][order].tobytes() and ti.tolist() == ids[keep][order].tolist())
        assert all(checks.values()), (checks, c)
        times = {"drop": [], "rebuild": []}
        for rep in range(self.a.warmup + self.a.reps):
            for f, fn in (("drop", drop), ("rebuild", rebuild)):
                prepare()
                t = self.timed(fn, 1)
                if rep >= self.a.warmup:
                    times[f] += t
        moved = 4 * k + 2 * 20 * T + 20 * (T - k)       # ids; every entry's id read, the kept entries copied out and back
        res = {"table": T, "dropped": k, "counters": c, "checks": checks, "bytes_moved": moved,
               "times": {f: summary(v) for f, v in times.items()}}
        drop_ms = statistics.fmean(times["drop"])
        res["drop_fraction_of_8TBps"] = round(moved / (drop_ms / 1e3) / HBM_BYTES_PER_S, 5)
        res["rebuild_over_drop"] = round(statistics.fmean(times["rebuild"]) / drop_ms, 3)
        print("[drop_10k] " + json.dumps(res), flush=True)
        r.close()
        return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default=",".join(SHAPES))
    ap.add_argument("--forms", default="join,dispatch,host")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_join_bench.json"))
    a = ap.parse_args()
    b = JoinBench(a)
    only = a.only.split(",")
    out = {"tool": "tools/ingest_join_bench.py", "scale": a.scale, "reps": a.reps, "warmup": a.warmup, "host_reps": a.host_reps,
           "forms": b.forms, "timing": "host clock, a device synchronise on both sides of every repeat", "shapes": {}}
    if os.path.exists(a.out):   # one shape per process, each under its own time limit: keep the other shapes' results
        with open(a.out) as fh:
            prev = json.load(fh)
        if all(prev.get(k) == out[k] for k in ("tool", "scale", "reps", "warmup")):
            out["shapes"] = {k: v for k, v in prev.get("shapes", {}).items() if k not in only}
    ok = True
    for name in SHAPES:
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
