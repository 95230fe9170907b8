#!/usr/bin/env python3
"""The ingest leaves (wq_ingest_leave_device + wq_remove_peers_device, csrc/wq_leave.hip) against the host leg
they replace and against wq_remove_peers alone, in one process, the forms alternating. Every shape runs on
C5's subscription table (1M entities, 27M entries) with a sender table of 1M uuids reserved to 2M; peer id k
holds uuid row k and one stamp in last_seen.

  device  IngestTick.leave: the sweep (stamps compared, leavers listed with their uuid text, bitmap, free list,
          stamps reset, sender table compacted) and the table's removal from the sweep's bitmap, back to back,
          asynchronous, nothing read back;
  host    the leg the two calls replace: last_seen downloaded, the compare in numpy, wq_remove_peers (which
          builds and uploads its bitmap and waits), wq_ingest_drop_peers_device, PeerIds.release per peer and
          the uuid text of every PeerDisconnect in Python;
  remove  wq_remove_peers alone on the same ids: the floor for the table pass, since the kernel is the same.

Shapes: nobody (no stamp is stale), stale_1k, stale_100k, everyone (every stamp stale), listed_10k (10,000
disconnects listed, no stamp stale).

Before every repeat (untimed) the leavers' subscriptions are applied again from their exported rows, the sender
table is set again and the stamps are reset, so every repeat does the same work. Before anything is timed the
sweep's counters are checked against the shape's construction, the table after the device form must export
the same bytes as after wq_remove_peers, and the leavers' text must be Python's. Then --warmup untimed and
--reps timed repeats of device and remove, alternating, and --host-reps of the host leg after one warm-up; a
synchronise on both sides of each; min / mean / max with every number.

bytes_moved is what the two calls must read and write once. The sweep: 8 B per live sender entry (id, stamp),
2 B per reserved entry (the reason byte, written and read), 12 B per 64 reserved entries, 4 B per 32 ids and
listed id, 73 B per leaver (its rows, text, offset, free-list entry, stamp), and with leavers 60 B per kept
entry (read, copied out and back). The table pass, when somebody leaves: 128 B per live cube record, a lower
bound (the pass also walks the empty record slots and the lists above 24 peers).

One shape per process keeps every GPU step under a time limit of its own; a run with --only adds its shapes
to the file the earlier runs wrote.

    python tools/ingest_leave_bench.py [--scale 1.0] [--only nobody,stale_1k,stale_100k,everyone,listed_10k]
                                       [--reps 7] [--warmup 2] [--host-reps 3] [--out profiles/ingest_leave_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import traceback
import uuid

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from peer_budget_bench import Bench, summary  # noqa: E402

HBM_BYTES_PER_S = 8e12
SHAPES = ("nobody", "stale_1k", "stale_100k", "everyone", "listed_10k")
NOW, MAX_AGE = 1000, 10


class LeaveBench(Bench):
    def run(self, name, stale, listed):
        """stale, listed: fractions of the 1M peers (stale None: everyone)."""
        from worldql_server_amd import abi, ingest, synth_ext
        from worldql_server_amd.router import Router
        from worldql_server_amd.subscriptions import PeerIds
        torch = self.torch
        c5 = synth_ext.config_c5(scale=self.a.scale)
        T = c5.n
        r = Router(16, 0)
        r.apply_ops(c5.initial_ops())
        st = r.stats()
        table = np.random.default_rng(1).integers(0, 256, (T, 16), dtype=np.uint8)   # distinct with overwhelming probability
        ids = np.arange(T, dtype=np.uint32)
        r.set_ingest_peers(table, ids)
        r.reserve_peers(2 * T)
        rng = np.random.default_rng(2)
        n_stale = T if stale is None else int(round(stale * T))
        n_listed = int(round(listed * T))
        stale_ids = np.sort(rng.choice(T, n_stale, replace=False)).astype(np.uint32)
        listed_ids = np.sort(rng.choice(T, n_listed, replace=False)).astype(np.uint32)
        gone = np.union1d(stale_ids, listed_ids).astype(np.uint32)
        base = np.full(T, NOW - 1, np.uint32)
        base[stale_ids] = NOW - MAX_AGE - 1
        d_base = self.dev_u32(base)
        last_seen = d_base.clone()
        d_listed = self.dev_u32(listed_ids) if n_listed else None
        tick = ingest.IngestTick(r, capacity=16)

        # the leavers' subscriptions, to put them back before every repeat
        rows_cap = st["n_entries"] if len(gone) == T else 40 * len(gone) + 64
        rows = torch.zeros((max(rows_cap, 1), 5), dtype=torch.int64, device=self.dev)
        rc, n_rows = r.export_table_device(rows.data_ptr(), rows_cap, peers=None if len(gone) == T else gone)
        assert rc == 0, (rc, n_rows, rows_cap)
        state = dict(dirty=False)

        def restore():                    # untimed
            if state["dirty"] and len(gone):
                r.apply_ops_device(rows.data_ptr(), n_rows)
                r.set_ingest_peers(table, ids)
            last_seen.copy_(d_base)
            state["dirty"] = False
            self.sync()

        def device():
            tick.leave(last_seen, NOW, MAX_AGE, leave_ids=d_listed)
            state["dirty"] = True

        def remove():
            r.remove_peers(gone)
            state["dirty"] = True

        snap = None
        if "host" in self.forms:
            host = PeerIds()
            for k in range(T):
                host.id(k)                # peer k holds id k
            snap = host.snapshot()
            del host

        def host_leg(host):
            seen = last_seen.cpu().numpy().view(np.uint32).astype(np.int64)          # the download
            is_stale = (seen != abi.SEEN_NEVER) & (NOW > seen) & (NOW - seen > MAX_AGE)
            out = np.union1d(np.flatnonzero(is_stale), listed_ids).astype(np.uint32)
            r.remove_peers(out)
            d_out = self.dev_u32(out)
            r.drop_peers_device(d_out.data_ptr() if len(out) else None, len(out))
            text = []
            for i in out:
                host.release(int(i))
                text.append(str(uuid.UUID(bytes=table[i].tobytes())))
            state["dirty"] = True
            return len(text)

        def table_bytes():
            buf = torch.zeros((st["n_entries"], 5), dtype=torch.int64, device=self.dev)
            rc, n = r.export_table_device(buf.data_ptr(), st["n_entries"])
            assert rc == 0
            return buf[:n]

        # checks, untimed
        restore()
        device()
        lv = tick.read_leave()
        c = lv["counters"]
        after_device = table_bytes()
        order = np.lexsort(table[gone].T[::-1]) if len(gone) else np.zeros(0, np.int64)
        checks = dict(left_as_built=c["n_left"] == len(gone) and c["n_stale"] == n_stale and c["n_listed_found"] == n_listed,
                      no_overflow=c["overflow"] == 0 and c["error"] == 0, table_shrank=c["n_table"] == T - len(gone),
                      leavers_in_uuid_order=lv["l_id"].tolist() == gone[order].tolist(),
                      text_is_pythons=lv["l_param"][:36 * min(len(gone), 1000)].tobytes().decode() ==
                      "".join(str(uuid.UUID(bytes=table[i].tobytes())) for i in gone[order][:1000]))
        restore()
        remove()
        self.sync()
        after_remove = table_bytes()
        checks["table_equals_remove_peers"] = after_device.shape == after_remove.shape and bool(torch.equal(after_device, after_remove))
        checks["rows_left"] = int(after_remove.shape[0]) == st["n_entries"] - n_rows
        del after_device, after_remove
        restore()
        checks["restored"] = r.stats()["n_entries"] == st["n_entries"] and len(r.read_peers()[1]) == T
        assert all(checks.values()), (checks, c)

        k = len(gone)
        sweep = 8 * T + 2 * 2 * T + 12 * (2 * T // 64) + 4 * (T // 32) + 4 * n_listed + 73 * k + (60 * (T - k) if k else 0)
        moved = sweep + (128 * st["n_cubes"] if k else 0)   # with nobody leaving every block of the table pass returns at once
        res = {"senders": T, "table_entries": st["n_entries"], "table_cubes": st["n_cubes"], "stale": n_stale, "listed": n_listed,
               "left": k, "leave_counters": c, "bytes_moved": moved, "bytes_moved_sweep": sweep, "checks": checks}

        fns = {"device": device, "remove": remove}
        for fn in fns.values():
            for _ in range(self.a.warmup):
                restore(), fn(), self.sync()
        times = {f: [] for f in fns}
        for _ in range(self.a.reps):      # alternating
            for f, fn in fns.items():
                restore()
                times[f] += self.timed(fn, 1)
        if snap is not None:
            times["host"] = []
            for rep in range(self.a.host_reps + 1):
                restore()
                host = PeerIds.restore(snap)
                t = self.timed(lambda: host_leg(host), 1)
                if rep:                   # the first one warms up
                    times["host"] += t
            res["host_note"] = "download of last_seen, numpy compare, wq_remove_peers, wq_ingest_drop_peers_device, " \
                               "PeerIds.release and str(uuid.UUID) per leaver"
        res["times"] = {f: summary(v) for f, v in times.items()}
        dev_ms = statistics.fmean(times["device"])
        res["device_fraction_of_8TBps"] = round(moved / (dev_ms / 1e3) / HBM_BYTES_PER_S, 5)
        res["device_over_remove"] = round(dev_ms / statistics.fmean(times["remove"]), 3)
        if "host" in times:
            res["host_over_device"] = round(statistics.fmean(times["host"]) / dev_ms, 3)
        print(f"[{name}] " + json.dumps(res), flush=True)
        r.close()
        return res

    def shape_nobody(self):
        return self.run("nobody", 0.0, 0.0)

    def shape_stale_1k(self):
        return self.run("stale_1k", 0.001, 0.0)

    def shape_stale_100k(self):
        return self.run("stale_100k", 0.1, 0.0)

    def shape_everyone(self):
        return self.run("everyone", None, 0.0)

    def shape_listed_10k(self):
        return self.run("listed_10k", 0.0, 0.01)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default=",".join(SHAPES))
    ap.add_argument("--forms", default="device,remove,host")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_leave_bench.json"))
    a = ap.parse_args()
    b = LeaveBench(a)
    only = a.only.split(",")
    out = {"tool": "tools/ingest_leave_bench.py", "scale": a.scale, "reps": a.reps, "warmup": a.warmup, "host_reps": a.host_reps,
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
