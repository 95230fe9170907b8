"""The record store: RecordCreate / RecordRead / RecordDelete (include/wq_router.h, wq_records.hip).

`RecordStoreRef` is the definition in plain Python — the reference's DatabaseClient
(worldql_server/src/database/client.rs, world_region.rs, query_constants.rs) and
handle_record_read (processing/record_read.rs) restated, with what the reference leaves open
fixed as the header says. `GpuRecordStore` is the ctypes binding of the wq_records_* calls and
`RecordProcessor` the host side of the three instructions around it. `DeviceRecordProcessor` is the same
with the per-record work on the device (wq_records_dispatch_device through ingest.IngestTick).
`slab_store_np` is the definition of wq_slab_store_device (csrc/wq_slab.hip), which keeps the created
records' payloads in device memory, and `DeviceRecordSlab` the torch-side owner of that slab.
`slab_compact_np` is the definition of wq_slab_compact_device (csrc/wq_slab_compact.hip), the slab's canonical
form: DeviceRecordSlab compacts, exports and loads through it, and DeviceRecordProcessor.snapshot / restore
with save_snapshot / load_snapshot carry the device record path across a restart.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import abi
from .world_names import GLOBAL_WORLD, SanitizeError, WorldIds, sanitize_world_name

CREATE, DELETE = 0, 1            # WQ_RECORD_CREATE / WQ_RECORD_DELETE
READ_DEDUPE = 1                  # WQ_RECORD_READ_DEDUPE
NO_AFTER = -(1 << 63)            # INT64_MIN: no `after`
I64_MAX = (1 << 63) - 1
AXIS_BIAS = 1 << 23              # wq_device.hpp kAxisBias
MAX_PACKED_WORLD = (1 << 24) - 2  # wq_device.hpp kMaxPackedWorld
MAX_ORDINALS = 0xFFFFFFC0        # record_ops.hpp kRecMaxOrdinals: rows the regions of one read call may hold

REC_OP_DTYPE = np.dtype([("kind", np.uint32), ("world", np.uint32), ("pos", np.float64, (3,)),
                         ("uuid_hi", np.uint64), ("uuid_lo", np.uint64), ("ts_us", np.int64),
                         ("handle", np.uint32), ("reserved", np.uint32)])  # struct wq_rec_op
assert REC_OP_DTYPE.itemsize == 64

REC_ROW_DTYPE = np.dtype([("world", np.uint32), ("handle", np.uint32), ("region", np.int64, (3,)),
                          ("uuid_hi", np.uint64), ("uuid_lo", np.uint64), ("ts_us", np.int64),
                          ("seq", np.uint64)])  # struct wq_rec_row: one stored row of a snapshot
assert REC_ROW_DTYPE.itemsize == 64


class RecVacuumResult(ctypes.Structure):  # struct wq_rec_vacuum_result
    _fields_ = [(f, ctypes.c_uint64) for f in ("rows_before", "rows_after", "bytes_before", "bytes_after")]


class RecImportResult(ctypes.Structure):  # struct wq_rec_import_result
    _fields_ = [("imported", ctypes.c_uint64), ("rejected", ctypes.c_uint64)]


class RecApplyResult(ctypes.Structure):  # struct wq_rec_apply_result
    _fields_ = [("created", ctypes.c_uint64), ("deleted_rows", ctypes.c_uint64), ("rejected", ctypes.c_uint64),
                ("rows_live", ctypes.c_uint64)]


class RecTotals(ctypes.Structure):  # struct wq_rec_totals
    _fields_ = [(f, ctypes.c_uint64) for f in ("created", "deleted_rows", "deduped_rows", "rejected_ops",
                                                "rejected_queries")]


class ReadTooLarge(OverflowError):
    """The regions of one read call hold 2^32 - 64 rows or more (WQ_E_CAPACITY): split the call."""


class RecReadResult(ctypes.Structure):  # struct wq_rec_read_result
    _fields_ = [("returned", ctypes.c_uint64), ("deduped_rows", ctypes.c_uint64), ("rejected", ctypes.c_uint64),
                ("scanned", ctypes.c_uint64), ("overflow", ctypes.c_uint32), ("error", ctypes.c_uint32)]


# ---- the two quantisers (world_region.rs:93-129) ----

def _sat_i64(c: float) -> int:
    """Rust's saturating `c as i64` for c >= 0."""
    return I64_MAX if c >= 9223372036854775808.0 else int(c)


def region_coord(c: float, size: int) -> int:
    """clamp_region_coord: the minimum of c's region. NaN has none (ValueError)."""
    if math.isnan(c):
        raise ValueError("NaN has no region")
    if c == 0.0:
        return 0
    if c >= 0.0:
        ci = _sat_i64(c)
        return ci - ci % size
    ci = _sat_i64((-c) + float(size))
    return -(ci - ci % size)


def table_coord(c: int, table_size: int) -> int:
    """clamp_table_size: multiples stay, the rest goes down on the positive side and to minus the
    table of (-c) + table_size on the negative one."""
    if c % table_size == 0:
        return c
    if c >= 0:
        return c - c % table_size
    nc = -c + table_size
    return -(nc - nc % table_size)


def region_coord_np(coords, size: int) -> np.ndarray:
    """clamp_region_coord over an array (i64). NaN raises ValueError."""
    c = np.ascontiguousarray(coords, dtype=np.float64)
    if np.isnan(c).any():
        raise ValueError("NaN has no region")
    neg = c < 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.where(neg, (-c) + np.float64(size), c)  # one f64 add on the negative side
        sat = a >= 9223372036854775808.0
        ci = np.where(sat, I64_MAX, np.where(sat, 0.0, a).astype(np.int64))
    r = ci - np.fmod(ci, np.int64(size))
    return np.where(neg, -r, r).astype(np.int64)


def table_coord_np(region, table_size: int) -> np.ndarray:
    """clamp_table_size over an array of i64 (inputs within +-2^62)."""
    c = np.ascontiguousarray(region, dtype=np.int64)
    t = np.int64(table_size)
    rem = np.fmod(c, t)  # truncated, like Rust's %
    nc = -c + t
    neg = -(nc - np.fmod(nc, t))
    return np.where(rem == 0, c, np.where(c >= 0, c - rem, neg)).astype(np.int64)


def position_packable(sizes, world: int, pos) -> bool:
    """The limit of this version: no NaN, every region index in [-2^23, 2^23), world < 2^24 - 1."""
    if any(math.isnan(float(c)) for c in pos) or world > MAX_PACKED_WORLD:
        return False
    return all(-AXIS_BIAS <= region_coord(float(c), s) // s < AXIS_BIAS for c, s in zip(pos, sizes))


class RecordStoreRef:
    """The definition. Rows live in a list; a row is dead once `live` is False. Every op the store
    receives gets the next sequence number, rejected ones included."""

    def __init__(self, rx: int, ry: int, rz: int, table_size: int):
        sizes = (int(rx), int(ry), int(rz))
        if any(s < 1 or s > 0xFFFF for s in sizes) or table_size < 1 or any(table_size % s for s in sizes):
            raise ValueError("region sizes must be >= 1 and divide the table size")
        self.sizes, self.table_size = sizes, int(table_size)
        self.rows: list[dict] = []
        self.by_region: dict[tuple, list[int]] = {}
        self.by_table_uuid: dict[tuple, list[int]] = {}
        self.by_region_uuid: dict[tuple, list[int]] = {}
        self.ops_seen = 0
        self.live = 0
        self.dead: list[int] = []
        self.totals_ = {"created": 0, "deleted_rows": 0, "deduped_rows": 0, "rejected_ops": 0, "rejected_queries": 0}
        self.deduped_cross = 0  # rows a dedupe killed in another region than the returned row's

    # -- keys --
    def region(self, pos) -> tuple:
        return tuple(region_coord(float(c), s) for c, s in zip(pos, self.sizes))

    def table(self, region) -> tuple:
        return tuple(table_coord(r, self.table_size) for r in region)

    def packable(self, world: int, pos) -> bool:
        return position_packable(self.sizes, world, pos)

    def _kill(self, i: int) -> int:
        row = self.rows[i]
        if not row["live"]:
            return 0
        row["live"] = False
        self.live -= 1
        self.dead.append(row["handle"])
        return 1

    # -- ops --
    def apply(self, ops) -> dict:
        """ops: REC_OP_DTYPE records (or dicts with the same fields), applied in order."""
        created = deleted = rejected = 0
        for op in ops:
            seq = self.ops_seen
            self.ops_seen += 1
            kind, world = int(op["kind"]), int(op["world"])
            pos = [float(c) for c in op["pos"]]
            if kind not in (CREATE, DELETE) or not self.packable(world, pos):
                rejected += 1
                continue
            reg = self.region(pos)
            uuid = (int(op["uuid_hi"]), int(op["uuid_lo"]))
            if kind == CREATE:
                i = len(self.rows)
                self.rows.append({"world": world, "region": reg, "table": self.table(reg), "uuid": uuid,
                                  "ts": int(op["ts_us"]), "seq": seq, "handle": int(op["handle"]), "live": True})
                self.by_region.setdefault((world, reg), []).append(i)
                self.by_table_uuid.setdefault((world, self.table(reg), uuid), []).append(i)
                self.by_region_uuid.setdefault((world, reg, uuid), []).append(i)
                self.live += 1
                created += 1
            else:  # every row of (region, uuid) stored so far, whatever its time
                for i in self.by_region_uuid.pop((world, reg, uuid), ()):
                    deleted += self._kill(i)
        for k, v in (("created", created), ("deleted_rows", deleted), ("rejected_ops", rejected)):
            self.totals_[k] += v
        return {"created": created, "deleted_rows": deleted, "rejected": rejected, "rows_live": self.live}

    def read(self, queries, dedupe: bool = False, capacity: int | None = None) -> dict:
        """queries: (world, pos, after_us | None) each. All of them are answered from the store as it
        is now; the dedupe deletions of every returned row apply afterwards. Returns offsets[n + 1],
        handles and ts_us (cut at `capacity`), and the counters of wq_rec_read_result."""
        # the one limit of a call, checked before anything is answered or killed
        if len(queries) * self.live > MAX_ORDINALS:  # (cheap bound first)
            counts, total = {}, 0
            for w, p, _ in queries:
                p = [float(c) for c in p]
                if not self.packable(int(w), p):
                    continue
                key = (int(w), self.region(p))
                if key not in counts:
                    counts[key] = sum(1 for i in self.by_region.get(key, ()) if self.rows[i]["live"])
                total += counts[key]
            if total > MAX_ORDINALS:
                raise ReadTooLarge(total)
        offsets, winners, rejected, scanned = [0], [], 0, 0
        for world, pos, after in queries:
            pos = [float(c) for c in pos]
            after = NO_AFTER if after is None else int(after)
            if not self.packable(int(world), pos):
                rejected += 1
                offsets.append(len(winners))
                continue
            best: dict[tuple, dict] = {}
            for i in self.by_region.get((int(world), self.region(pos)), ()):
                row = self.rows[i]
                if not row["live"]:
                    continue
                scanned += 1
                if not row["ts"] > after:
                    continue
                cur = best.get(row["uuid"])
                # the row met later wins on equal times: the higher sequence number
                if cur is None or (row["ts"], row["seq"]) > (cur["ts"], cur["seq"]):
                    best[row["uuid"]] = row
            winners.extend(best[u] for u in sorted(best))
            offsets.append(len(winners))
        self.totals_["rejected_queries"] += rejected
        deduped = 0
        if dedupe:
            for w in winners:
                for i in self.by_table_uuid.get((w["world"], w["table"], w["uuid"]), ()):
                    if self.rows[i]["ts"] < w["ts"]:
                        k = self._kill(i)
                        deduped += k
                        self.deduped_cross += k if self.rows[i]["region"] != w["region"] else 0
        self.totals_["deduped_rows"] += deduped
        self._sweep()
        cap = len(winners) if capacity is None else int(capacity)
        return {"offsets": np.array(offsets, dtype=np.uint32),
                "handles": np.array([w["handle"] for w in winners[:cap]], dtype=np.uint32),
                "ts_us": np.array([w["ts"] for w in winners[:cap]], dtype=np.int64),
                "returned": len(winners), "deduped_rows": deduped, "rejected": rejected, "scanned": scanned,
                "overflow": int(len(winners) > cap), "error": 0}

    def _sweep(self):
        """Drops dead rows from the lookup lists once they outnumber the live ones (speed only)."""
        if len(self.rows) - self.live <= max(self.live, 1024) or getattr(self, "_swept", 0) == len(self.rows):
            return
        self._swept = len(self.rows)
        for d in (self.by_region, self.by_table_uuid, self.by_region_uuid):
            for k in list(d):
                d[k] = [i for i in d[k] if self.rows[i]["live"]]
                if not d[k]:
                    del d[k]

    def drain_dead(self) -> np.ndarray:
        out = np.array(sorted(self.dead), dtype=np.uint32)
        self.dead = []
        return out

    def stats(self) -> tuple:
        """(rows_live, rows_stored, ops_seen)."""
        return self.live, len(self.rows), self.ops_seen

    def totals(self) -> dict:
        """Counts since the store was made (wq_records_totals)."""
        return dict(self.totals_)

    # -- vacuum and snapshots --
    def _index(self):
        """The three lookup lists from the rows (ascending row index, as appends leave them)."""
        self.by_region, self.by_table_uuid, self.by_region_uuid = {}, {}, {}
        for i, row in enumerate(self.rows):
            self.by_region.setdefault((row["world"], row["region"]), []).append(i)
            self.by_table_uuid.setdefault((row["world"], row["table"], row["uuid"]), []).append(i)
            self.by_region_uuid.setdefault((row["world"], row["region"], row["uuid"]), []).append(i)
        self.__dict__.pop("_swept", None)

    def vacuum(self) -> dict:
        """wq_records_vacuum: the dead rows go, the live ones keep their order, seq, ts and handle.
        Nothing a later call returns changes but `rows_stored`; the undrained dead list stays."""
        before = len(self.rows)
        if before != self.live:
            self.rows = [row for row in self.rows if row["live"]]
            self._index()
        return {"rows_before": before, "rows_after": len(self.rows)}

    def export_rows(self) -> tuple:
        """wq_records_export: (the live rows in row order as REC_ROW_DTYPE, ops_seen). Changes nothing."""
        live = [row for row in self.rows if row["live"]]
        out = np.zeros(len(live), dtype=REC_ROW_DTYPE)
        for i, row in enumerate(live):
            out[i] = (row["world"], row["handle"], row["region"], row["uuid"][0], row["uuid"][1], row["ts"], row["seq"])
        return out, self.ops_seen

    def import_rows(self, rows, ops_seen: int) -> dict:
        """wq_records_import into a store that has received no op (else ValueError). A row whose
        corner is off this store's region grid, whose region index or world is not packable or whose
        seq is not below `ops_seen` is rejected and counted; two accepted rows with the same (world,
        region, uuid, ts, seq) refuse the import (ValueError, the store stays empty). The table is
        this store's, computed from the region."""
        if self.ops_seen != 0 or self.rows:
            raise ValueError("an import needs a store that has received no op")
        accepted, seen, rejected = [], set(), 0
        for r in rows:
            world, seq = int(r["world"]), int(r["seq"])
            reg = tuple(int(c) for c in r["region"])
            if (world > MAX_PACKED_WORLD or seq >= ops_seen or any(c % s for c, s in zip(reg, self.sizes))
                    or not all(-AXIS_BIAS <= c // s < AXIS_BIAS for c, s in zip(reg, self.sizes))):
                rejected += 1
                continue
            uuid = (int(r["uuid_hi"]), int(r["uuid_lo"]))
            key = (world, reg, uuid, int(r["ts_us"]), seq)
            if key in seen:
                raise ValueError("the snapshot holds two rows with the same region, uuid, time and seq")
            seen.add(key)
            accepted.append({"world": world, "region": reg, "table": self.table(reg), "uuid": uuid,
                             "ts": int(r["ts_us"]), "seq": seq, "handle": int(r["handle"]), "live": True})
        self.rows = accepted
        self._index()
        self.live, self.ops_seen = len(accepted), int(ops_seen)
        return {"imported": len(accepted), "rejected": rejected}


def make_ops(kind, world, pos, uuid_hi, uuid_lo, ts_us=0, handle=0) -> np.ndarray:
    """REC_OP_DTYPE array from broadcastable columns (pos: [n, 3])."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    ops = np.zeros(len(pos), dtype=REC_OP_DTYPE)
    ops["kind"], ops["world"], ops["pos"] = kind, world, pos
    ops["uuid_hi"], ops["uuid_lo"], ops["ts_us"], ops["handle"] = uuid_hi, uuid_lo, ts_us, handle
    return ops


class GpuRecordStore:
    """wq_records_* on a Router's handle (one store per handle; single-GPU handles only)."""

    def __init__(self, router, rx: int, ry: int, rz: int, table_size: int):
        self.router, self.lib, self.h = router, router.lib, router.h
        router._check(self.lib.wq_records_open(self.h, rx, ry, rz, table_size))
        self.sizes, self.table_size = (int(rx), int(ry), int(rz)), int(table_size)
        self.open = True

    def close(self):
        if self.open and getattr(self.router, "h", None):
            self.router._check(self.lib.wq_records_close(self.h))
        self.open = False

    def apply(self, ops) -> dict:
        ops = np.ascontiguousarray(ops, dtype=REC_OP_DTYPE)
        res = RecApplyResult()
        self.router._check(self.lib.wq_records_apply(self.h, ops.ctypes.data_as(ctypes.c_void_p) if len(ops) else None,
                                                     len(ops), ctypes.byref(res)))
        return {"created": res.created, "deleted_rows": res.deleted_rows, "rejected": res.rejected,
                "rows_live": res.rows_live}

    def apply_device(self, ops_ptr: int, n: int) -> None:
        """wq_records_apply_device: asynchronous on the handle's stream."""
        self.router._check(self.lib.wq_records_apply_device(self.h, ops_ptr or None, n))

    @staticmethod
    def _result(res, offsets, handles, ts, capacity) -> dict:
        k = min(int(res.returned), capacity)
        return {"offsets": offsets, "handles": handles[:k], "ts_us": ts[:k], "returned": int(res.returned),
                "deduped_rows": int(res.deduped_rows), "rejected": int(res.rejected), "scanned": int(res.scanned),
                "overflow": int(res.overflow),
                "error": int(res.error)}

    def read(self, world, pos, after_us=None, dedupe: bool = False, capacity: int = 0, canary: int = 0) -> dict:
        """wq_records_read on host arrays with room for `capacity` rows. With canary > 0 that many
        words follow each output array, and the result's "canaries_ok" says whether they survived."""
        world = np.ascontiguousarray(world, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        n = len(world)
        after = None if after_us is None else np.ascontiguousarray(after_us, dtype=np.int64)
        mark32, mark64 = 0xA5A5A5A5, -0x5A5A5A5A5A5A5A5B
        offsets = np.full(n + 1 + canary, mark32, dtype=np.uint32)
        handles = np.full(capacity + canary, mark32, dtype=np.uint32)
        ts = np.full(capacity + canary, mark64, dtype=np.int64)
        res = RecReadResult()
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = self.lib.wq_records_read(
            self.h, n, p(world) if n else None, p(pos) if n else None, None if after is None or not n else p(after),
            READ_DEDUPE if dedupe else 0, p(offsets), p(handles) if capacity else None, p(ts) if capacity else None,
            capacity, ctypes.byref(res))
        if rc == abi.WQ_E_CAPACITY:
            raise ReadTooLarge(self.lib.wq_last_error(self.h).decode())
        self.router._check(rc)
        out = self._result(res, offsets[: n + 1], handles[:capacity], ts[:capacity], capacity)
        k = len(out["handles"])
        out["canaries_ok"] = bool((offsets[n + 1:] == mark32).all() and (handles[k:] == mark32).all()
                                  and (ts[k:] == mark64).all())
        return out

    def read_device(self, n: int, world_ptr: int, pos_ptr: int, after_ptr: int | None, dedupe: bool,
                    offsets_ptr: int, handles_ptr: int, ts_ptr: int, capacity: int) -> dict:
        """wq_records_read_device: device arrays in and out; the counters come back as a dict."""
        res = RecReadResult()
        rc = self.lib.wq_records_read_device(
            self.h, n, world_ptr or None, pos_ptr or None, after_ptr or None, READ_DEDUPE if dedupe else 0,
            offsets_ptr, handles_ptr or None, ts_ptr or None, capacity, ctypes.byref(res))
        if rc == abi.WQ_E_CAPACITY:
            raise ReadTooLarge(self.lib.wq_last_error(self.h).decode())
        self.router._check(rc)
        return {"returned": int(res.returned), "deduped_rows": int(res.deduped_rows), "rejected": int(res.rejected),
                "scanned": int(res.scanned), "overflow": int(res.overflow), "error": int(res.error)}

    def drain_dead(self) -> np.ndarray:
        n = ctypes.c_size_t()
        rc = self.lib.wq_records_drain_dead(self.h, None, 0, ctypes.byref(n))
        if rc not in (0, abi.WQ_E_CAPACITY):
            self.router._check(rc)
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            self.router._check(self.lib.wq_records_drain_dead(self.h, out.ctypes.data_as(ctypes.c_void_p), n.value,
                                                              ctypes.byref(n)))
        return out

    def stats(self) -> tuple:
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self.router._check(self.lib.wq_records_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def totals(self) -> dict:
        t = RecTotals()
        self.router._check(self.lib.wq_records_totals(self.h, ctypes.byref(t)))
        return {f: int(getattr(t, f)) for f, _ in RecTotals._fields_}

    def vacuum(self) -> dict:
        """wq_records_vacuum: rows and bytes (row arrays, dead list, views) before and after."""
        res = RecVacuumResult()
        self.router._check(self.lib.wq_records_vacuum(self.h, ctypes.byref(res)))
        return {f: int(getattr(res, f)) for f, _ in RecVacuumResult._fields_}

    def export_device(self, rows_ptr: int, capacity: int) -> tuple:
        """wq_records_export_device into device memory with room for `capacity` rows: (the live
        count, ops_seen). A capacity below the count writes nothing and raises WQError (WQ_E_CAPACITY);
        a null pointer with capacity 0 asks for the count."""
        n, ops = ctypes.c_size_t(), ctypes.c_uint64()
        rc = self.lib.wq_records_export_device(self.h, rows_ptr or None, capacity, ctypes.byref(n), ctypes.byref(ops))
        if not (rc == abi.WQ_E_CAPACITY and not capacity):
            self.router._check(rc)
        return n.value, ops.value

    def export_rows(self) -> tuple:
        """wq_records_export: (the live rows in row order as REC_ROW_DTYPE, ops_seen)."""
        n, ops = ctypes.c_size_t(), ctypes.c_uint64()
        rc = self.lib.wq_records_export(self.h, None, 0, ctypes.byref(n), ctypes.byref(ops))
        if rc not in (0, abi.WQ_E_CAPACITY):
            self.router._check(rc)
        out = np.zeros(n.value, dtype=REC_ROW_DTYPE)
        if n.value:
            self.router._check(self.lib.wq_records_export(self.h, out.ctypes.data_as(ctypes.c_void_p), n.value,
                                                          ctypes.byref(n), ctypes.byref(ops)))
        return out, ops.value

    def import_device(self, rows_ptr: int, n: int, ops_seen: int) -> dict:
        """wq_records_import_device: n wq_rec_row in device memory into this (unused) store."""
        res = RecImportResult()
        self.router._check(self.lib.wq_records_import_device(self.h, rows_ptr or None, n, ops_seen, ctypes.byref(res)))
        return {"imported": int(res.imported), "rejected": int(res.rejected)}

    def import_rows(self, rows, ops_seen: int) -> dict:
        """wq_records_import of REC_ROW_DTYPE rows (WQError: a used store or a duplicate row)."""
        rows = np.ascontiguousarray(rows, dtype=REC_ROW_DTYPE)
        res = RecImportResult()
        self.router._check(self.lib.wq_records_import(
            self.h, rows.ctypes.data_as(ctypes.c_void_p) if len(rows) else None, len(rows), ops_seen, ctypes.byref(res)))
        return {"imported": int(res.imported), "rejected": int(res.rejected)}


def region_quantize(lib, coords, size: int) -> np.ndarray:
    """wq_region_quantize (host)."""
    c = np.ascontiguousarray(coords, dtype=np.float64)
    out = np.zeros(len(c), dtype=np.int64)
    rc = lib.wq_region_quantize(c.ctypes.data_as(ctypes.c_void_p), len(c), size, out.ctypes.data_as(ctypes.c_void_p))
    if rc:
        raise ValueError(f"wq_region_quantize: {rc}")
    return out


def table_quantize(lib, region, table_size: int) -> np.ndarray:
    """wq_table_quantize (host)."""
    r = np.ascontiguousarray(region, dtype=np.int64)
    out = np.zeros(len(r), dtype=np.int64)
    rc = lib.wq_table_quantize(r.ctypes.data_as(ctypes.c_void_p), len(r), table_size,
                               out.ctypes.data_as(ctypes.c_void_p))
    if rc:
        raise ValueError(f"wq_table_quantize: {rc}")
    return out


def parse_epoch_millis(parameter: str):
    """utils/time.rs:6-16: a u64 of epoch milliseconds -> microseconds; None when it does not parse."""
    s = parameter
    if s.startswith("+"):
        s = s[1:]
    if not s or not all("0" <= ch <= "9" for ch in s):
        return None
    ms = int(s)
    if ms >= 1 << 64 or ms // 1000 > 8_210_298_412_799:  # chrono's NaiveDateTime range
        return None
    return ms * 1000


class RecordProcessor:
    """The three record instructions of processing/thread.rs around a store (`GpuRecordStore` or
    `RecordStoreRef`). The payload of a record (its data, flex and exact position) stays here, in a
    slab indexed by the `handle` the store keeps; slots of rows the store killed are freed from its
    dead list. Events are dicts: {"instruction", "world_name", "sender_uuid", "parameter",
    "position", "records"}, a record {"uuid": (hi, lo), "world_name", "position", "data", "flex"}.
    With `vacuum_dead_fraction` set, the store is vacuumed after a `process` call once more than that
    share of its stored rows is dead; the replies are the same either way."""

    def __init__(self, store, worlds: WorldIds | None = None, dedupe: bool = True,
                 vacuum_dead_fraction: float | None = None):
        self.store = store
        self.vacuum_dead_fraction = vacuum_dead_fraction
        self.vacuums = 0
        self.worlds = worlds if worlds is not None else WorldIds()
        self.dedupe = dedupe
        self.slab: list = []
        self.free: list[int] = []
        self.dropped = 0  # records and reads the reference would have dropped or failed on

    def _slot(self, record) -> int:
        if self.free:
            i = self.free.pop()
            self.slab[i] = record
            return i
        self.slab.append(record)
        return len(self.slab) - 1

    def _ops(self, kind: int, ev, now_us: int) -> list:
        ops = []
        for rec in ev.get("records") or ():
            if rec.get("position") is None:  # insert_records / delete_records: no position, no row
                self.dropped += 1
                continue
            try:
                world = self.worlds.intern(sanitize_world_name(rec["world_name"]))
            except SanitizeError:
                self.dropped += 1
                continue
            if not position_packable(self.store.sizes, world, rec["position"]):  # the store would reject it
                self.dropped += 1
                continue
            handle = self._slot(rec) if kind == CREATE else 0
            ops.append((kind, world, tuple(rec["position"]), rec["uuid"][0], rec["uuid"][1], now_us, handle))
        return ops

    def process(self, events, now_us: int) -> list:
        """One batch of decoded events in order. Creates and deletes become one apply per run of
        them, reads one read call per run of reads. Returns [(sender_uuid, world_name, records)]:
        one RecordReply per read that found something (record_read.rs:55-58)."""
        replies, ops, reads = [], [], []

        def flush_ops():
            if ops:
                arr = np.zeros(len(ops), dtype=REC_OP_DTYPE)
                for i, (k, w, p, hi, lo, t, hd) in enumerate(ops):
                    arr[i] = (k, w, p, hi, lo, t, hd, 0)
                res = self.store.apply(arr)
                self.dropped += int(res["rejected"])
                ops.clear()
                self._free_dead()

        def read_batch(batch):
            """The records of every read of `batch`, from one call: one snapshot. A sizing call (no
            dedupe, no room for rows: it changes nothing) gives the row count, then one call answers and
            dedupes. A batch the store finds too large for one call is answered in two halves."""
            world = [r[1] for r in batch]
            pos = [r[2] for r in batch]
            after = [NO_AFTER if r[3] is None else r[3] for r in batch]
            try:
                if isinstance(self.store, RecordStoreRef):
                    out = self.store.read(list(zip(world, pos, after)), dedupe=self.dedupe)
                else:
                    need = self.store.read(world, pos, after, dedupe=False, capacity=0)["returned"]
                    out = self.store.read(world, pos, after, dedupe=self.dedupe, capacity=need)
            except ReadTooLarge:
                if len(batch) == 1:
                    raise
                return read_batch(batch[: len(batch) // 2]) + read_batch(batch[len(batch) // 2:])
            off = out["offsets"]
            return [[self.slab[int(hd)] for hd in out["handles"][int(off[i]): int(off[i + 1])]]
                    for i in range(len(batch))]

        def flush_reads():
            if not reads:
                return
            for (ev, _, _, _), recs in zip(reads, read_batch(list(reads))):
                if recs:
                    replies.append((ev["sender_uuid"], ev["world_name"], recs))
            reads.clear()
            self._free_dead()

        for ev in events:
            ins = ev["instruction"]
            if ins not in ("RecordCreate", "RecordRead", "RecordDelete") or ev["world_name"] == GLOBAL_WORLD:
                continue
            if ins == "RecordRead":
                flush_ops()
                if ev.get("position") is None:
                    self.dropped += 1
                    continue
                after = None
                if ev.get("parameter") is not None:
                    after = parse_epoch_millis(ev["parameter"])
                    if after is None:  # record_read.rs:31-37: the read is dropped
                        self.dropped += 1
                        continue
                try:
                    world = self.worlds.intern(sanitize_world_name(ev["world_name"]))
                except SanitizeError:
                    self.dropped += 1
                    continue
                reads.append((ev, world, tuple(ev["position"]), after))
            else:
                flush_reads()
                ops.extend(self._ops(CREATE if ins == "RecordCreate" else DELETE, ev, now_us))
        flush_ops()
        flush_reads()
        if self.vacuum_dead_fraction is not None:
            live, stored, _ = self.store.stats()
            if stored and 1.0 - live / stored > self.vacuum_dead_fraction:
                self.store.vacuum()
                self.vacuums += 1
        return replies

    def _free_dead(self):
        for hd in self.store.drain_dead():
            self.slab[int(hd)] = None
            self.free.append(int(hd))


class DeviceRecordProcessor:
    """RecordProcessor with the per-record work on the device: a tick's frames go through the decoder, the
    dispatch and wq_records_dispatch_device (ingest.IngestTick), and the host is left with one read of the
    counters, the run table and the payload references, the copy of the created records' payloads into the
    slab, and the store calls in run order on a GpuRecordStore: apply_device on slices of the ops,
    read_device on slices of the query rows (a sizing call, then the answering call, as
    RecordProcessor.process's read_batch). The slab and the free list are RecordProcessor's; the call's
    creates take the free handles in the order RecordProcessor would pop them, then the slab's end.

    A tick is exact up to the dispatch's first_deferred: records and reads whose world name the handle's
    table does not hold are listed by the device and handed, after the tick's runs, to a RecordProcessor
    over the same store, slab and free list; the names it interns are added to the router's table, so the
    next tick resolves them on the device. A slab entry holds the record's uuid, position, data and flex;
    its world_name is the sanitized name."""

    def __init__(self, store, tick, world_names, dedupe: bool = True, compact_at: float | None = None):
        self.store, self.tick, self.router, self.dedupe = store, tick, store.router, dedupe
        self.compact_at = compact_at   # process_frames's slab: DeviceRecordSlab's policy (None: never compacts)
        self.totals_base: dict = {}    # what a restored snapshot had counted
        self.names = [n if isinstance(n, str) else bytes(n).decode("utf-8") for n in world_names]
        self.fallback = RecordProcessor(store, WorldIds(), dedupe)
        for n in self.names:
            self.fallback.worlds.intern(n)
        self.slab, self.free = self.fallback.slab, self.fallback.free   # shared with the fallback
        self.deferred = 0
        self.sizing_rejected = 0   # queries the sizing calls rejected: the answering calls count them again
        self.last_counters: dict = {}

    def totals(self) -> dict:
        """The store's totals with every rejected query of the device's runs counted once, as a store that is
        asked once counts them (the sizing call and the answering call both reject it)."""
        t = self.store.totals()
        t["rejected_queries"] -= self.sizing_rejected
        for k, v in self.totals_base.items():
            t[k] += v
        return t

    def process(self, data, offsets, now_us: int, d_frames=None, d_offsets=None) -> list:
        """One tick of frames (data u8, offsets u64[n + 1], host arrays; d_frames / d_offsets: the same on
        the device when the caller has uploaded them). Returns RecordProcessor.process's replies:
        [(sender_uuid, world_name, records)]."""
        import torch
        from . import ingest
        tick, dev = self.tick, self.tick.device
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if d_frames is None:
            d_frames = torch.from_numpy(data.copy() if len(data) else np.zeros(1, np.uint8)).to(dev)[:len(data)]
            d_offsets = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        tick.decode(d_frames, d_offsets).dispatch()
        tick.records_dispatch(d_frames, d_offsets, now_us, free_handles=self.free[::-1], handle_next=len(self.slab))
        cnt, runs = tick.read_records_ctrl()
        self.last_counters = cnt
        if cnt["overflow"] or cnt["error"]:
            raise ValueError(f"records dispatch: overflow {cnt['overflow']:#x}, error {cnt['error']:#x}")
        n_ops, off = cnt["n_creates"] + cnt["n_deletes"], [int(v) for v in offsets]
        frame = lambda f: data[off[f]:off[f + 1]].tobytes()   # noqa: E731

        # the created records' payloads, under the handles the device gave them
        if cnt["n_creates"]:
            ops, refs = tick.read_records_rows("ops", 0, n_ops), tick.read_records_rows("op_ref", 0, n_ops)
            taken = min(cnt["n_creates"], len(self.free))
            del self.free[len(self.free) - taken:]
            self.slab.extend([None] * (cnt["n_creates"] - taken))
            cache = (-1, b"")
            for op, ref in zip(ops, refs):
                if op["kind"] != CREATE:
                    continue
                if cache[0] != ref["frame"]:
                    cache = (int(ref["frame"]), frame(int(ref["frame"])))
                b = cache[1]
                self.slab[int(op["handle"])] = {
                    "uuid": (int(op["uuid_hi"]), int(op["uuid_lo"])), "world_name": self.names[int(op["world"])],
                    "position": tuple(float(c) for c in op["pos"]),
                    "data": b[ref["data_off"]:ref["data_off"] + ref["data_len"]].decode("utf-8") if ref["bits"] & 1 else None,
                    "flex": b[ref["flex_off"]:ref["flex_off"] + ref["flex_len"]] if ref["bits"] & 2 else None}

        # the runs in order
        replies, o = [], tick.r_out
        q_src = tick.read_records_rows("q_src", 0, cnt["n_read"])
        msg = tick.read_msg_rows(q_src) if cnt["n_read"] else None
        for a, b in zip(runs[:-1], runs[1:]):
            if a["kind"] == abi.RRUN_APPLY:
                lo, hi = int(a["op_begin"]), int(b["op_begin"])
                self.store.apply_device(o.ops + 64 * lo, hi - lo)
                continue
            lo, hi = int(a["q_begin"]), int(b["q_begin"])
            replies += self._read(lo, hi, q_src, msg, frame)
        self._free_dead()

        # what the device deferred: the host's, after the tick
        n_def = cnt["n_deferred_records"] + cnt["n_read_deferred"]
        if n_def:
            self.deferred += n_def
            pairs = tick.read_records_rows("defer", 0, n_def)
            frames_idx = sorted({int(p["frame"]) for p in pairs})
            rows = dict(zip(frames_idx, tick.read_msg_rows(frames_idx)))
            events = [ingest.deferred_event(frame(int(p["frame"])), rows[int(p["frame"])], int(p["record"])) for p in pairs]
            replies += self.fallback.process(events, now_us)
            if len(self.fallback.worlds) > len(self.names):
                self.names = [self.fallback.worlds.name(w) for w in range(len(self.fallback.worlds))]
                self.router.set_worlds(self.names)
        return replies

    def _read(self, lo: int, hi: int, q_src, msg, frame) -> list:
        """One read run: rows [lo, hi) of the query arrays. A batch the store finds too large for one call is
        answered in two halves, as RecordProcessor.process's read_batch."""
        import torch
        import uuid as _uuid
        o, n = self.tick.r_out, hi - lo
        d_off = torch.empty(n + 1, dtype=torch.int32, device=self.tick.device)
        args = (n, o.q_world + 4 * lo, o.q_pos + 24 * lo, o.q_after + 8 * lo)
        try:
            sizing = self.store.read_device(*args, False, d_off.data_ptr(), 0, 0, 0)
            need = sizing["returned"]
            self.sizing_rejected += sizing["rejected"]
            d_h = torch.empty(max(need, 1), dtype=torch.int32, device=self.tick.device)
            d_ts = torch.empty(max(need, 1), dtype=torch.int64, device=self.tick.device)
            self.store.read_device(*args, self.dedupe, d_off.data_ptr(), d_h.data_ptr() if need else 0,
                                   d_ts.data_ptr() if need else 0, need)
        except ReadTooLarge:
            if n == 1:
                raise
            return self._read(lo, lo + n // 2, q_src, msg, frame) + self._read(lo + n // 2, hi, q_src, msg, frame)
        off = d_off.cpu().numpy().view(np.uint32)
        handles = d_h.cpu().numpy().view(np.uint32)
        out = []
        for i in range(n):
            recs = [self.slab[int(hd)] for hd in handles[int(off[i]):int(off[i + 1])]]
            if recs:
                m = msg[lo + i]
                b = frame(int(q_src[lo + i]))
                w0 = int(m["world_off"])
                out.append((_uuid.UUID(bytes=bytes(m["sender_uuid"])), b[w0:w0 + int(m["world_len"])].decode("utf-8"), recs))
        return out

    def _free_dead(self):
        for hd in self.store.drain_dead():
            self.slab[int(hd)] = None
            self.free.append(int(hd))


    # ---- the same tick with the slab and the replies on the device ----

    def process_frames(self, data, offsets, now_us: int, d_frames=None, d_offsets=None) -> dict:
        """`process`'s tick with the payloads in a DeviceRecordSlab (`self.dslab`, filled by
        wq_slab_store_device from the frames where they lie) and the replies built by
        wq_frames_build_records_device: nothing per record happens on the host. Returns a dict of device
        tensors: frames (u8), offsets (i64[n + 1]), sizes (i32[n]) and recipients (i32[n]: the decode's
        `sender` of each answered query, -1 = 0xFFFFFFFF for a sender the table lacks), one frame per READ
        query in run order; a query that found nothing has a frame of size 0 (WQ_FRAMES_SKIP_EMPTY) and is
        sent to nobody. A reply is Message { RecordReply, the query's world name as its frame held it, the
        records, the rest default }, the bytes of the host serializer. Read back: the dispatch's counters and
        runs, the slab's and the builder's counters, the reads' totals and the store's dead list, as `process`
        reads for control. The handles are this path's own (`process` and `process_frames` do not share a
        slab: use one of them on a store). Deferred creates and deletes (a world name outside the router's
        table) go through the host after the tick, the payload by DeviceRecordSlab.put_host; a deferred
        read raises NotImplementedError: answer it with `process`."""
        import torch
        from . import ingest
        tick, dev = self.tick, self.tick.device
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if d_frames is None:
            d_frames = torch.from_numpy(data.copy() if len(data) else np.zeros(1, np.uint8)).to(dev)[:len(data)]
            d_offsets = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        if not hasattr(self, "dslab"):
            self.dslab, self.d_free, self.d_next = DeviceRecordSlab(self.router, dev, compact_at=self.compact_at), [], 0
        tick.decode(d_frames, d_offsets).dispatch()
        tick.records_dispatch(d_frames, d_offsets, now_us, free_handles=self.d_free[::-1], handle_next=self.d_next)
        cnt, runs = tick.read_records_ctrl()
        self.last_counters = cnt
        if cnt["overflow"] or cnt["error"]:
            raise ValueError(f"records dispatch: overflow {cnt['overflow']:#x}, error {cnt['error']:#x}")
        if cnt["n_read_deferred"]:
            raise NotImplementedError("process_frames: a read of a world outside the router's table; use process")
        n_ops = cnt["n_creates"] + cnt["n_deletes"]
        if cnt["n_creates"]:
            taken = min(cnt["n_creates"], len(self.d_free))
            del self.d_free[len(self.d_free) - taken:]
            self.d_next += cnt["n_creates"] - taken
            got = tick.slab_store(d_frames, d_offsets, self.dslab, n_ops)
            if got["error"]:
                raise ValueError(f"slab store: error {got['error']:#x}")
        out, o = [], tick.r_out
        for a, b in zip(runs[:-1], runs[1:]):
            if a["kind"] == abi.RRUN_APPLY:
                lo, hi = int(a["op_begin"]), int(b["op_begin"])
                self.store.apply_device(o.ops + 64 * lo, hi - lo)
                continue
            out += self._read_frames(int(a["q_begin"]), int(b["q_begin"]), d_frames, d_offsets)
        self._free_dead_device()
        if cnt["n_deferred_records"]:
            self._deferred_records(cnt, data, offsets, now_us)
        i32 = lambda: torch.zeros(0, dtype=torch.int32, device=dev)   # noqa: E731
        frames = torch.cat([x[0] for x in out]) if out else torch.zeros(0, dtype=torch.uint8, device=dev)
        sizes = torch.cat([x[1] for x in out]) if out else i32()
        off = torch.zeros(sizes.numel() + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(sizes.to(torch.int64), 0)
        return dict(frames=frames, offsets=off, sizes=sizes, recipients=torch.cat([x[2] for x in out]) if out else i32())

    def _read_frames(self, lo: int, hi: int, d_frames, d_offsets) -> list:
        """One read run on the device: rows [lo, hi) of the query arrays -> [(frames, sizes, recipients)]."""
        import torch
        tick, o, n, dev = self.tick, self.tick.r_out, hi - lo, self.tick.device
        d_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        args = (n, o.q_world + 4 * lo, o.q_pos + 24 * lo, o.q_after + 8 * lo)
        try:
            sizing = self.store.read_device(*args, False, d_off.data_ptr(), 0, 0, 0)
            need = sizing["returned"]
            self.sizing_rejected += sizing["rejected"]
            d_h = torch.empty(max(need, 1), dtype=torch.int32, device=dev)
            d_ts = torch.empty(max(need, 1), dtype=torch.int64, device=dev)
            self.store.read_device(*args, self.dedupe, d_off.data_ptr(), d_h.data_ptr() if need else 0,
                                   d_ts.data_ptr() if need else 0, need)
        except ReadTooLarge:
            if n == 1:
                raise
            return self._read_frames(lo, lo + n // 2, d_frames, d_offsets) + self._read_frames(lo + n // 2, hi, d_frames, d_offsets)
        return [tick.build_record_frames(lo, hi, d_frames, d_offsets, d_off, d_h if need else None, need, self.dslab.view())]

    def _free_dead_device(self):
        dead = self.store.drain_dead()
        if len(dead):
            self.dslab.free(dead)
            self.d_free.extend(int(h) for h in dead)

    def _deferred_records(self, cnt, data, offsets, now_us: int):
        """The deferred creates and deletes on the host, after the tick: the names are interned and added to the
        router's table, the ops applied through the host form, the created payloads put into the device slab."""
        from . import ingest
        off = [int(v) for v in offsets]
        frame = lambda f: data[off[f]:off[f + 1]].tobytes()   # noqa: E731
        pairs = self.tick.read_records_rows("defer", 0, cnt["n_deferred_records"])
        self.deferred += len(pairs)
        idx = sorted({int(p["frame"]) for p in pairs})
        rows = dict(zip(idx, self.tick.read_msg_rows(idx)))
        ops, puts = [], []
        for p in pairs:
            ev = ingest.deferred_event(frame(int(p["frame"])), rows[int(p["frame"])], int(p["record"]))
            kind = CREATE if ev["instruction"] == "RecordCreate" else DELETE
            for r in ev["records"]:
                try:
                    world = self.fallback.worlds.intern(sanitize_world_name(r["world_name"]))
                except SanitizeError:
                    continue
                if r.get("position") is None or not position_packable(self.store.sizes, world, r["position"]):
                    continue
                handle = 0
                if kind == CREATE:
                    handle = self.d_free.pop() if self.d_free else self.d_next
                    self.d_next += handle == self.d_next
                    puts.append((handle, r, world))
                ops.append((kind, world, tuple(r["position"]), r["uuid"][0], r["uuid"][1], now_us, handle, 0))
        if len(self.fallback.worlds) > len(self.names):
            self.names = [self.fallback.worlds.name(w) for w in range(len(self.fallback.worlds))]
            self.router.set_worlds(self.names)
        for handle, r, world in puts:
            self.dslab.put_host(handle, r, world)
        if ops:
            self.store.apply(np.array(ops, dtype=REC_OP_DTYPE))
            self._free_dead_device()

    # ---- process_frames's state across a restart ----

    def snapshot(self) -> dict:
        """What process_frames has built up, as a dict of numpy arrays (save_snapshot writes it): the store's
        live rows and ops_seen, its region sizes, table size and the dedupe flag, the slab in canonical form
        (DeviceRecordSlab.export), the free handles in order (the order decides which handle the next create
        gets) and the next unused handle, the totals so far and the world names as bytes plus offsets. The
        store's dead list is drained into the slab first."""
        import torch
        if not hasattr(self, "dslab"):
            self.dslab, self.d_free, self.d_next = DeviceRecordSlab(self.router, self.tick.device, compact_at=self.compact_at), [], 0
        torch.cuda.synchronize()
        self._free_dead_device()
        rows, ops_seen = self.store.export_rows()
        entries, payload = self.dslab.export()
        names = [n.encode("utf-8") for n in self.names]
        t = self.totals()
        return dict(rows=rows, ops_seen=np.array([ops_seen], np.uint64),
                    store_shape=np.array([*self.store.sizes, self.store.table_size], np.uint32),
                    dedupe=np.array([1 if self.dedupe else 0], np.uint8), slab_entries=entries, slab_payload=payload,
                    free=np.array(self.d_free, np.uint32), next=np.array([self.d_next], np.uint64),
                    totals=np.array([t[f] for f, _ in RecTotals._fields_], np.uint64),
                    world_bytes=np.frombuffer(b"".join(names), np.uint8).copy(),
                    world_off=np.cumsum([0] + [len(n) for n in names]).astype(np.uint64))

    def restore(self, snap: dict) -> dict:
        """A snapshot into this processor, which is fresh and stands over a fresh store of the snapshot's shape
        (ValueError otherwise): the rows through import_rows, the slab through DeviceRecordSlab.load, which
        validates it, the world names into the router's table, the free list, the next handle and the totals
        as they were. Returns the slab's load counters."""
        shape = [int(v) for v in snap["store_shape"]]
        if shape != [*self.store.sizes, self.store.table_size] or bool(snap["dedupe"][0]) != bool(self.dedupe):
            raise ValueError("restore: the snapshot is of a store of another shape or dedupe flag")
        if hasattr(self, "dslab"):
            raise ValueError("restore: the processor has been used")
        off, raw = [int(v) for v in snap["world_off"]], np.asarray(snap["world_bytes"], np.uint8).tobytes()
        self.names = [raw[a:b].decode("utf-8") for a, b in zip(off[:-1], off[1:])]
        self.fallback = RecordProcessor(self.store, WorldIds(), self.dedupe)
        for n in self.names:
            self.fallback.worlds.intern(n)
        self.slab, self.free = self.fallback.slab, self.fallback.free
        self.router.set_worlds(self.names)
        got = self.store.import_rows(np.asarray(snap["rows"]).view(REC_ROW_DTYPE).reshape(-1), int(snap["ops_seen"][0]))
        if got["rejected"]:
            raise ValueError(f"restore: the store rejected {got['rejected']} rows")
        self.dslab = DeviceRecordSlab(self.router, self.tick.device, compact_at=self.compact_at)
        cnt = self.dslab.load(np.asarray(snap["slab_entries"]).view(abi.SLAB_ENTRY_DTYPE).reshape(-1), snap["slab_payload"])
        self.d_free, self.d_next = [int(h) for h in snap["free"]], int(snap["next"][0])
        self.totals_base = {f: int(v) for (f, _), v in zip(RecTotals._fields_, snap["totals"])}
        return cnt


# ---- the record payload slab (wq_slab_store_device, csrc/wq_slab.hip) ----

def slab_store_np(ops, op_ref, frames, offsets, entries, payload, cursor: int):
    """The definition of wq_slab_store_device: the header's rules in plain Python. ops (REC_OP_DTYPE) and
    op_ref (abi.REC_OP_REF_DTYPE) as the record dispatch wrote them, frames u8 / offsets u64[n_frames + 1]
    the tick's frames, entries (abi.SLAB_ENTRY_DTYPE) and payload (u8) the slab, cursor the arena's fill.
    Returns (entries, payload, cursor, counters): copies with the call applied, or unchanged after an
    overflow, and the counters as a dict with abi.SLAB_COUNTERS_DTYPE's fields."""
    ops = np.ascontiguousarray(ops, dtype=REC_OP_DTYPE)
    op_ref = np.ascontiguousarray(op_ref, dtype=abi.REC_OP_REF_DTYPE)
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    fo = [int(v) for v in np.ascontiguousarray(offsets, dtype=np.uint64)]
    n_frames = max(len(fo) - 1, 0)
    n_frame_bytes = fo[n_frames] if n_frames else 0
    entries, payload = np.array(entries, dtype=abi.SLAB_ENTRY_DTYPE), np.array(payload, dtype=np.uint8)
    error, at, need, plan = 0, int(cursor), 0, []
    for op, ref in zip(ops, op_ref):
        if int(op["kind"]) != CREATE:
            continue
        bits = int(ref["bits"]) & 3
        want = [(int(ref["data_off"]), int(ref["data_len"]) if bits & 1 else 0),
                (int(ref["flex_off"]), int(ref["flex_len"]) if bits & 2 else 0)]
        parts = [b"", b""]
        if want[0][1] or want[1][1]:   # nothing to copy: the frame is not looked at
            f = int(ref["frame"])
            ok = f < n_frames and fo[f] <= fo[f + 1] <= n_frame_bytes
            if not ok:
                error |= abi.SLAB_ERROR_FRAME
            else:
                for k, (o, ln) in enumerate(want):
                    if not ln:
                        continue
                    if o + ln > fo[f + 1] - fo[f]:
                        error |= abi.SLAB_ERROR_FLEX if k else abi.SLAB_ERROR_DATA
                        continue
                    parts[k] = frames[fo[f] + o:fo[f] + o + ln].tobytes()
        need = max(need, int(op["handle"]) + 1)
        plan.append((op, bits, at, parts))
        at += len(parts[0]) + len(parts[1])
    total = at - int(cursor)
    overflow = (abi.SLAB_OVERFLOW_ARENA if int(cursor) > len(payload) or total > len(payload) - int(cursor) else 0) | \
               (abi.SLAB_OVERFLOW_ENTRIES if need > len(entries) else 0)
    if not overflow:
        for op, bits, off, parts in plan:
            e = entries[int(op["handle"])]
            e["uuid"] = np.frombuffer(int(op["uuid_hi"]).to_bytes(8, "big") + int(op["uuid_lo"]).to_bytes(8, "big"), np.uint8)
            e["pos"], e["world"] = op["pos"], op["world"]
            e["bits"] = bits | abi.SLAB_POSITION | abi.SLAB_LIVE
            e["off"], e["data_len"], e["flex_len"] = off, len(parts[0]), len(parts[1])
            blob = parts[0] + parts[1]
            payload[off:off + len(blob)] = np.frombuffer(blob, np.uint8)
    counters = dict(n_ops=len(ops), n_creates=len(plan), bytes_stored=total, bytes_need=min(int(cursor) + total, 2**64 - 1),
                    entries_need=need, cursor=int(cursor) if overflow else at, overflow=overflow, error=error)
    return entries, payload, counters["cursor"], counters


def slab_counters(raw) -> dict:
    """abi.SLAB_COUNTERS_DTYPE bytes as slab_store_np's counters dict."""
    c = np.frombuffer(bytes(raw), dtype=abi.SLAB_COUNTERS_DTYPE)[0]
    return {k: int(c[k]) for k in abi.SLAB_COUNTERS_DTYPE.names}


# ---- slab compaction (wq_slab_compact_device, csrc/wq_slab_compact.hip) ----

def slab_compact_np(entries, payload, n_dst_entries: int, n_dst_bytes: int, dst=None):
    """The definition of wq_slab_compact_device: the header's rules in plain Python. entries
    (abi.SLAB_ENTRY_DTYPE) and payload (u8) are the source slab, n_dst_entries / n_dst_bytes the sizes of the
    destination; dst = (entries, payload, cursor) is the destination as it stands before the call (zeros and
    cursor 0 when None). Returns (entries, payload, cursor, counters): the destination with the call applied,
    or unchanged after an overflow, and the counters as a dict with abi.SLAB_COMPACT_COUNTERS_DTYPE's fields."""
    src = np.ascontiguousarray(entries, dtype=abi.SLAB_ENTRY_DTYPE)
    arena = np.ascontiguousarray(payload, dtype=np.uint8)
    if dst is None:
        dst = (np.zeros(n_dst_entries, abi.SLAB_ENTRY_DTYPE), np.zeros(n_dst_bytes, np.uint8), 0)
    d_ent, d_pay, cursor = np.array(dst[0], dtype=abi.SLAB_ENTRY_DTYPE), np.array(dst[1], dtype=np.uint8), int(dst[2])
    assert len(d_ent) == n_dst_entries and len(d_pay) == n_dst_bytes
    n, error, at, need, plan = len(arena), 0, 0, 0, []
    for i in np.flatnonzero(src["bits"] & np.uint32(abi.SLAB_LIVE)):
        i, e = int(i), src[i]
        off, dl, fl = int(e["off"]), int(e["data_len"]), int(e["flex_len"])
        if off + dl + fl > n:        # Python integers: no wrap
            error |= abi.SLAB_COMPACT_ERROR_RANGE
            off = dl = fl = 0
        plan.append((i, at, off, dl, fl))
        at += dl + fl
        need = i + 1
    total = min(at, 2**64 - 1)
    overflow = (abi.SLAB_OVERFLOW_ARENA if total > n_dst_bytes else 0) | (abi.SLAB_OVERFLOW_ENTRIES if need > n_dst_entries else 0)
    if not overflow:
        d_ent[:] = np.zeros(1, abi.SLAB_ENTRY_DTYPE)[0]
        for i, to, off, dl, fl in plan:
            d_ent[i] = src[i]
            d_ent[i]["off"], d_ent[i]["data_len"], d_ent[i]["flex_len"] = to, dl, fl
            d_pay[to:to + dl + fl] = arena[off:off + dl + fl]
        cursor = total
    counters = dict(n_entries=len(src), n_live=len(plan), bytes_live=total, entries_need=need, overflow=overflow, error=error)
    return d_ent, d_pay, cursor, counters


SNAPSHOT_KEYS = ("rows", "ops_seen", "store_shape", "dedupe", "slab_entries", "slab_payload", "free", "next", "totals",
                 "world_bytes", "world_off")


def save_snapshot(path, snap: dict) -> None:
    """DeviceRecordProcessor.snapshot's dict in one .npz, without pickle: the structured arrays (rows, slab
    entries) go in as their bytes."""
    flat = {k: np.ascontiguousarray(snap[k]) for k in SNAPSHOT_KEYS}
    for k in ("rows", "slab_entries"):
        flat[k] = flat[k].view(np.uint8).reshape(-1)
    with open(path, "wb") as f:
        np.savez(f, **flat)


def load_snapshot(path) -> dict:
    """save_snapshot's file as the dict DeviceRecordProcessor.restore takes (ValueError: a file that is not one)."""
    with np.load(path, allow_pickle=False) as z:
        if set(z.files) != set(SNAPSHOT_KEYS):
            raise ValueError("load_snapshot: not a record snapshot")
        snap = {k: z[k] for k in SNAPSHOT_KEYS}
    if len(snap["rows"]) % REC_ROW_DTYPE.itemsize or len(snap["slab_entries"]) % abi.SLAB_ENTRY_DTYPE.itemsize:
        raise ValueError("load_snapshot: rows or slab entries are not whole")
    snap["rows"] = snap["rows"].view(REC_ROW_DTYPE)
    snap["slab_entries"] = snap["slab_entries"].view(abi.SLAB_ENTRY_DTYPE)
    return snap


def slab_compact_counters(raw) -> dict:
    """abi.SLAB_COMPACT_COUNTERS_DTYPE bytes as slab_compact_np's counters dict."""
    c = np.frombuffer(bytes(raw), dtype=abi.SLAB_COMPACT_COUNTERS_DTYPE)[0]
    return {k: int(c[k]) for k in abi.SLAB_COMPACT_COUNTERS_DTYPE.names}


class DeviceRecordSlab:
    """The payload slab in device memory: torch tensors for the entries (abi.SLAB_ENTRY_DTYPE, indexed by
    the store's handle) and the byte arena, and the arena's fill as a device word. `store` is
    Router.slab_store_device with grow-and-retry: the one read-back is the call's counters. `free` clears
    the live bit of dead handles and adds their payload bytes to the dead count: `dead_bytes` says how much
    of the arena nothing refers to any more. `put_host` stores one record the host holds (what the host
    fallback creates from deferred records).

    `compact` rewrites the slab through Router.slab_compact_device into fresh tensors, live payloads back to
    back in handle order, and swaps them in; `export` / `load` are the same call into a buffer the host reads
    and from one it uploaded. compact_at (None: never, the default) is the opt-in policy: `free` compacts when
    dead_bytes / cursor reaches it, and a `store` that overflows grows by compacting into the larger arena
    instead of copying the dead bytes along."""

    def __init__(self, router, device, n_entries: int = 1024, n_payload_bytes: int = 1 << 16, compact_at: float | None = None):
        import torch
        self.router, self.device = router, device
        self.compact_at = compact_at
        self.compactions = 0
        self._floor_bytes = max(n_payload_bytes, 16)   # a compaction does not shrink the arena below it
        # zeros, and waited for: the calls run on the handle's stream, not torch's
        self.entries = torch.zeros(max(n_entries, 1), 8, dtype=torch.int64, device=device)
        self.payload = torch.zeros(max(n_payload_bytes, 16), dtype=torch.uint8, device=device)
        self.ctrl = torch.zeros(8 + abi.SLAB_COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=device)  # cursor, counters
        self.dead = torch.zeros(1, dtype=torch.int64, device=device)
        self.cursor = 0          # the host's mirror of the device word, as of the last store
        self.grows = 0
        torch.cuda.synchronize()

    @property
    def n_entries(self) -> int:
        return self.entries.shape[0]

    @property
    def n_payload_bytes(self) -> int:
        return self.payload.numel()

    @property
    def dead_bytes(self) -> int:
        """Arena bytes of freed entries (one read-back)."""
        return int(self.dead.item())

    def view(self) -> "abi.SlabView":
        return abi.SlabView(entries=self.entries.data_ptr(), n_entries=self.n_entries, payload=self.payload.data_ptr(),
                            n_payload_bytes=self.n_payload_bytes)

    def _grow(self, n_entries: int, n_bytes: int) -> None:
        import torch
        if n_entries <= self.n_entries and n_bytes <= self.n_payload_bytes:
            return
        torch.cuda.synchronize()
        if n_entries > self.n_entries:
            new = torch.zeros(max(n_entries, 2 * self.n_entries), 8, dtype=torch.int64, device=self.device)
            new[:self.n_entries] = self.entries
            self.entries = new
        if n_bytes > self.n_payload_bytes:
            new = torch.zeros(max(n_bytes, 2 * self.n_payload_bytes), dtype=torch.uint8, device=self.device)
            new[:self.cursor] = self.payload[:self.cursor]
            self.payload = new
        self.grows += 1
        torch.cuda.synchronize()

    def store(self, ops_ptr: int, op_ref_ptr: int, n_ops: int, frames_ptr: int, frame_offsets_ptr: int, n_frames: int) -> dict:
        """One wq_slab_store_device call on device arrays; after an overflow the slab grows to what the
        counters ask for and the call is repeated once. Returns the counters of the call that fitted."""
        import torch
        for _ in range(2):
            self.router.slab_store_device(ops_ptr, op_ref_ptr, n_ops, frames_ptr, frame_offsets_ptr, n_frames, self.view(),
                                          self.ctrl.data_ptr(), self.ctrl.data_ptr() + 8)
            torch.cuda.synchronize()
            cnt = slab_counters(self.ctrl[8:].cpu().numpy())
            if not cnt["overflow"]:
                self.cursor = cnt["cursor"]
                return cnt
            if self.compact_at is None:
                self._grow(cnt["entries_need"], cnt["bytes_need"])
            else:
                self.compact(min_entries=cnt["entries_need"], extra_bytes=cnt["bytes_stored"])
                self.grows += 1
        raise RuntimeError(f"slab store: overflow {cnt['overflow']:#x} after growing")

    def free(self, handles) -> None:
        """Clears the live bit of the given handles' entries (a torch index write); their payload bytes count
        as dead. Handles that are not live, or past the entries, change nothing."""
        import torch
        hd = np.unique(np.asarray(handles, dtype=np.int64))
        hd = hd[hd < self.n_entries]
        if not len(hd):
            return
        idx = torch.from_numpy(hd).to(self.device)
        w5, w7 = self.entries[idx, 5], self.entries[idx, 7]
        live = w5 < 0   # bit 31 of `bits` is the word's sign
        self.dead += torch.where(live, (w7 & 0xFFFFFFFF) + ((w7 >> 32) & 0xFFFFFFFF), torch.zeros_like(w7)).sum()
        self.entries[idx, 5] = w5 & 0x7FFFFFFFFFFFFFFF
        torch.cuda.synchronize()
        if self.compact_at is not None and self.cursor and self.dead_bytes >= self.compact_at * self.cursor:
            self.compact()

    # ---- the canonical form: compaction, export, load (Router.slab_compact_device) ----

    def _rewrite(self, src: "abi.SlabView", n_entries: int, n_bytes: int, cursor_ptr: int, extra_bytes: int = 0):
        """`src` compacted into fresh tensors of at least n_entries / n_bytes, the total into the device word at
        cursor_ptr; after an overflow the sizes come from the counters and the call is repeated once.
        Returns (entries, payload, counters): one read-back a call."""
        import torch
        for _ in range(2):
            ent = torch.empty(n_entries, 8, dtype=torch.int64, device=self.device)
            pay = torch.empty(n_bytes, dtype=torch.uint8, device=self.device)
            dst = abi.SlabView(entries=ent.data_ptr() if n_entries else None, n_entries=n_entries,
                               payload=pay.data_ptr() if n_bytes else None, n_payload_bytes=n_bytes)
            torch.cuda.synchronize()   # the call runs on the handle's stream, not torch's
            self.router.slab_compact_device(src, dst, cursor_ptr, self.ctrl.data_ptr() + 8)
            torch.cuda.synchronize()
            cnt = slab_compact_counters(self.ctrl[8:8 + abi.SLAB_COMPACT_COUNTERS_DTYPE.itemsize].cpu().numpy())
            if not cnt["overflow"]:
                return ent, pay, cnt
            n_entries, n_bytes = max(n_entries, cnt["entries_need"]), max(n_bytes, cnt["bytes_live"] + extra_bytes)
        raise RuntimeError(f"slab compact: overflow {cnt['overflow']:#x} after resizing")

    def _adopt(self, ent, pay, cnt) -> None:
        import torch
        self.entries, self.payload, self.cursor = ent, pay, cnt["bytes_live"]
        self.dead.zero_()
        torch.cuda.synchronize()

    def compact(self, min_entries: int = 0, extra_bytes: int = 0) -> dict:
        """The slab compacted into fresh tensors and swapped in: live payloads back to back in handle order
        from byte 0, dead entries zeroed, the cursor (device word and mirror) at the live bytes and `dead_bytes`
        0. The new arena is sized from the host's cursor and one read of `dead`, twice the live bytes plus
        extra_bytes and not below the constructor's size; the entries keep their count, or grow to
        min_entries. Returns the call's counters plus "reclaimed", the bytes the cursor fell by."""
        before = self.cursor
        live = max(self.cursor - self.dead_bytes, 0)
        n_entries = self.n_entries if min_entries <= self.n_entries else max(min_entries, 2 * self.n_entries)
        ent, pay, cnt = self._rewrite(self.view(), n_entries, max(2 * (live + extra_bytes), self._floor_bytes),
                                      self.ctrl.data_ptr(), extra_bytes)
        self._adopt(ent, pay, cnt)
        self.compactions += 1
        return dict(cnt, reclaimed=before - self.cursor)

    def export(self):
        """(entries as abi.SLAB_ENTRY_DTYPE, payload u8) in canonical form, as numpy: the entries up to the
        highest live handle, the live payloads back to back. A sizing call, then the compaction into scratch
        tensors of exactly that size, read back; the slab itself is not changed."""
        import torch
        word = torch.zeros(1, dtype=torch.int64, device=self.device)
        ent, pay, _ = self._rewrite(self.view(), 0, 0, word.data_ptr())
        return (ent.cpu().numpy().reshape(-1).view(abi.SLAB_ENTRY_DTYPE).copy(), pay.cpu().numpy().copy())

    def load(self, entries, payload) -> dict:
        """A slab from the host (what `export` returned, or any entries and arena bytes) uploaded to staging
        and compacted into this slab's own tensors, which replaces what it held. The call is the validator: an
        entry whose range leaves `payload` comes out live and empty, with error bit 0 in the returned counters."""
        import torch
        e = np.ascontiguousarray(entries, dtype=abi.SLAB_ENTRY_DTYPE)
        b = np.ascontiguousarray(payload, dtype=np.uint8)
        s_ent = torch.from_numpy(e.view(np.int64).reshape(-1, 8).copy()).to(self.device)
        s_pay = torch.from_numpy(b.copy()).to(self.device)
        src = abi.SlabView(entries=s_ent.data_ptr() if len(e) else None, n_entries=len(e),
                           payload=s_pay.data_ptr() if len(b) else None, n_payload_bytes=len(b))
        ent, pay, cnt = self._rewrite(src, max(self.n_entries, len(e)), max(2 * len(b), self._floor_bytes), self.ctrl.data_ptr())
        self._adopt(ent, pay, cnt)
        return cnt

    def put_host(self, handle: int, record: dict, world: int) -> None:
        """One record from the host under `handle`: {"uuid": (hi, lo), "position", "data" (str or None),
        "flex" (bytes or None)}; world: its id in the router's table. Per-record host work (three small uploads
        and a device synchronise a record): it is for the few records the host fallback creates from deferred
        entries, not for a tick's creates."""
        import torch
        data = None if record.get("data") is None else record["data"].encode("utf-8")
        flex = None if record.get("flex") is None else bytes(record["flex"])
        blob = (data or b"") + (flex or b"")
        if handle >= self.n_entries or self.cursor + len(blob) > self.n_payload_bytes:
            self._grow(handle + 1, self.cursor + len(blob))
        e = np.zeros(1, dtype=abi.SLAB_ENTRY_DTYPE)
        e["uuid"][0] = np.frombuffer(int(record["uuid"][0]).to_bytes(8, "big") + int(record["uuid"][1]).to_bytes(8, "big"), np.uint8)
        e["pos"][0], e["world"] = record["position"], world
        e["bits"] = (abi.SLAB_DATA if data is not None else 0) | (abi.SLAB_FLEX if flex is not None else 0) | \
            abi.SLAB_POSITION | abi.SLAB_LIVE
        e["off"], e["data_len"], e["flex_len"] = self.cursor, len(data or b""), len(flex or b"")
        self.entries[handle] = torch.from_numpy(e.view(np.int64).copy()).to(self.device)
        if blob:
            self.payload[self.cursor:self.cursor + len(blob)] = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(self.device)
        self.cursor += len(blob)
        self.ctrl[:8] = torch.from_numpy(np.array([self.cursor], np.uint64).view(np.uint8).copy()).to(self.device)
        torch.cuda.synchronize()

    def read(self):
        """(entries as abi.SLAB_ENTRY_DTYPE, the arena's bytes below the cursor): synchronizes; for tests."""
        import torch
        torch.cuda.synchronize()
        return (self.entries.cpu().numpy().reshape(-1).view(abi.SLAB_ENTRY_DTYPE).copy(),
                self.payload[:self.cursor].cpu().numpy().copy())

    def get(self, handle: int, raw_data: bool = False):
        """The record under `handle` as put_host takes it, plus "world"; None when it is not live (reads back).
        raw_data: `data` as the bytes the arena holds, not decoded."""
        e = self.entries[handle].cpu().numpy().view(abi.SLAB_ENTRY_DTYPE)[0]
        if not int(e["bits"]) & abi.SLAB_LIVE:
            return None
        off, dl, fl = int(e["off"]), int(e["data_len"]), int(e["flex_len"])
        raw = self.payload[off:off + dl + fl].cpu().numpy().tobytes()
        u = bytes(e["uuid"])
        return {"uuid": (int.from_bytes(u[:8], "big"), int.from_bytes(u[8:], "big")), "world": int(e["world"]),
                "position": tuple(float(c) for c in e["pos"]),
                "data": (raw[:dl] if raw_data else raw[:dl].decode("utf-8")) if int(e["bits"]) & abi.SLAB_DATA else None,
                "flex": raw[dl:] if int(e["bits"]) & abi.SLAB_FLEX else None}
