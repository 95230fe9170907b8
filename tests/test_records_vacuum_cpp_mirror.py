"""The vacuum, export and import arithmetic of csrc/record_ops.hpp on the CPU
(tests/cpp/records_vacuum_host_shim.hip: rec_row_move, rec_row_export, rec_row_import and
rec_adjacent_equal in the flag / scan / move / remap and classify / sort / check shape of
wq_records.hip) against RecordStoreRef, byte for byte: the shared scripts with a vacuum or an
export / import after every step, and the hand-written cases of test_records_vacuum_host.py. Needs
hipcc only, no GPU. Every output array is followed by canary words that must survive the call; the
shim keeps its own canaries behind every array a vacuum or an import writes (return code -100).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from worldql_server_amd import records as R

from test_records_host import cases
from test_records_vacuum_host import CASES, case_processor_vacuums_unseen, points_of, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 16
MARK32, MARK64 = 0xA5A5A5A5, -0x5A5A5A5A5A5A5A5B

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("records_vacuum_shim") / "librecordsvacuumshim.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-o", out, os.path.join(ROOT, "tests", "cpp", "records_vacuum_host_shim.hip")])
    lib = ctypes.CDLL(out)
    vp, sz, u32, u16, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint64
    lib.wq_test_rec_open.restype, lib.wq_test_rec_open.argtypes = vp, [u16, u16, u16, u32]
    lib.wq_test_rec_close.restype, lib.wq_test_rec_close.argtypes = None, [vp]
    lib.wq_test_rec_apply.restype, lib.wq_test_rec_apply.argtypes = None, [vp, vp, sz, vp]
    lib.wq_test_rec_read.restype, lib.wq_test_rec_read.argtypes = ctypes.c_int, [vp, sz, vp, vp, vp, u32, vp, vp, vp, sz, vp]
    lib.wq_test_rec_drain.restype, lib.wq_test_rec_drain.argtypes = sz, [vp, vp, sz]
    lib.wq_test_rec_stats.restype, lib.wq_test_rec_stats.argtypes = None, [vp, vp]
    lib.wq_test_rec_vacuum.restype, lib.wq_test_rec_vacuum.argtypes = ctypes.c_int, [vp, vp]
    lib.wq_test_rec_export.restype, lib.wq_test_rec_export.argtypes = ctypes.c_int, [vp, vp, sz, ctypes.POINTER(sz),
                                                                                      ctypes.POINTER(u64)]
    lib.wq_test_rec_import.restype, lib.wq_test_rec_import.argtypes = ctypes.c_int, [vp, vp, sz, u64, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Refused(Exception):
    pass


class ShimStore:
    """The shim's host store behind the interface of test_records_vacuum_host.RefStore. The totals
    are summed here from the calls' results (the shim keeps none)."""
    refused = Refused

    def __init__(self, lib, cfg):
        self.lib, self.cfg, self.st = lib, tuple(cfg), lib.wq_test_rec_open(*cfg)
        self.totals_ = {"created": 0, "deleted_rows": 0, "deduped_rows": 0, "rejected_ops": 0, "rejected_queries": 0}

    def close(self):
        if self.st:
            self.lib.wq_test_rec_close(self.st)
        self.st = None

    def apply(self, ops):
        ops = np.ascontiguousarray(ops, dtype=R.REC_OP_DTYPE)
        res = R.RecApplyResult()
        self.lib.wq_test_rec_apply(self.st, _p(ops), len(ops), ctypes.byref(res))
        for k, f in (("created", "created"), ("deleted_rows", "deleted_rows"), ("rejected_ops", "rejected")):
            self.totals_[k] += getattr(res, f)
        return {"created": res.created, "deleted_rows": res.deleted_rows, "rejected": res.rejected,
                "rows_live": res.rows_live}

    def _read(self, world, pos, after, dedupe, cap):
        world = np.ascontiguousarray(world, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        n = len(world)
        off = np.full(n + 1 + CANARY, MARK32, np.uint32)
        hd = np.full(cap + CANARY, MARK32, np.uint32)
        ts = np.full(cap + CANARY, MARK64, np.int64)
        res = R.RecReadResult()
        rc = self.lib.wq_test_rec_read(self.st, n, _p(world), _p(pos), None if after is None else _p(after), int(dedupe),
                                       _p(off), _p(hd), _p(ts), cap, ctypes.byref(res))
        assert rc == 0
        k = min(cap, int(res.returned))
        assert (off[n + 1:] == MARK32).all() and (hd[k:] == MARK32).all() and (ts[k:] == MARK64).all(), "canaries"
        self.totals_["deduped_rows"] += res.deduped_rows
        self.totals_["rejected_queries"] += res.rejected
        out = {f: int(getattr(res, f)) for f, _ in R.RecReadResult._fields_}
        out.update(offsets=off[: n + 1], handles=hd[:k], ts_us=ts[:k])
        return out

    def step(self, step, want_res):
        if step[0] == "apply":
            return self.apply(step[1])
        _, world, pos, after, dedupe, cap = step
        return self._read(world, pos, after, dedupe, int(want_res["returned"]) if cap is None else cap)

    def read(self, qs, dedupe=False):
        world, pos = [q[0] for q in qs], [q[1] for q in qs]
        need = self._read(world, pos, None, False, 0)["returned"]
        return self._read(world, pos, None, dedupe, need)

    def drain_dead(self):
        n = self.lib.wq_test_rec_drain(self.st, None, 0)
        out = np.full(n + CANARY, MARK32, np.uint32)
        assert self.lib.wq_test_rec_drain(self.st, _p(out), n) == n and (out[n:] == MARK32).all()
        return out[:n]

    def stats(self):
        st = np.zeros(3, np.uint64)
        self.lib.wq_test_rec_stats(self.st, _p(st))
        return tuple(int(v) for v in st)

    def totals(self):
        return dict(self.totals_)

    def vacuum(self):
        res = R.RecVacuumResult()
        assert self.lib.wq_test_rec_vacuum(self.st, ctypes.byref(res)) == 0, "a canary behind a fresh array died"
        return {"rows_before": int(res.rows_before), "rows_after": int(res.rows_after)}

    def export_rows(self):
        n, ops = ctypes.c_size_t(), ctypes.c_uint64()
        live = self.stats()[0]
        if live:  # one short: nothing is written
            short = np.full((live - 1) * 8 + CANARY, MARK64, np.int64)
            rc = self.lib.wq_test_rec_export(self.st, _p(short), live - 1, ctypes.byref(n), ctypes.byref(ops))
            assert rc == -5 and n.value == live and (short == MARK64).all()
        buf = np.full(live * 8 + CANARY, MARK64, np.int64)
        rc = self.lib.wq_test_rec_export(self.st, _p(buf), live, ctypes.byref(n), ctypes.byref(ops))
        assert rc == 0 and n.value == live and (buf[live * 8:] == MARK64).all()
        return buf[: live * 8].view(R.REC_ROW_DTYPE).copy(), ops.value

    def import_rows(self, rows, ops_seen):
        rows = np.ascontiguousarray(rows, dtype=R.REC_ROW_DTYPE)
        res = R.RecImportResult()
        rc = self.lib.wq_test_rec_import(self.st, _p(rows), len(rows), ops_seen, ctypes.byref(res))
        if rc == -1:  # WQ_E_INVALID
            raise Refused()
        assert rc == 0, rc
        self.totals_ = {k: 0 for k in self.totals_}
        return {"imported": int(res.imported), "rejected": int(res.rejected)}


@pytest.fixture
def open_shim(shim):
    return lambda cfg, which=0: ShimStore(shim, cfg)


@pytest.mark.parametrize("form", ["vacuum", "snapshot"])
@pytest.mark.parametrize("name", sorted(cases()))
def test_invisible_in_every_shared_script(open_shim, name, form):
    dropped = sum(replay(open_shim, name, form, pts) for pts in points_of(name))
    if name in ("random_stream", "deletes", "duplicates", "capacity", "one_region_many_queries"):
        assert dropped > 0


@pytest.mark.parametrize("case", [c for c in CASES if c is not case_processor_vacuums_unseen], ids=lambda c: c.__name__)
def test_hand_written(open_shim, case):
    case(open_shim)
