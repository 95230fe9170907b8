"""Python binding of the C ABI (include/wq_router.h) — the HIP routing library, nothing else.

`Router` is a thin ctypes wrapper; every compute call runs the gfx950 kernels of
libwq_router.so. There is no CPU fallback: without the library or without a gfx950 device the
constructor raises `WQError`.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import abi

PKG = os.path.dirname(os.path.abspath(__file__))
# WQ_LIBRARY: another in-tree build of the same sources (A/B timing of a kernel variant on one box)
LIB_PATH = os.environ.get("WQ_LIBRARY") or os.path.join(PKG, "libwq_router.so")

_lib = None

# typedef int (*wq_exchange_fn)(void* ctx, const void* d_send, const size_t* send_bytes, void* d_recv,
#                               const size_t* recv_bytes, void* hip_stream)
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t),
                               ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p)


class WQError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"wq error {code}: {msg}")
        self.code = code


class FollowResult(ctypes.Structure):  # struct wq_follow_result
    _fields_ = [("n_unsubscribe", ctypes.c_uint64), ("n_subscribe", ctypes.c_uint64),
                ("n_followed", ctypes.c_uint64)]


def load_library(build_if_missing: bool = True):
    """Load libwq_router.so (building it with hipcc if it is absent and hipcc exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if not build_if_missing or not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
            raise ImportError(f"{LIB_PATH} is missing: run `python -m worldql_server_amd.build`")
        from .build import build
        build()
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7. Loading torch
    # first makes this library's libamdhip64.so.7 dependency resolve to that same copy (two
    # runtimes in one process do not share devices). Without torch the system runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    vp, sz, u32, u16, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_int
    sig = {
        "wq_router_create": ([u16, i32, ctypes.POINTER(vp)], i32),
        "wq_router_create_multi": ([u16, i32, vp, ctypes.POINTER(vp)], i32),
        "wq_multi_info": ([vp, ctypes.POINTER(u32)], i32),
        "wq_router_create_multi_mode": ([u16, i32, vp, i32, ctypes.POINTER(vp)], i32),
        "wq_multi_mode": ([vp, ctypes.POINTER(i32)], i32),
        "wq_route_tick_slices_device": ([vp, vp, i32, vp], i32),
        "wq_shard_tick_stats": ([vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)], i32),
        "wq_router_destroy": ([vp], i32),
        "wq_last_error": ([vp], ctypes.c_char_p),
        "wq_set_stream": ([vp, vp], i32),
        "wq_get_stats": ([vp, vp], i32),
        "wq_apply_ops": ([vp, vp, sz], i32),
        "wq_host_alloc": ([sz, ctypes.POINTER(vp)], i32),
        "wq_host_free": ([vp], i32),
        "wq_apply_ops_device": ([vp, vp, sz], i32),
        "wq_remove_peers": ([vp, vp, sz], i32),
        "wq_route_tick": ([vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, ctypes.POINTER(sz)], i32),
        "wq_route_tick_device": ([vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp], i32),
        "wq_route_global": ([vp, vp, vp, vp, sz, vp, vp, vp, sz, ctypes.POINTER(sz)], i32),
        "wq_route_global_device": ([vp, vp, vp, vp, sz, vp, vp, vp, sz, vp], i32),
        "wq_peer_major_device": ([vp, vp, vp, sz, sz, vp, u32, vp, vp], i32),
        "wq_tick_sends_device": ([vp, ctypes.POINTER(abi.TickSendsIn), vp, vp, sz, vp], i32),
        "wq_peer_budget_device": ([vp, vp, vp, u32, sz, vp, sz, vp, sz, u32, vp, vp, vp, vp], i32),
        "wq_peer_budget_bytes_device": ([vp, vp, vp, u32, sz, vp, vp, sz, vp, sz, ctypes.c_uint64, vp, vp, vp, vp, vp],
                                        i32),
        "wq_peer_rotate_device": ([vp, vp, vp, u32, sz, vp, vp, sz, vp, sz, u32, vp, ctypes.c_uint64, vp, vp, vp, vp, vp,
                                   vp], i32),
        "wq_peer_pack_device": ([vp, vp, vp, u32, sz, vp, vp, sz, sz, u32, vp, sz, vp, vp, vp], i32),
        "wq_frames_set_worlds": ([vp, vp, vp, u32], i32),
        "wq_frames_build_device": ([vp, ctypes.POINTER(abi.FramesSrc), sz, vp, sz, vp, vp, vp], i32),
        "wq_ingest_set_peers": ([vp, vp, vp, u32], i32),
        "wq_frames_decode_device": ([vp, vp, vp, sz, sz, ctypes.POINTER(abi.IngestOut), vp], i32),
        "wq_debug_set_ingest_list": ([vp, ctypes.c_int64], i32),
        "wq_ingest_dispatch_device": ([vp, ctypes.POINTER(abi.DispatchIn), sz, ctypes.POINTER(abi.DispatchOut), vp], i32),
        "wq_ingest_peers_reserve": ([vp, sz], i32),
        "wq_ingest_join_device": ([vp, ctypes.POINTER(abi.JoinIn), sz, ctypes.POINTER(abi.JoinOut), vp], i32),
        "wq_ingest_drop_peers_device": ([vp, vp, sz, vp], i32),
        "wq_ingest_leave_device": ([vp, ctypes.POINTER(abi.LeaveIn), ctypes.POINTER(abi.LeaveOut), vp], i32),
        "wq_remove_peers_device": ([vp, vp, ctypes.c_uint32, vp], i32),
        "wq_ingest_peers_read": ([vp, vp, vp, sz, ctypes.POINTER(sz)], i32),
        "wq_csr_diff_device": ([vp, sz, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp], i32),
        "wq_csr_diff": ([vp, sz, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, vp, sz, ctypes.POINTER(sz),
                         ctypes.POINTER(sz)], i32),
        "wq_records_dispatch_device": ([vp, ctypes.POINTER(abi.RecDispatchIn), ctypes.POINTER(abi.RecDispatchOut), vp], i32),
        "wq_frames_build_records_device": ([vp, ctypes.POINTER(abi.FramesSrc), ctypes.POINTER(abi.FramesRecSrc), sz, vp, sz, vp, vp, vp], i32),
        "wq_slab_store_device": ([vp, vp, vp, sz, vp, vp, sz, ctypes.POINTER(abi.SlabView), vp, vp], i32),
        "wq_slab_compact_device": ([vp, ctypes.POINTER(abi.SlabView), ctypes.POINTER(abi.SlabView), vp, vp], i32),
        "wq_records_open": ([vp, u16, u16, u16, u32], i32),
        "wq_records_close": ([vp], i32),
        "wq_records_apply": ([vp, vp, sz, vp], i32),
        "wq_records_apply_device": ([vp, vp, sz], i32),
        "wq_records_read": ([vp, sz, vp, vp, vp, u32, vp, vp, vp, sz, vp], i32),
        "wq_records_read_device": ([vp, sz, vp, vp, vp, u32, vp, vp, vp, sz, vp], i32),
        "wq_records_drain_dead": ([vp, vp, sz, ctypes.POINTER(sz)], i32),
        "wq_records_stats": ([vp] + [ctypes.POINTER(ctypes.c_uint64)] * 3, i32),
        "wq_records_totals": ([vp, vp], i32),
        "wq_records_vacuum": ([vp, vp], i32),
        "wq_records_export": ([vp, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64)], i32),
        "wq_records_export_device": ([vp, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64)], i32),
        "wq_records_import": ([vp, vp, sz, ctypes.c_uint64, vp], i32),
        "wq_records_import_device": ([vp, vp, sz, ctypes.c_uint64, vp], i32),
        "wq_region_quantize": ([vp, sz, u16, vp], i32),
        "wq_table_quantize": ([vp, sz, u32, vp], i32),
        "wq_is_subscribed": ([vp, sz, vp, vp, i32, vp, vp], i32),
        "wq_is_subscribed_any": ([vp, sz, vp, vp, vp], i32),
        "wq_world_peers": ([vp, u32, vp, sz, ctypes.POINTER(sz)], i32),
        "wq_quantize": ([vp, sz, u16, vp], i32),
        "wq_quantize_device": ([vp, vp, sz, vp], i32),
        "wq_profile_enable": ([vp, i32], i32),
        "wq_profile_read": ([vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)], i32),
        "wq_profile_read_phases": ([vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64),
                                    ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)], i32),
        "wq_probe_sclk": ([vp, ctypes.POINTER(ctypes.c_double)], i32),
        "wq_debug_set_hash_bits": ([vp, i32], i32),
        "wq_debug_set_record_slack": ([vp, u32], i32),
        "wq_debug_set_route_config": ([vp, i32], i32),
        "wq_debug_set_route_chunks": ([vp, i32], i32),
        "wq_debug_route_config_count": ([], i32),
        "wq_debug_set_route_calls": ([vp, ctypes.c_uint64], i32),
        "wq_debug_route_calls": ([vp, ctypes.POINTER(ctypes.c_uint64)], i32),
        "wq_debug_set_timeline": ([vp, vp], i32),
        "wq_debug_update_counts": ([vp] + [ctypes.POINTER(ctypes.c_uint64)] * 3, i32),
        "wq_set_peer_positions": ([vp, vp, sz], i32),
        "wq_set_peer_positions_device": ([vp, vp, sz], i32),
        "wq_set_radius": ([vp, ctypes.c_double], i32),
        "wq_follow_set_reach": ([vp, u32], i32),
        "wq_follow_reset": ([vp], i32),
        "wq_follow_peers": ([vp, vp, vp, sz, ctypes.POINTER(FollowResult)], i32),
        "wq_follow_peers_device": ([vp, vp, vp, sz, ctypes.POINTER(FollowResult)], i32),
        "wq_follow_last_ops": ([vp, ctypes.POINTER(vp), ctypes.POINTER(sz)], i32),
        "wq_follow_read_ops": ([vp, vp, sz, ctypes.POINTER(sz)], i32),
        "wq_follow_state_read": ([vp, vp, vp, sz, ctypes.POINTER(sz)], i32),
        "wq_follow_state_load": ([vp, vp, vp, sz], i32),
        "wq_table_export": ([vp, ctypes.POINTER(abi.ExportFilter), vp, sz, ctypes.POINTER(sz)], i32),
        "wq_table_export_device": ([vp, ctypes.POINTER(abi.ExportFilter), vp, sz, ctypes.POINTER(sz)], i32),
        "wq_set_fanout_hint": ([vp, ctypes.c_double], i32),
        "wq_debug_route_shape": ([vp, ctypes.POINTER(i32), ctypes.POINTER(i32)], i32),
        "wq_route_health": ([vp, ctypes.POINTER(u32), ctypes.POINTER(u32)], i32),
        "wq_shard_ops": ([vp, vp, sz, u32, vp], i32),
        "wq_shard_messages_device": ([vp, vp, vp, vp, vp, vp, sz, u32, vp, vp], i32),
        "wq_route_records_device": ([vp, vp, sz, vp, vp, vp, sz, vp], i32),
        "wq_hub_create": ([u32, ctypes.POINTER(vp)], i32),
        "wq_hub_destroy": ([vp], i32),
        "wq_shard_attach_hub": ([vp, vp, u32], i32),
        "wq_rccl_unique_id": ([vp], i32),
        "wq_shard_attach_rccl": ([vp, u32, u32, vp], i32),
        "wq_shard_attach_exchange": ([vp, u32, u32, EXCHANGE_FN, vp], i32),
        "wq_shard_detach": ([vp], i32),
        "wq_shard_info": ([vp, ctypes.POINTER(u32), ctypes.POINTER(u32)], i32),
        "wq_sharded_apply_ops": ([vp, vp, sz], i32),
        "wq_sharded_route_tick_device": ([vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, ctypes.POINTER(sz)], i32),
        "wq_sharded_route_tick_async": ([vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp], i32),
        "wq_sharded_copy_out": ([vp, vp, vp, vp, sz], i32),
        "wq_sharded_route_owner_device": ([vp, vp, vp, vp, vp, vp, sz, ctypes.POINTER(abi.OwnerView)], i32),
        "wq_sharded_route_owner_slots": ([vp, vp, vp, vp, vp, vp, sz, ctypes.POINTER(abi.OwnerSlotView)], i32),
        "wq_sharded_route_owner_slots_async": ([vp, vp, vp, vp, vp, vp, sz, vp, ctypes.POINTER(abi.OwnerSlotView)],
                                               i32),
        "wq_shard_last_bytes": ([vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)], i32),
        "wq_debug_set_shard_form": ([vp, i32], i32),
        "wq_debug_inject_shard_failure": ([vp, i32], i32),
    }
    for name, (args, res) in sig.items():
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = res
    _lib = lib
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class PinnedArray:
    """A numpy array over pinned host memory (wq_host_alloc): DMA-able by the host-array ABI."""

    def __init__(self, shape, dtype):
        self.lib = load_library()
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = ctypes.c_void_p()
        rc = self.lib.wq_host_alloc(max(n, 1), ctypes.byref(p))
        if rc != 0:
            raise WQError(rc, "wq_host_alloc")
        self.ptr = p
        buf = (ctypes.c_uint8 * max(n, 1)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=np.uint8, count=n).view(dt).reshape(shape)

    def close(self):
        if self.ptr:
            self.array = None
            self.lib.wq_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WQStats(ctypes.Structure):
    _fields_ = [("n_entries", ctypes.c_uint64), ("n_cubes", ctypes.c_uint64), ("n_any", ctypes.c_uint64),
                ("table_slots", ctypes.c_uint64), ("hash_fallbacks", ctypes.c_uint64),
                ("cube_size", ctypes.c_uint32), ("device", ctypes.c_int32)]


def quantize(coords, cube_size: int) -> np.ndarray:
    """Kernel (1) on host arrays: CubeArea::coord_clamp per coordinate (cube_area.rs:23-44)."""
    lib = load_library()
    c = np.ascontiguousarray(coords, dtype=np.float64)
    out = np.empty(c.shape, dtype=np.int64)
    rc = lib.wq_quantize(_p(c), c.size, cube_size, _p(out))
    if rc != 0:
        raise WQError(rc, lib.wq_last_error(None).decode())
    return out


class Router:
    """One subscription table on one GPU (`WorldMap` of worldql_server/src/subscriptions/world_map.rs)."""

    def __init__(self, cube_size: int = 16, device: int = 0, hash_bits: int = 64):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.wq_router_create(cube_size, device, ctypes.byref(h))
        if rc != 0:
            raise WQError(rc, self.lib.wq_last_error(None).decode())
        self.h = h
        self.cube_size = cube_size
        self.device = device
        if hash_bits != 64:
            self._check(self.lib.wq_debug_set_hash_bits(self.h, hash_bits))

    @classmethod
    def multi(cls, cube_size: int = 16, devices=(0,), mode: str = "cube") -> "Router":
        """One handle over len(devices) GPUs (wq_router_create_multi_mode): the same API, the one-table
        result; mode "cube" = the table sharded by cube hash over the devices (they may repeat),
        "replicate" = every device holds the whole table and routes its own slice."""
        self = cls.__new__(cls)
        self.lib = load_library()
        devs = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        m = {"cube": abi.MULTI_CUBE_HASH, "replicate": abi.MULTI_REPLICATE}[mode]
        rc = self.lib.wq_router_create_multi_mode(cube_size, len(devices), devs, m, ctypes.byref(h))
        if rc != 0:
            raise WQError(rc, self.lib.wq_last_error(None).decode())
        self.h = h
        self.cube_size = cube_size
        self.device = devices[0]
        return self

    def n_gpus(self) -> int:
        n = ctypes.c_uint32()
        self._check(self.lib.wq_multi_info(self.h, ctypes.byref(n)))
        return n.value

    def multi_mode(self) -> int:
        m = ctypes.c_int()
        self._check(self.lib.wq_multi_mode(self.h, ctypes.byref(m)))
        return m.value

    def route_slices_device(self, slices, with_msgs: bool = False):
        """wq_route_tick_slices_device: slices = one (pos_ptr, world_ptr, sender_ptr, repl_ptr, n_msgs
        [, keys_ptr]) per device of the handle, on that device. Returns a list of abi.SliceView (device
        pointers into the handle's workspace, valid until its next route_slices_device call)."""
        G = len(slices)
        ins = (abi.MsgSlice * G)()
        for g, sl in enumerate(slices):
            pos, wo, se, rp, n = sl[:5]
            keys = sl[5] if len(sl) > 5 else None
            ins[g] = abi.MsgSlice(None if keys else (pos or None), keys or None, wo or None, se or None, rp or None, n)
        outs = (abi.SliceView * G)()
        self._check(self.lib.wq_route_tick_slices_device(self.h, ins, int(with_msgs), outs))
        return [outs[g] for g in range(G)]

    def shard_tick_stats(self):
        """(exact, budgeted) slot ticks run on this shard (wq_shard_tick_stats)."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.wq_shard_tick_stats(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def _check(self, rc: int):
        if rc != 0:
            raise WQError(rc, self.lib.wq_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.wq_router_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- table ----
    def apply_ops(self, ops: np.ndarray) -> None:
        ops = np.ascontiguousarray(ops, dtype=abi.OP_DTYPE)
        self._check(self.lib.wq_apply_ops(self.h, _p(ops), len(ops)))

    def apply_ops_device(self, ops_ptr: int, n: int) -> None:
        """A subscribe / unsubscribe batch already on the device (40-byte wq_op records)."""
        self._check(self.lib.wq_apply_ops_device(self.h, ops_ptr or None, n))

    def remove_peers(self, peers) -> None:
        a = np.ascontiguousarray(peers, dtype=np.uint32)
        self._check(self.lib.wq_remove_peers(self.h, _p(a), len(a)))

    def stats(self) -> dict:
        s = WQStats()
        self._check(self.lib.wq_get_stats(self.h, ctypes.byref(s)))
        return {f: getattr(s, f) for f, _ in WQStats._fields_}

    # ---- hot path ----
    def route(self, pos, world, sender, repl, keys=None, with_msgs: bool = False, capacity: int | None = None):
        """One tick on host arrays. Returns (offsets[M+1], peers[P], msgs[P] or None)."""
        world = np.ascontiguousarray(world, dtype=np.uint32)
        M = len(world)
        sender = np.ascontiguousarray(sender, dtype=np.uint32)
        repl = np.ascontiguousarray(repl, dtype=np.uint8)
        pos_a = None if pos is None else np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        keys_a = None if keys is None else np.ascontiguousarray(keys, dtype=np.int64).reshape(-1, 3)
        cap = capacity if capacity is not None else max(1024, 16 * M)
        while True:
            offsets = np.empty(M + 1, dtype=np.uint32)
            peers = np.empty(max(cap, 1), dtype=np.uint32)
            msgs = np.empty(max(cap, 1), dtype=np.uint32) if with_msgs else None
            n = ctypes.c_size_t()
            rc = self.lib.wq_route_tick(self.h, _p(pos_a), _p(keys_a), _p(world), _p(sender), _p(repl), M,
                                        _p(offsets), _p(peers), _p(msgs), cap, ctypes.byref(n))
            # (more pairs than the u32 offsets hold is WQ_E_CAPACITY too: no buffer cures it, raised below)
            if rc == abi.WQ_E_CAPACITY and cap < n.value <= abi.MAX_PAIRS and capacity is None:
                cap = n.value
                continue
            self._check(rc)
            P = n.value
            return offsets, peers[:P], (msgs[:P] if with_msgs else None)

    def route_device(self, pos_ptr: int, world_ptr: int, sender_ptr: int, repl_ptr: int, n_msgs: int,
                     offsets_ptr: int, peers_ptr: int, msgs_ptr: int | None, capacity: int,
                     counters_ptr: int | None = None, keys_ptr: int | None = None) -> None:
        """Asynchronous tick on device pointers (e.g. torch tensors' data_ptr())."""
        self._check(self.lib.wq_route_tick_device(self.h, pos_ptr or None, keys_ptr or None, world_ptr, sender_ptr,
                                                  repl_ptr, n_msgs, offsets_ptr, peers_ptr or None,
                                                  msgs_ptr or None, capacity, counters_ptr or None))

    def route_global(self, world, sender, repl, with_msgs: bool = False, capacity: int | None = None):
        """A tick of GlobalMessages to named worlds (global_message.rs:36-84) on host arrays.
        Returns (offsets[M+1], peers[P], msgs[P] or None); peers per message ascending."""
        world = np.ascontiguousarray(world, dtype=np.uint32)
        M = len(world)
        sender = np.ascontiguousarray(sender, dtype=np.uint32)
        repl = np.ascontiguousarray(repl, dtype=np.uint8)
        cap = capacity if capacity is not None else max(1024, 16 * M)
        while True:
            offsets = np.empty(M + 1, dtype=np.uint32)
            peers = np.empty(max(cap, 1), dtype=np.uint32)
            msgs = np.empty(max(cap, 1), dtype=np.uint32) if with_msgs else None
            n = ctypes.c_size_t()
            rc = self.lib.wq_route_global(self.h, _p(world), _p(sender), _p(repl), M, _p(offsets), _p(peers),
                                          _p(msgs), cap, ctypes.byref(n))
            # (more pairs than the u32 offsets hold is WQ_E_CAPACITY too: no buffer cures it, raised below)
            if rc == abi.WQ_E_CAPACITY and cap < n.value <= abi.MAX_PAIRS and capacity is None:
                cap = n.value
                continue
            self._check(rc)
            P = n.value
            return offsets, peers[:P], (msgs[:P] if with_msgs else None)

    def route_global_device(self, world_ptr: int, sender_ptr: int, repl_ptr: int, n_msgs: int, offsets_ptr: int,
                            peers_ptr: int | None, msgs_ptr: int | None, capacity: int,
                            counters_ptr: int | None = None) -> None:
        self._check(self.lib.wq_route_global_device(self.h, world_ptr, sender_ptr, repl_ptr, n_msgs, offsets_ptr,
                                                    peers_ptr or None, msgs_ptr or None, capacity,
                                                    counters_ptr or None))

    def peer_major_device(self, offsets_ptr: int, peers_ptr: int | None, n_msgs: int, n_pairs: int,
                          connected_ptr: int | None, n_peers: int, peer_offsets_ptr: int, msgs_out_ptr: int | None):
        """Per-peer send lists of a tick's CSR, disconnected peers dropped (peer_map.rs:151-163)."""
        self._check(self.lib.wq_peer_major_device(self.h, offsets_ptr or None, peers_ptr or None, n_msgs, n_pairs,
                                                  connected_ptr or None, n_peers, peer_offsets_ptr,
                                                  msgs_out_ptr or None))

    def tick_sends_device(self, regions, offsets_ptr: int | None, n_offsets: int, peers_ptr: int | None, n_pairs: int,
                          src_ptrs, n_src, connected_ptr: int | None, n_peers: int, n_frames: int,
                          peer_offsets_ptr: int, frames_out_ptr: int | None, n_elems: int,
                          counters_ptr: int | None = None) -> None:
        """wq_tick_sends_device: one per-peer list of frames, ascending, from all of a tick's CSR regions;
        asynchronous on the handle's stream. regions: abi.SEND_REGION_DTYPE rows on the host (free to reuse
        on return); src_ptrs / n_src: the two src arrays (l_src, g_src) and their lengths; n_elems: the sum
        of the regions' capacities. The counters (abi.TICK_SENDS_COUNTERS_DTYPE) stay where counters_ptr
        points. Host definition: interest.tick_sends_np."""
        reg = np.ascontiguousarray(regions, dtype=abi.SEND_REGION_DTYPE).reshape(-1)
        src = abi.TickSendsIn(regions=_p(reg) if len(reg) else None, d_offsets=offsets_ptr or None, n_offsets=n_offsets,
                              d_peers=peers_ptr or None, n_pairs=n_pairs,
                              d_src=(ctypes.c_void_p * 2)(src_ptrs[0] or None, src_ptrs[1] or None),
                              n_src=(ctypes.c_size_t * 2)(n_src[0], n_src[1]), d_connected=connected_ptr or None,
                              n_regions=len(reg), n_peers=n_peers, n_frames=n_frames)
        self._check(self.lib.wq_tick_sends_device(self.h, ctypes.byref(src), peer_offsets_ptr or None,
                                                  frames_out_ptr or None, n_elems, counters_ptr or None))

    def peer_budget_device(self, peer_offsets_ptr: int | None, msgs_ptr: int | None, n_peers: int, n_in: int,
                           msg_pos_ptr: int | None, n_msgs: int, peer_pos_ptr: int | None, n_peer_pos: int, k: int,
                           budget_ptr: int | None, out_offsets_ptr: int | None, out_msgs_ptr: int | None,
                           counters_ptr: int | None = None) -> None:
        """wq_peer_budget_device: of every row of a peer-major CSR the min(budget, len) messages nearest to
        the peer, in input order; asynchronous on the handle's stream. peer_pos_ptr None: the handle's
        set_peer_positions. The counters (abi.BUDGET_COUNTERS_DTYPE) stay where counters_ptr points.
        Host definition: interest.peer_budget_np."""
        self._check(self.lib.wq_peer_budget_device(self.h, peer_offsets_ptr or None, msgs_ptr or None, n_peers, n_in,
                                                   msg_pos_ptr or None, n_msgs, peer_pos_ptr or None, n_peer_pos, k,
                                                   budget_ptr or None, out_offsets_ptr or None, out_msgs_ptr or None,
                                                   counters_ptr or None))

    def peer_budget_bytes_device(self, peer_offsets_ptr: int | None, msgs_ptr: int | None, n_peers: int, n_in: int,
                                 msg_pos_ptr: int | None, msg_size_ptr: int | None, n_msgs: int,
                                 peer_pos_ptr: int | None, n_peer_pos: int, w: int, budget_bytes_ptr: int | None,
                                 out_offsets_ptr: int | None, out_msgs_ptr: int | None,
                                 out_bytes_ptr: int | None = None, counters_ptr: int | None = None) -> None:
        """wq_peer_budget_bytes_device: of every row of a peer-major CSR the nearest messages whose sizes
        (msg_size_ptr: u32 per message) sum to at most the peer's byte budget (budget_bytes_ptr: u64 per
        peer, else w for everyone), in input order; asynchronous on the handle's stream. out_bytes_ptr
        (u64 per peer, optional) receives every row's kept bytes; the counters
        (abi.BUDGET_BYTES_COUNTERS_DTYPE) stay where counters_ptr points. Host definition:
        interest.peer_budget_bytes_np."""
        self._check(self.lib.wq_peer_budget_bytes_device(
            self.h, peer_offsets_ptr or None, msgs_ptr or None, n_peers, n_in, msg_pos_ptr or None, msg_size_ptr or None,
            n_msgs, peer_pos_ptr or None, n_peer_pos, w, budget_bytes_ptr or None, out_offsets_ptr or None,
            out_msgs_ptr or None, out_bytes_ptr or None, counters_ptr or None))

    def peer_rotate_device(self, peer_offsets_ptr: int | None, msgs_ptr: int | None, n_peers: int, n_in: int,
                           kept_offsets_ptr: int | None, kept_msgs_ptr: int | None, n_kept_in: int,
                           msg_size_ptr: int | None, n_msgs: int, r: int, extra_ptr: int | None, v: int,
                           extra_bytes_ptr: int | None, cursor_ptr: int | None, out_offsets_ptr: int | None,
                           out_msgs_ptr: int | None, out_bytes_ptr: int | None = None,
                           counters_ptr: int | None = None) -> None:
        """wq_peer_rotate_device: the fair share. Of every row of the full peer-major CSR the elements
        the kept CSR (either budget's output on it) holds, plus the cut elements that follow the peer's
        cursor (cursor_ptr: u32 per peer, a message index, updated in place) in cyclic order of message
        index: at most extra_ptr[p] of them (u32 per peer, else r for everyone) and, with msg_size_ptr
        (u32 per message), at most extra_bytes_ptr[p] bytes (u64 per peer, else v), the first always;
        asynchronous on the handle's stream. out_bytes_ptr (u64 per peer, optional, needs msg_size_ptr)
        receives every output row's bytes; the counters (abi.ROTATE_COUNTERS_DTYPE) stay where
        counters_ptr points. Host definition: interest.peer_rotate_np."""
        self._check(self.lib.wq_peer_rotate_device(
            self.h, peer_offsets_ptr or None, msgs_ptr or None, n_peers, n_in, kept_offsets_ptr or None,
            kept_msgs_ptr or None, n_kept_in, msg_size_ptr or None, n_msgs, r, extra_ptr or None, v,
            extra_bytes_ptr or None, cursor_ptr or None, out_offsets_ptr or None, out_msgs_ptr or None,
            out_bytes_ptr or None, counters_ptr or None))

    def peer_pack_device(self, peer_offsets_ptr: int | None, msgs_ptr: int | None, n_peers: int, n_in: int,
                         frames_ptr: int | None, frame_offsets_ptr: int | None, n_msgs: int, n_frame_bytes: int,
                         flags: int, out_ptr: int | None, capacity_bytes: int, out_peer_bytes_ptr: int | None,
                         out_elem_bytes_ptr: int | None = None, counters_ptr: int | None = None) -> None:
        """wq_peer_pack_device: for every row of a peer-major CSR the frames of its messages
        (frames_ptr[frame_offsets[m] .. frame_offsets[m + 1]), u64 offsets) in one contiguous byte run
        of out_ptr, in list order, each behind its u32 size with flags = abi.PACK_LEN_PREFIX;
        asynchronous on the handle's stream. out_peer_bytes_ptr (u64[n_peers + 1]) receives where every
        peer's run starts, out_elem_bytes_ptr (u64[n_in], optional) where every record starts; the
        counters (abi.PACK_COUNTERS_DTYPE) stay where counters_ptr points. out_ptr None with capacity 0
        sizes the buffer. Host definition: interest.peer_pack_np."""
        self._check(self.lib.wq_peer_pack_device(
            self.h, peer_offsets_ptr or None, msgs_ptr or None, n_peers, n_in, frames_ptr or None,
            frame_offsets_ptr or None, n_msgs, n_frame_bytes, flags, out_ptr or None, capacity_bytes,
            out_peer_bytes_ptr or None, out_elem_bytes_ptr or None, counters_ptr or None))

    # ---- frame builder (include/wq_router.h; host definition: frames.py) ----
    def set_worlds(self, names) -> None:
        """wq_frames_set_worlds: the handle's table world id -> name (a list of str or bytes; empty
        clears it) for build_frames_device. The table is copied; the call waits for the handle's stream."""
        from .frames import world_table
        raw, off = world_table(names)
        buf = ctypes.create_string_buffer(raw, max(len(raw), 1))
        self._check(self.lib.wq_frames_set_worlds(self.h, ctypes.addressof(buf), off.ctypes.data, len(off) - 1))

    def build_frames_device(self, src: "abi.FramesSrc", n_msgs: int, frames_ptr: int | None, capacity_bytes: int,
                            frame_offsets_ptr: int | None, frame_size_ptr: int | None = None,
                            counters_ptr: int | None = None) -> None:
        """wq_frames_build_device: the frames of n_msgs flat messages (src: abi.FramesSrc of device
        pointers, worlds as ids into set_worlds' table) written to frames_ptr exactly as
        codec.serialize_messages writes them, their u64 offsets[n_msgs + 1] to frame_offsets_ptr and
        their u32 sizes to frame_size_ptr (optional): the three arrays peer_budget_bytes_device and
        peer_pack_device take. Asynchronous on the handle's stream; the counters
        (abi.FRAMES_COUNTERS_DTYPE) stay where counters_ptr points. frames_ptr None with capacity 0
        sizes the buffer. Host definition: frames.build_frames_np."""
        self._check(self.lib.wq_frames_build_device(self.h, ctypes.byref(src), n_msgs, frames_ptr or None,
                                                    capacity_bytes, frame_offsets_ptr or None, frame_size_ptr or None,
                                                    counters_ptr or None))

    # ---- ingest: received frames decoded on the device (include/wq_router.h; host definition: ingest.py) ----
    def set_ingest_peers(self, uuids, ids=None) -> None:
        """wq_ingest_set_peers: the handle's table sender uuid -> peer id (uuids: n x 16 bytes, a list of
        uuid.UUID or of 16-byte strings; ids: u32 per uuid, None: the index; empty clears it). A uuid that
        occurs twice raises WQError (WQ_E_INVALID) and the old table stays. The table is copied; the call
        waits for the handle's stream."""
        from .ingest import uuid_rows
        u = uuid_rows(uuids)
        i = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
        if i is not None and len(i) != len(u):
            raise ValueError("ids: one per uuid")
        self._check(self.lib.wq_ingest_set_peers(self.h, u.ctypes.data if len(u) else None,
                                                 i.ctypes.data if i is not None and len(i) else None, len(u)))

    def decode_frames_device(self, frames_ptr: int | None, frame_offsets_ptr: int | None, n_frames: int,
                             n_frame_bytes: int, out: "abi.IngestOut", counters_ptr: int | None = None) -> None:
        """wq_frames_decode_device: n_frames received frames (frames_ptr[fo[i] .. fo[i + 1]), u64
        offsets) verified and decoded as codec.decode_packed does, with world ids (set_worlds' table) and
        peer ids (set_ingest_peers' table) resolved, into the device arrays of `out` (abi.IngestOut, each
        nullable): pos / world / sender / repl are route_device's inputs. Asynchronous on the handle's
        stream; the counters (abi.INGEST_COUNTERS_DTYPE) stay where counters_ptr points. Host definition:
        ingest.decode_frames_np."""
        self._check(self.lib.wq_frames_decode_device(self.h, frames_ptr or None, frame_offsets_ptr or None, n_frames,
                                                     n_frame_bytes, ctypes.byref(out) if out is not None else None,
                                                     counters_ptr or None))

    def dispatch_device(self, src: "abi.DispatchIn", n_frames: int, out: "abi.DispatchOut",
                        counters_ptr: int | None = None) -> None:
        """wq_ingest_dispatch_device: the decode's arrays (abi.DispatchIn: instruction, flags, world, sender,
        repl, pos; last_seen / n_last_seen / now for the heartbeat stamps) split by instruction into the
        device arrays of `out` (abi.DispatchOut, each nullable): the rows of route_device (l_*),
        route_global_device (g_*) and apply_ops_device (ops), the side lists, and the run table that says
        in which order to issue them. Asynchronous on the handle's stream; the counters
        (abi.DISPATCH_COUNTERS_DTYPE) stay where counters_ptr points. Host definition: ingest.dispatch_np."""
        self._check(self.lib.wq_ingest_dispatch_device(self.h, ctypes.byref(src) if src is not None else None, n_frames,
                                                       ctypes.byref(out) if out is not None else None,
                                                       counters_ptr or None))

    # ---- ingest joins (include/wq_router.h, "ingest joins"; host definition: ingest.join_peers_np) ----
    def reserve_peers(self, capacity: int) -> None:
        """wq_ingest_peers_reserve: room for `capacity` entries in the sender table, whose live count becomes
        a device word (join_peers_device and drop_peers_device change it, the decode reads it). Existing
        entries are kept; set_ingest_peers keeps working. Waits for the handle's stream."""
        self._check(self.lib.wq_ingest_peers_reserve(self.h, capacity))

    def join_peers_device(self, src: "abi.JoinIn", n_frames: int, out: "abi.JoinOut",
                          counters_ptr: int | None = None) -> None:
        """wq_ingest_join_device: between decode_frames_device and dispatch_device. The subscribes of
        senders the table lacks (abi.JoinIn: the decode's instruction, world, sender_uuid, and flags /
        sender, which are patched in place; the allocator state free_ids / n_free / id_next / id_limit) get
        their ids, the joins are listed in `out` (abi.JoinOut, each nullable) and merged into the handle's
        sender table. All or nothing on overflow. Asynchronous on the handle's stream; the counters
        (abi.JOIN_COUNTERS_DTYPE) stay where counters_ptr points. Host definition: ingest.join_peers_np."""
        self._check(self.lib.wq_ingest_join_device(self.h, ctypes.byref(src) if src is not None else None, n_frames,
                                                   ctypes.byref(out) if out is not None else None, counters_ptr or None))

    def drop_peers_device(self, ids_ptr: int | None, n: int, counters_ptr: int | None = None) -> None:
        """wq_ingest_drop_peers_device: every sender-table entry whose id is among the n device u32 at ids_ptr
        is removed (absent ids and duplicates are ignored). Asynchronous on the handle's stream. Host
        definition: ingest.drop_peers_np."""
        self._check(self.lib.wq_ingest_drop_peers_device(self.h, ids_ptr or None, n, counters_ptr or None))

    def read_peers(self):
        """wq_ingest_peers_read: the live sender table as (uuids u8[n, 16] ascending, ids u32[n]). Waits for
        the handle's stream."""
        n = ctypes.c_size_t(0)
        self._check(self.lib.wq_ingest_peers_read(self.h, None, None, 0, ctypes.byref(n)))
        u, i = np.zeros((n.value, 16), np.uint8), np.zeros(n.value, np.uint32)
        if n.value:
            self._check(self.lib.wq_ingest_peers_read(self.h, u.ctypes.data, i.ctypes.data, n.value, ctypes.byref(n)))
        return u, i

    # ---- ingest leaves (include/wq_router.h, "ingest leaves"; host definition: ingest.leave_peers_np) ----
    def leave_peers_device(self, src: "abi.LeaveIn", out: "abi.LeaveOut", counters_ptr: int | None = None) -> None:
        """wq_ingest_leave_device: the sweep. Every live sender-table entry whose id is listed in
        src.leave_ids or whose stamp in src.last_seen is stale (now - stamp > max_age, strict; never a pinned
        id, a stamp ahead or abi.SEEN_NEVER) leaves: `out` (abi.LeaveOut, each nullable) takes the leavers in
        uuid order with their uuid text as build_frames_device's param / param_offsets, the bitmap
        remove_peers_device takes and the new free list; the stamps of the leavers are reset, the clocks of
        new entries start, and the table is compacted. All or nothing on overflow. Asynchronous on the
        handle's stream; the counters (abi.LEAVE_COUNTERS_DTYPE) stay where counters_ptr points."""
        self._check(self.lib.wq_ingest_leave_device(self.h, ctypes.byref(src) if src is not None else None,
                                                    ctypes.byref(out) if out is not None else None, counters_ptr or None))

    def remove_peers_device(self, bits_ptr: int | None, n_ids: int, count_ptr: int | None = None) -> None:
        """wq_remove_peers_device: remove_peers for the ids < n_ids whose bit is set in the device bitmap at
        bits_ptr (u32 words), with nothing built, uploaded or waited for on the host. count_ptr: a device u64
        (the leave's n_left); when it holds 0 the kernel returns before it touches the table. Invalidates what
        remove_peers invalidates whether or not a bit is set: a call for the sweep interval, not every tick.
        Single-GPU handles only."""
        self._check(self.lib.wq_remove_peers_device(self.h, bits_ptr or None, n_ids, count_ptr or None))

    def records_dispatch_device(self, src: "abi.RecDispatchIn", out: "abi.RecDispatchOut",
                                counters_ptr: int | None = None) -> None:
        """wq_records_dispatch_device: the record frames of a decoded tick (abi.RecDispatchIn: the raw frames,
        the decode's msg / world / flags, the dispatch's database list, the handle allocator) walked record
        by record into the device arrays of `out` (abi.RecDispatchOut, each nullable): the ops of
        GpuRecordStore.apply_device with their payload references, the query rows of read_device, the
        deferred list and the run table. Needs an open record store (its region sizes decide what is
        packable). Asynchronous on the handle's stream; the counters (abi.RECDISP_COUNTERS_DTYPE) stay
        where counters_ptr points. Host definition: ingest.records_dispatch_np."""
        self._check(self.lib.wq_records_dispatch_device(self.h, ctypes.byref(src) if src is not None else None,
                                                        ctypes.byref(out) if out is not None else None,
                                                        counters_ptr or None))

    def build_record_frames_device(self, src: "abi.FramesSrc", rec: "abi.FramesRecSrc", n_msgs: int, frames_ptr: int | None,
                                   capacity_bytes: int, frame_offsets_ptr: int, frame_size_ptr: int | None = None,
                                   counters_ptr: int | None = None) -> None:
        """wq_frames_build_records_device: build_frames_device for messages that carry records. rec
        (abi.FramesRecSrc) holds a CSR of slab handles (row_offsets u32[n_msgs + 1], handles), the slab
        (abi.SlabView, read only), optional per-message world names as bytes and the flags
        (abi.FRAMES_SKIP_EMPTY). Output, capacity, sizing call and counters as build_frames_device. Asynchronous
        on the handle's stream. Host definition: frames.build_record_frames_np."""
        self._check(self.lib.wq_frames_build_records_device(self.h, ctypes.byref(src), ctypes.byref(rec), n_msgs,
                                                            frames_ptr or None, capacity_bytes, frame_offsets_ptr,
                                                            frame_size_ptr or None, counters_ptr or None))

    def slab_store_device(self, ops_ptr: int | None, op_ref_ptr: int | None, n_ops: int, frames_ptr: int | None,
                          frame_offsets_ptr: int | None, n_frames: int, view: "abi.SlabView", cursor_ptr: int,
                          counters_ptr: int | None = None) -> None:
        """wq_slab_store_device: the payloads of the creates among n_ops ops (wq_rec_op / wq_rec_op_ref as
        records_dispatch_device wrote them) copied from the tick's frames into the caller's slab (abi.SlabView:
        entries indexed by handle and a byte arena, device memory), placed from the device word at cursor_ptr,
        which the call advances. All or nothing: an arena or entry array that is too small leaves slab and
        cursor as they were and says so in the counters (abi.SLAB_COUNTERS_DTYPE, where counters_ptr points).
        Asynchronous on the handle's stream; nothing is read back. Host definition: records.slab_store_np."""
        self._check(self.lib.wq_slab_store_device(self.h, ops_ptr or None, op_ref_ptr or None, n_ops, frames_ptr or None,
                                                  frame_offsets_ptr or None, n_frames,
                                                  ctypes.byref(view) if view is not None else None, cursor_ptr or None,
                                                  counters_ptr or None))

    def slab_compact_device(self, src: "abi.SlabView", dst: "abi.SlabView", dst_cursor_ptr: int,
                            counters_ptr: int | None = None) -> None:
        """wq_slab_compact_device: the slab `src` rewritten into `dst` (both abi.SlabView, device memory that
        does not overlap) in its canonical form: live payloads back to back in handle order, every other
        entry zero, the total in the device word at dst_cursor_ptr. All or nothing: a dst that is too small
        is left as it was and the counters (abi.SLAB_COMPACT_COUNTERS_DTYPE, where counters_ptr points) say
        what suffices. Asynchronous on the handle's stream; nothing is read back. Host definition:
        records.slab_compact_np."""
        self._check(self.lib.wq_slab_compact_device(self.h, ctypes.byref(src) if src is not None else None,
                                                    ctypes.byref(dst) if dst is not None else None, dst_cursor_ptr or None,
                                                    counters_ptr or None))

    def set_ingest_list(self, entries: int) -> None:
        """wq_debug_set_ingest_list: a test hook, the long-string work list's capacity (0: none; negative:
        the default). Results are identical for every value."""
        self._check(self.lib.wq_debug_set_ingest_list(self.h, entries))

    # ---- interest changes between two ticks (include/wq_router.h; host reference: interest.py) ----
    def csr_diff(self, old_offsets, old_peers, new_offsets, new_peers, with_left: bool = True,
                 ent_capacity: int | None = None, left_capacity: int | None = None):
        """wq_csr_diff on host arrays: (ent_offsets, ent_peers, left_offsets, left_peers, n_entered,
        n_left); the left arrays are None and n_left 0 with with_left=False. Without a capacity the
        outputs are sized to hold any result; with one, a result that does not fit raises WQError
        (WQ_E_CAPACITY) whose .sizes holds (n_entered, n_left) and .offsets the two offset arrays."""
        oo = np.ascontiguousarray(old_offsets, dtype=np.uint32)
        no = np.ascontiguousarray(new_offsets, dtype=np.uint32)
        op = np.ascontiguousarray(old_peers, dtype=np.uint32)
        npr = np.ascontiguousarray(new_peers, dtype=np.uint32)
        if len(oo) != len(no) or len(oo) < 1:
            raise ValueError("both CSRs need offsets[n_rows + 1] over the same rows")
        M = len(oo) - 1
        ce = len(npr) if ent_capacity is None else ent_capacity
        cl = (len(op) if left_capacity is None else left_capacity) if with_left else 0
        eo = np.empty(M + 1, dtype=np.uint32)
        ep = np.empty(max(ce, 1), dtype=np.uint32)
        lo = np.empty(M + 1, dtype=np.uint32) if with_left else None
        lp = np.empty(max(cl, 1), dtype=np.uint32) if with_left else None
        ne, nl = ctypes.c_size_t(), ctypes.c_size_t()
        rc = self.lib.wq_csr_diff(self.h, M, _p(oo), _p(op) if len(op) else None, len(op), _p(no),
                                  _p(npr) if len(npr) else None, len(npr), _p(eo), _p(ep) if ce else None, ce,
                                  _p(lo), _p(lp) if cl else None, cl, ctypes.byref(ne), ctypes.byref(nl))
        if rc == abi.WQ_E_CAPACITY:
            err = WQError(rc, self.lib.wq_last_error(self.h).decode())
            err.sizes = (ne.value, nl.value)
            err.offsets = (eo, lo)
            raise err
        self._check(rc)
        return eo, ep[: ne.value], lo, (lp[: nl.value] if with_left else None), ne.value, nl.value

    def csr_diff_device(self, n_rows: int, old_offsets_ptr: int, old_peers_ptr: int | None, old_capacity: int,
                        new_offsets_ptr: int, new_peers_ptr: int | None, new_capacity: int, ent_offsets_ptr: int,
                        ent_peers_ptr: int | None, ent_capacity: int, left_offsets_ptr: int | None = None,
                        left_peers_ptr: int | None = None, left_capacity: int = 0,
                        counters_ptr: int | None = None) -> None:
        """wq_csr_diff_device: asynchronous on the handle's stream; the counters (abi.DIFF_COUNTERS_DTYPE)
        stay where counters_ptr points."""
        self._check(self.lib.wq_csr_diff_device(self.h, n_rows, old_offsets_ptr or None, old_peers_ptr or None,
                                                old_capacity, new_offsets_ptr or None, new_peers_ptr or None,
                                                new_capacity, ent_offsets_ptr or None, ent_peers_ptr or None,
                                                ent_capacity, left_offsets_ptr or None, left_peers_ptr or None,
                                                left_capacity, counters_ptr or None))

    # ---- multi-GPU (cube-hash ownership: wq_shard.hip, wq_sharded*.hip) ----
    def shard_ops(self, ops: np.ndarray, n_shards: int) -> np.ndarray:
        """Owner shard of each op (abi.SHARD_ALL for REMOVE_PEER)."""
        ops = np.ascontiguousarray(ops, dtype=abi.OP_DTYPE)
        out = np.empty(len(ops), dtype=np.uint32)
        self._check(self.lib.wq_shard_ops(self.h, _p(ops), len(ops), n_shards, _p(out)))
        return out

    def shard_messages_device(self, pos_ptr: int | None, keys_ptr: int | None, world_ptr: int, sender_ptr: int,
                              repl_ptr: int, n_msgs: int, n_shards: int, recs_ptr: int, counts_ptr: int) -> None:
        """Group a tick's messages by owner shard into 40-byte records (asynchronous)."""
        self._check(self.lib.wq_shard_messages_device(self.h, pos_ptr or None, keys_ptr or None, world_ptr or None,
                                                      sender_ptr or None, repl_ptr or None, n_msgs, n_shards,
                                                      recs_ptr or None, counts_ptr))

    def route_records_device(self, recs_ptr: int | None, n_msgs: int, offsets_ptr: int, peers_ptr: int | None,
                             msgs_ptr: int | None, capacity: int, counters_ptr: int | None = None) -> None:
        """Route received records on this shard (asynchronous)."""
        self._check(self.lib.wq_route_records_device(self.h, recs_ptr or None, n_msgs, offsets_ptr,
                                                     peers_ptr or None, msgs_ptr or None, capacity,
                                                     counters_ptr or None))

    # ---- multi-GPU behind the ABI: this handle as one shard of G (include/wq_router.h) ----
    def attach_hub(self, hub: "Hub", rank: int) -> None:
        self._check(self.lib.wq_shard_attach_hub(self.h, hub.h, rank))
        self._hub = hub  # keep it alive while attached

    def attach_rccl(self, n_shards: int, rank: int, uid: bytes) -> None:
        assert len(uid) == abi.RCCL_ID_BYTES
        buf = ctypes.create_string_buffer(bytes(uid), abi.RCCL_ID_BYTES)
        self._check(self.lib.wq_shard_attach_rccl(self.h, n_shards, rank, buf))

    def attach_exchange(self, n_shards: int, rank: int, fn) -> None:
        """fn(d_send, send_bytes[G], d_recv, recv_bytes[G], stream) -> None: the caller's all-to-all
        (device pointers as ints, byte counts as lists). Exceptions count as failures."""
        G = n_shards

        def tramp(_ctx, send, sb, recv, rb, stream):
            try:
                fn(send or 0, [sb[i] for i in range(G)], recv or 0, [rb[i] for i in range(G)], stream or 0)
                return 0
            except Exception:  # noqa: BLE001 — reported through the C status
                import traceback
                traceback.print_exc()
                return 1
        self._xfn = EXCHANGE_FN(tramp)  # keep the trampoline alive
        self._check(self.lib.wq_shard_attach_exchange(self.h, n_shards, rank, self._xfn, None))

    def detach_shard(self) -> None:
        self._check(self.lib.wq_shard_detach(self.h))

    def shard_info(self):
        g, r = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.wq_shard_info(self.h, ctypes.byref(g), ctypes.byref(r)))
        return g.value, r.value

    def sharded_apply_ops(self, ops: np.ndarray) -> None:
        """The tick's whole op stream (every shard gets the same); this shard keeps what it owns."""
        ops = np.ascontiguousarray(ops, dtype=abi.OP_DTYPE)
        self._check(self.lib.wq_sharded_apply_ops(self.h, _p(ops), len(ops)))

    def sharded_route_device(self, pos_ptr, world_ptr, sender_ptr, repl_ptr, n_msgs, offsets_ptr, peers_ptr,
                             msgs_ptr, capacity, keys_ptr=None):
        """One collective sharded tick on this shard's ingested messages (device pointers).
        Returns (rc, P): rc is WQ_OK or WQ_E_CAPACITY (then sharded_copy_out with room for P)."""
        n = ctypes.c_size_t()
        rc = self.lib.wq_sharded_route_tick_device(self.h, pos_ptr or None, keys_ptr or None, world_ptr or None,
                                                   sender_ptr or None, repl_ptr or None, n_msgs, offsets_ptr,
                                                   peers_ptr or None, msgs_ptr or None, capacity, ctypes.byref(n))
        if rc not in (0, abi.WQ_E_CAPACITY):
            self._check(rc)
        return rc, n.value

    def sharded_route_async(self, pos_ptr, world_ptr, sender_ptr, repl_ptr, n_msgs, offsets_ptr, peers_ptr,
                            msgs_ptr, capacity, counters_ptr=None, keys_ptr=None) -> None:
        """wq_sharded_route_tick_async: the collective tick without its end-of-tick read; P and the
        status bits (64: a budget was too small, route the tick again) land in counters_ptr."""
        self._check(self.lib.wq_sharded_route_tick_async(self.h, pos_ptr or None, keys_ptr or None, world_ptr or None,
                                                         sender_ptr or None, repl_ptr or None, n_msgs, offsets_ptr,
                                                         peers_ptr or None, msgs_ptr or None, capacity,
                                                         counters_ptr or None))

    def sharded_route_owner_device(self, pos_ptr, world_ptr, sender_ptr, repl_ptr, n_msgs, keys_ptr=None):
        """The owner-side form of the collective sharded tick: the pairs stay on the shard that routed
        them. Returns an abi.OwnerView of device pointers valid until the next sharded call."""
        v = abi.OwnerView()
        self._check(self.lib.wq_sharded_route_owner_device(self.h, pos_ptr or None, keys_ptr or None, world_ptr or None,
                                                           sender_ptr or None, repl_ptr or None, n_msgs,
                                                           ctypes.byref(v)))
        return v

    def sharded_route_owner_slots(self, pos_ptr, world_ptr, sender_ptr, repl_ptr, n_msgs, keys_ptr=None):
        """wq_sharded_route_owner_slots: the owner form on budgeted 20-byte slots (one exchange per
        tick; the pairs stay on the owner). Returns an abi.OwnerSlotView of device pointers valid
        until the next sharded call."""
        v = abi.OwnerSlotView()
        self._check(self.lib.wq_sharded_route_owner_slots(self.h, pos_ptr or None, keys_ptr or None, world_ptr or None,
                                                          sender_ptr or None, repl_ptr or None, n_msgs,
                                                          ctypes.byref(v)))
        return v

    def sharded_route_owner_slots_async(self, pos_ptr, world_ptr, sender_ptr, repl_ptr, n_msgs, counters_ptr=None,
                                        keys_ptr=None):
        """wq_sharded_route_owner_slots_async: the owner-slot tick without its end-of-tick read; P and the
        status bits land in counters_ptr (view.n_pairs is 2^64-1 when the tick ran asynchronously)."""
        v = abi.OwnerSlotView()
        self._check(self.lib.wq_sharded_route_owner_slots_async(self.h, pos_ptr or None, keys_ptr or None,
                                                                world_ptr or None, sender_ptr or None, repl_ptr or None,
                                                                n_msgs, counters_ptr or None, ctypes.byref(v)))
        return v

    def sharded_copy_out(self, offsets_ptr, peers_ptr, msgs_ptr, capacity) -> None:
        self._check(self.lib.wq_sharded_copy_out(self.h, offsets_ptr, peers_ptr or None, msgs_ptr or None, capacity))

    def shard_last_bytes(self):
        """(bytes sent to, bytes received from) OTHER shards in this shard's latest sharded tick."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.wq_shard_last_bytes(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def inject_shard_failure(self, step: int) -> None:
        """Test hook: the next sharded tick fails locally at step 1 or 3 (wq_debug_inject_shard_failure)."""
        self._check(self.lib.wq_debug_inject_shard_failure(self.h, step))

    def set_shard_form(self, expanded: bool) -> None:
        """True: the sharded tick returns expanded (message, peer) pairs (the radius filter's form);
        False (default): row references + one pool of cube lists per destination."""
        self._check(self.lib.wq_debug_set_shard_form(self.h, int(expanded)))

    # ---- C5 radius filter (include/wq_router.h) ----
    def set_peer_positions(self, pos) -> None:
        p = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        self._check(self.lib.wq_set_peer_positions(self.h, _p(p), len(p)))

    def set_peer_positions_device(self, pos_ptr: int, n_peers: int) -> None:
        self._check(self.lib.wq_set_peer_positions_device(self.h, pos_ptr or None, n_peers))

    def set_radius(self, radius: float) -> None:
        self._check(self.lib.wq_set_radius(self.h, float(radius)))

    # ---- follow moving peers (include/wq_router.h; host reference: follow.py) ----
    def follow_set_reach(self, reach: int) -> None:
        """Reach of the followed neighbourhood, 0..2 (default 1); only while no peer is followed."""
        self._check(self.lib.wq_follow_set_reach(self.h, reach))

    def follow_reset(self) -> None:
        """Drops all follow state; no op is emitted."""
        self._check(self.lib.wq_follow_reset(self.h))

    def follow_peers(self, world, pos) -> dict:
        """world[n], pos[n x 3] indexed by peer id (abi.WORLD_INVALID: stop following): the table
        follows the moves. Returns {n_unsubscribe, n_subscribe, n_followed}."""
        w = np.ascontiguousarray(world, dtype=np.uint32)
        p = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        if len(p) != len(w):
            raise ValueError("world and pos must cover the same peers")
        res = FollowResult()
        self._check(self.lib.wq_follow_peers(self.h, _p(w), _p(p), len(w), ctypes.byref(res)))
        return {f: getattr(res, f) for f, _ in FollowResult._fields_}

    def follow_peers_device(self, world_ptr: int, pos_ptr: int, n: int) -> dict:
        """The same on device arrays, read on the handle's stream; asynchronous after the read-back
        of the op totals (keep the arrays unchanged until the stream has passed the call)."""
        res = FollowResult()
        self._check(self.lib.wq_follow_peers_device(self.h, world_ptr or None, pos_ptr or None, n, ctypes.byref(res)))
        return {f: getattr(res, f) for f, _ in FollowResult._fields_}

    def follow_last_ops_device(self):
        """(device pointer or 0, n) of the latest follow call's ops (wq_follow_last_ops)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self.lib.wq_follow_last_ops(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p.value or 0, n.value

    def follow_last_ops(self) -> np.ndarray:
        """The latest follow call's ops, copied to the host (abi.OP_DTYPE, stream order)."""
        _, n = self.follow_last_ops_device()
        out = np.zeros(n, dtype=abi.OP_DTYPE)
        got = ctypes.c_size_t()
        self._check(self.lib.wq_follow_read_ops(self.h, _p(out) if n else None, n, ctypes.byref(got)))
        return out[: got.value]

    def follow_state(self):
        """(world[n], pos[n x 3]) of the peers the follow state covers (wq_follow_state_read); a peer
        that is not followed reads abi.WORLD_INVALID and zeros."""
        n = ctypes.c_size_t()
        rc = self.lib.wq_follow_state_read(self.h, None, None, 0, ctypes.byref(n))
        if rc not in (0, abi.WQ_E_CAPACITY):
            self._check(rc)
        w = np.zeros(n.value, np.uint32)
        p = np.zeros((n.value, 3), np.float64)
        if n.value:
            self._check(self.lib.wq_follow_state_read(self.h, _p(w), _p(p), n.value, ctypes.byref(n)))
        return w, p

    def follow_state_load(self, world, pos) -> None:
        """Installs a follow state (wq_follow_state_load): no op is emitted; only while no peer is
        followed. Set the reach first."""
        w = np.ascontiguousarray(world, dtype=np.uint32)
        p = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        if len(p) != len(w):
            raise ValueError("world and pos must cover the same peers")
        self._check(self.lib.wq_follow_state_load(self.h, _p(w), _p(p), len(w)))

    # ---- table snapshots (include/wq_router.h; host definition: snapshot.py) ----
    @staticmethod
    def _export_filter(world, peers):
        """(ctypes pointer or None, the array it points into)."""
        if world is None and peers is None:
            return None, None
        ids = None if peers is None else np.ascontiguousarray(peers, dtype=np.uint32).reshape(-1)
        if ids is not None and len(ids) == 0:
            ids = np.zeros(1, np.uint32)[:0]
        f = abi.ExportFilter(abi.WORLD_INVALID if world is None else int(world), 0 if ids is None else len(ids), None)
        if ids is not None:  # (a zero-length list still needs a non-null pointer: null = every peer)
            f.peers = ids.ctypes.data
        return ctypes.pointer(f), (ids, f)

    def export_table(self, world=None, peers=None, capacity: int | None = None, out=None) -> np.ndarray:
        """Every live (world, cube, peer) as one SUBSCRIBE op with a raw key, in canonical order
        (wq_table_export): `world` None = every world, `peers` None = every peer. With `capacity`
        only that many rows are asked for: the call then raises WQError(WQ_E_CAPACITY) when the
        table holds more. `out` (abi.OP_DTYPE, e.g. a PinnedArray's array) receives the rows."""
        fp, keep = self._export_filter(world, peers)
        n = ctypes.c_size_t()
        if capacity is None and out is None:
            rc = self.lib.wq_table_export(self.h, fp, None, 0, ctypes.byref(n))
            if rc not in (0, abi.WQ_E_CAPACITY):
                self._check(rc)
            capacity = n.value
        if out is None:
            out = np.zeros(capacity, dtype=abi.OP_DTYPE)
        elif capacity is None:
            capacity = len(out)
        self._check(self.lib.wq_table_export(self.h, fp, _p(out) if capacity else None, capacity, ctypes.byref(n)))
        del keep
        return out[: n.value]

    def export_table_device(self, ptr: int, capacity: int, world=None, peers=None):
        """The same into device memory on the handle's device (wq_table_export_device). Returns
        (rc, n): n is the full row count, rc WQ_E_CAPACITY when it exceeds `capacity` (the first
        `capacity` rows are written); other errors raise."""
        fp, keep = self._export_filter(world, peers)
        n = ctypes.c_size_t()
        rc = self.lib.wq_table_export_device(self.h, fp, ptr or None, capacity, ctypes.byref(n))
        del keep
        if rc not in (0, abi.WQ_E_CAPACITY):
            self._check(rc)
        return rc, n.value

    def set_fanout_hint(self, pairs_per_message: float) -> None:
        """Expected recipients per message (e.g. the previous tick's P / M): >= 16 selects the
        count / scan / emit tick shape (wq_set_fanout_hint)."""
        self._check(self.lib.wq_set_fanout_hint(self.h, float(pairs_per_message)))

    def route_shape(self):
        """(heavy_fanout, fanout_auto) of the next default-config tick (wq_debug_route_shape)."""
        a, b = ctypes.c_int(), ctypes.c_int()
        self._check(self.lib.wq_debug_route_shape(self.h, ctypes.byref(a), ctypes.byref(b)))
        return bool(a.value), bool(b.value)

    def route_health(self):
        """(error bits OR, overflow OR) over every route / global call since the last read
        (wq_route_health; clears them)."""
        e, o = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.wq_route_health(self.h, ctypes.byref(e), ctypes.byref(o)))
        return e.value, o.value

    def check_health(self) -> None:
        """Raises WQError when any tick since the last check reported an error or an overflow."""
        e, o = self.route_health()
        if e & 16:
            raise WQError(abi.WQ_E_INVALID, f"a device op batch held an invalid op and was not applied "
                                            f"(error bits {e:#x})")
        if e & 8:
            raise WQError(abi.WQ_E_INVALID, f"a tick ran on a table still missing an incremental batch the "
                                            f"device could not apply (error bits {e:#x})")
        if e & 4:
            raise WQError(abi.WQ_E_TIMEOUT, f"a route look-back spin gave up (error bits {e:#x})")
        if e or o:
            raise WQError(abi.WQ_E_CAPACITY, f"route error bits {e:#x}, overflow {o}")

    def set_stream(self, stream_ptr: int | None) -> None:
        self._check(self.lib.wq_set_stream(self.h, stream_ptr or None))

    # ---- queries ----
    def is_subscribed(self, world, peer, key_is_raw: bool, key_or_pos) -> np.ndarray:
        world = np.ascontiguousarray(world, dtype=np.uint32)
        peer = np.ascontiguousarray(peer, dtype=np.uint32)
        k = np.ascontiguousarray(key_or_pos, dtype=np.int64 if key_is_raw else np.float64).reshape(-1, 3)
        out = np.zeros(len(world), dtype=np.uint8)
        self._check(self.lib.wq_is_subscribed(self.h, len(world), _p(world), _p(peer), int(key_is_raw), _p(k),
                                              _p(out)))
        return out.astype(bool)

    def is_subscribed_any(self, world, peer) -> np.ndarray:
        world = np.ascontiguousarray(world, dtype=np.uint32)
        peer = np.ascontiguousarray(peer, dtype=np.uint32)
        out = np.zeros(len(world), dtype=np.uint8)
        self._check(self.lib.wq_is_subscribed_any(self.h, len(world), _p(world), _p(peer), _p(out)))
        return out.astype(bool)

    def world_peers(self, world: int) -> np.ndarray:
        n = ctypes.c_size_t()
        rc = self.lib.wq_world_peers(self.h, world, None, 0, ctypes.byref(n))
        if rc not in (0, abi.WQ_E_CAPACITY):
            self._check(rc)
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        self._check(self.lib.wq_world_peers(self.h, world, _p(out), n.value, ctypes.byref(n)))
        return out[: n.value]

    def update_counts(self, lanes: bool = False):
        """(batches applied incrementally, batches that fell back to the full rebuild)
        [+ incremental batches in which a cube took the wave path (list > 48 peers), lanes=True]."""
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.wq_debug_update_counts(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return (a.value, b.value, c.value) if lanes else (a.value, b.value)

    def set_record_slack(self, slots_per_cube: int) -> None:
        self._check(self.lib.wq_debug_set_record_slack(self.h, slots_per_cube))

    def route_config_count(self) -> int:
        return int(self.lib.wq_debug_route_config_count())

    def set_route_config(self, cfg: int) -> None:
        self._check(self.lib.wq_debug_set_route_config(self.h, cfg))

    def set_route_chunks(self, chunks: int) -> None:
        """Chunks of the pipelined heavy tick (wq_debug_set_route_chunks; 0 = default)."""
        self._check(self.lib.wq_debug_set_route_chunks(self.h, chunks))

    def route_calls(self) -> int:
        """The handle's route-call counter (wq_debug_route_calls): the single-launch tick's granule tag
        is this counter modulo abi.TICK_TAG_PERIOD, plus one."""
        n = ctypes.c_uint64()
        self._check(self.lib.wq_debug_route_calls(self.h, ctypes.byref(n)))
        return n.value

    def set_route_calls(self, calls: int) -> None:
        """wq_debug_set_route_calls: a test hook that moves the route-call counter."""
        self._check(self.lib.wq_debug_set_route_calls(self.h, calls))

    # ---- instrumentation ----
    def profile_enable(self, on: bool = True) -> None:
        self._check(self.lib.wq_profile_enable(self.h, int(on)))

    def profile_read(self):
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        self._check(self.lib.wq_profile_read(self.h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def profile_read_phases(self):
        """(kernel ms, launches, [count, tile_scan, emit] ms summed over the three-launch launches, their
        number) — wq_profile_read_phases; resets like profile_read."""
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        ph, npz = (ctypes.c_double * 3)(), ctypes.c_uint64()
        self._check(self.lib.wq_profile_read_phases(self.h, ctypes.byref(ms), ctypes.byref(n), ph, ctypes.byref(npz)))
        return ms.value, n.value, list(ph), npz.value

    def probe_sclk(self) -> float:
        """The shader clock in MHz right now (wq_probe_sclk)."""
        mhz = ctypes.c_double()
        self._check(self.lib.wq_probe_sclk(self.h, ctypes.byref(mhz)))
        return mhz.value


class Hub:
    """An in-process exchange for G router handles of one process (wq_hub_create)."""

    def __init__(self, n_shards: int):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.wq_hub_create(n_shards, ctypes.byref(h))
        if rc != 0:
            raise WQError(rc, "wq_hub_create")
        self.h = h
        self.n_shards = n_shards

    def close(self):
        if getattr(self, "h", None):
            self.lib.wq_hub_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rccl_unique_id() -> bytes:
    """wq_rccl_unique_id: the 128-byte communicator id rank 0 hands to every rank."""
    lib = load_library()
    buf = ctypes.create_string_buffer(abi.RCCL_ID_BYTES)
    rc = lib.wq_rccl_unique_id(buf)
    if rc != 0:
        raise WQError(rc, "wq_rccl_unique_id (librccl not loadable?)")
    return buf.raw
