// wq_shard_exchange.hip — the exchanges of the multi-GPU tick (wq_sharded.hip, wq_sharded_slots.hip),
// all ordered on the handle's stream, segments contiguous in rank order:
//   RCCL      grouped ncclSend / ncclRecv over xGMI; librccl is loaded at run time (the copy a
//             PyTorch process already holds, else the system's), so the library has no link-time
//             RCCL dependency; the self segment is a device copy;
//   hub       G handles of ONE process (a server driving its GPUs from one thread each): a
//             barrier and peer copies (hipMemcpyPeerAsync over xGMI between GPUs);
//   callback  the caller's all-to-all (e.g. gloo in tests).
// Every wait is bounded. Attaching a handle to an exchange, releasing it, and the small ABI calls
// that only read the attachment live here too.
#include <dlfcn.h>

#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include <rocprim/rocprim.hpp>

#include "route_scan.hpp"
#include "shard_ctx.hpp"

// ---------------------------------------------------------------------------------------------
// in-process hub
// ---------------------------------------------------------------------------------------------
struct wq_hub {
    uint32_t G = 0;
    std::mutex mu;
    std::condition_variable cv;
    uint32_t arrived = 0;
    uint64_t gen = 0;
    bool broken = false;  // a rank timed out: every later wait fails at once
    struct Post {
        const void* const* send = nullptr;  // per buffer
        const size_t* const* sbytes = nullptr;
        int n = 0;
        int device = 0;
        hipEvent_t ready = nullptr;  // the poster's send buffers are complete once this has fired
        hipEvent_t done = nullptr;   // the poster has finished reading its peers' send buffers
    };
    std::vector<Post> post;
    std::vector<uint32_t> attached;

    // Generation barrier, bounded: false on timeout (then the hub is broken for good).
    bool barrier(double timeout_s) {
        std::unique_lock<std::mutex> lk(mu);
        if (broken) return false;
        const uint64_t g = gen;
        if (++arrived == G) {
            arrived = 0;
            ++gen;
            cv.notify_all();
            return true;
        }
        const bool ok = cv.wait_for(lk, std::chrono::duration<double>(timeout_s),
                                    [&] { return gen != g || broken; });
        if (!ok || broken) {
            broken = true;
            cv.notify_all();
            return false;
        }
        return true;
    }
};

namespace wq {

// ---------------------------------------------------------------------------------------------
// RCCL, resolved at run time
// ---------------------------------------------------------------------------------------------
namespace {

struct RcclApi {
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
    std::string why;
};

RcclApi& rccl() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* lib = nullptr;
        const char* env = getenv("WQ_RCCL_LIBRARY");
        if (env && *env) lib = dlopen(env, RTLD_NOW | RTLD_LOCAL);
        // the copy a PyTorch-ROCm process has already loaded (one RCCL per process), else the system's
        const char* names[] = {"librccl.so", "librccl.so.1"};
        for (const char* n : names)
            if (!lib) lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
        for (const char* n : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"})
            if (!lib) lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (!lib) {
            api.why = std::string("librccl not found: ") + (dlerror() ? dlerror() : "");
            return;
        }
        api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
        api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
        api.Send = reinterpret_cast<decltype(api.Send)>(dlsym(lib, "ncclSend"));
        api.Recv = reinterpret_cast<decltype(api.Recv)>(dlsym(lib, "ncclRecv"));
        api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(dlsym(lib, "ncclGroupStart"));
        api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(dlsym(lib, "ncclGroupEnd"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
        api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.Send && api.Recv && api.GroupStart &&
                 api.GroupEnd && api.GetErrorString;
        if (!api.ok) api.why = "librccl lacks ncclSend / ncclRecv / group calls";
    });
    return api;
}

constexpr double kHubTimeoutS = 120.0;

std::vector<size_t> prefix(const size_t* b, uint32_t G) {
    std::vector<size_t> o(G + 1, 0);
    for (uint32_t i = 0; i < G; ++i) o[i + 1] = o[i] + b[i];
    return o;
}

}  // namespace

uint32_t pass_blocks(uint32_t n) {
    static const uint32_t env = getenv("WQ_DEBUG_SHARD_TPB") ? (uint32_t)std::max(1, atoi(getenv("WQ_DEBUG_SHARD_TPB"))) : 0u;
    const uint32_t tpb = env ? env : route_tiles_per_block(n);
    return (n + tpb - 1) / tpb;
}

int exchange(wq_router* h, const Xfer& x) {
    ShardCtx& sc = *h->shard;
    const uint32_t G = sc.G, me = sc.rank;
    hipStream_t s = h->stream;
    if (sc.kind == kXCallback) {
        for (int k = 0; k < x.n; ++k) {
            if (x.skip_self[k]) return set_error(h, WQ_E_INVALID, "exchange: the caller's callback copies every segment");
            const int rc = sc.fn(sc.fn_ctx, x.send[k], x.sbytes[k], x.recv[k], x.rbytes[k], (void*)s);
            if (rc) return set_error(h, WQ_E_RCCL, "the caller's exchange callback failed");
        }
        return WQ_OK;
    }
    if (sc.kind == kXRccl) {
        RcclApi& api = rccl();
        for (int k = 0; k < x.n; ++k) {  // the self segment: a device copy
            const auto so = prefix(x.sbytes[k], G), ro = prefix(x.rbytes[k], G);
            if (x.sbytes[k][me] != x.rbytes[k][me]) return set_error(h, WQ_E_INVALID, "self segment size mismatch");
            if (x.sbytes[k][me] && !x.skip_self[k])
                WQ_HIP(h, hipMemcpyAsync(static_cast<char*>(x.recv[k]) + ro[me],
                                         static_cast<const char*>(x.send[k]) + so[me], x.sbytes[k][me],
                                         hipMemcpyDeviceToDevice, s));
        }
        ncclResult_t r = api.GroupStart();
        for (int k = 0; k < x.n && r == ncclSuccess; ++k) {
            const auto so = prefix(x.sbytes[k], G), ro = prefix(x.rbytes[k], G);
            for (uint32_t p = 0; p < G && r == ncclSuccess; ++p) {
                if (p == me) continue;
                if (x.sbytes[k][p])
                    r = api.Send(static_cast<const char*>(x.send[k]) + so[p], x.sbytes[k][p], ncclUint8, (int)p,
                                 sc.comm, s);
                if (r == ncclSuccess && x.rbytes[k][p])
                    r = api.Recv(static_cast<char*>(x.recv[k]) + ro[p], x.rbytes[k][p], ncclUint8, (int)p, sc.comm,
                                 s);
            }
        }
        const ncclResult_t r2 = api.GroupEnd();
        if (r == ncclSuccess) r = r2;
        if (r != ncclSuccess) {
            h->err = std::string("RCCL exchange: ") + api.GetErrorString(r);
            return WQ_E_RCCL;
        }
        return WQ_OK;
    }
    if (sc.kind == kXHub) {
        // No host wait on the GPU: each rank's send buffers are complete at its `ready` event, which
        // the readers' streams wait on before their peer copies; each reader records `done` after
        // them, and every rank's stream waits on all `done` events before it goes on (and may
        // overwrite a send buffer). The host threads only meet at the two barriers.
        wq_hub& hub = *sc.hub;
        WQ_HIP(h, hipEventRecord(sc.ev_ready, s));
        wq_hub::Post& mine = hub.post[me];
        mine.send = x.send;
        mine.sbytes = x.sbytes;
        mine.n = x.n;
        mine.device = h->device;
        mine.ready = sc.ev_ready;
        if (!hub.barrier(kHubTimeoutS)) return set_error(h, WQ_E_RCCL, "hub exchange: a peer never arrived");
        int rc = WQ_OK;
        for (uint32_t src = 0; src < G && rc == WQ_OK; ++src) {
            const wq_hub::Post& p = hub.post[src];
            if (p.n != x.n) {
                rc = set_error(h, WQ_E_INVALID, "hub exchange: ranks disagree on the buffer count");
                break;
            }
            if (src != me) {
                const hipError_t we = hipStreamWaitEvent(s, p.ready, 0);
                if (we != hipSuccess) {
                    rc = set_error(h, WQ_E_HIP, "hub exchange wait", we);
                    break;
                }
            }
            for (int k = 0; k < x.n; ++k) {
                const size_t bytes = p.sbytes[k][me];
                if (bytes != x.rbytes[k][src]) {
                    rc = set_error(h, WQ_E_INVALID, "hub exchange: send / receive sizes disagree");
                    break;
                }
                if (!bytes || (src == me && x.skip_self[k])) continue;
                size_t soff = 0, roff = 0;
                for (uint32_t d = 0; d < me; ++d) soff += p.sbytes[k][d];
                for (uint32_t q = 0; q < src; ++q) roff += x.rbytes[k][q];
                char* dst = static_cast<char*>(x.recv[k]) + roff;
                const char* from = static_cast<const char*>(p.send[k]) + soff;
                const hipError_t e = p.device == h->device
                                         ? hipMemcpyAsync(dst, from, bytes, hipMemcpyDeviceToDevice, s)
                                         : hipMemcpyPeerAsync(dst, h->device, from, p.device, bytes, s);
                if (e != hipSuccess) {
                    rc = set_error(h, WQ_E_HIP, "hub exchange copy", e);
                    break;
                }
            }
        }
        hipError_t e = hipEventRecord(sc.ev_done, s);  // done reading the peers' buffers ...
        mine.done = sc.ev_done;
        if (!hub.barrier(kHubTimeoutS))                  // ... before any of them reuses one
            return set_error(h, WQ_E_RCCL, "hub exchange: a peer never finished");
        for (uint32_t d = 0; d < G && e == hipSuccess; ++d)
            if (d != me) e = hipStreamWaitEvent(s, hub.post[d].done, 0);
        if (rc) return rc;
        if (e != hipSuccess) return set_error(h, WQ_E_HIP, "hub exchange events", e);
        return WQ_OK;
    }
    return set_error(h, WQ_E_INVALID, "no exchange attached");
}

int fatal_receive(wq_router* h, const char* what) {
    ShardCtx& sc = *h->shard;
    if (sc.kind == kXHub) {
        std::lock_guard<std::mutex> lk(sc.hub->mu);
        sc.hub->broken = true;
        sc.hub->cv.notify_all();
    }
    return set_error(h, WQ_E_OOM, what);
}

int status_error(wq_router* h, uint64_t st, uint32_t from) {
    const uint32_t bits = (uint32_t)(st >> 32), code = (uint32_t)st;
    std::string who = " (shard " + std::to_string(from) + ")";
    if (code) return set_error(h, -(int)code, ("sharded tick: a shard's local step failed" + who).c_str());
    if (bits & kErrStale)
        return set_error(h, WQ_E_INVALID, ("sharded tick: a shard's table is still missing an incremental batch the "
                                           "device could not apply" + who).c_str());
    if (bits & 4u) return set_error(h, WQ_E_TIMEOUT, ("sharded tick: a bounded spin gave up" + who).c_str());
    return set_error(h, WQ_E_CAPACITY, ("sharded tick: more than 2^32-1 pairs in one owner block" + who).c_str());
}

int scan_excl(wq_router* h, DevBuf& tmp, const uint32_t* in, uint32_t* out, size_t n) {
    if (!n) return WQ_OK;
    // one launch (route_scan.hpp launch_scan_u32) up to 2^32 - 1 elements; WQ_SCAN_MULTI=0: rocPRIM
    static const bool multi = !getenv("WQ_SCAN_MULTI") || atoi(getenv("WQ_SCAN_MULTI")) != 0;
    if (multi && n < 0xFFFFFFFFull) return launch_scan_u32(h, in, out, (uint32_t)n, nullptr);
    size_t bytes = 0;
    WQ_HIP(h, rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), h->stream));
    WQ_ALLOC(h, tmp, bytes);
    WQ_HIP(h, rocprim::exclusive_scan(tmp.p, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), h->stream));
    return WQ_OK;
}

namespace {

int attach(wq_router* h, uint32_t G, uint32_t rank) {
    if (!h || G == 0 || G > WQ_MAX_SHARDS || rank >= G) return WQ_E_INVALID;
    if (h->shard) return set_error(h, WQ_E_INVALID, "an exchange is already attached (wq_shard_detach first)");
    h->shard = new (std::nothrow) ShardCtx();
    if (!h->shard) return WQ_E_OOM;
    ShardCtx& sc = *h->shard;
    sc.G = G;
    sc.rank = rank;
    // the small exchange vectors live here for the handle's whole attachment: a tick never has to
    // allocate before its first exchange
    bool ok = sc.small.ensure(kSmallBytes) == hipSuccess &&
              hipHostMalloc(&sc.hsmall, kSmallBytes, hipHostMallocDefault) == hipSuccess &&
              hipStreamCreateWithFlags(&sc.side, hipStreamNonBlocking) == hipSuccess;
    // the hub's events order peer copies (system scope); the side stream's fork / join only work on
    // this device: a device-scope release is enough there
    for (hipEvent_t* e : {&sc.ev_ready, &sc.ev_done})
        ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    for (hipEvent_t* e : {&sc.ev_fork, &sc.ev_join})
        ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming | hipEventReleaseToDevice) == hipSuccess;
    for (uint32_t k = 0; k < ShardCtx::kRing; ++k) {
        ok = ok && hipHostMalloc(&sc.asnap[k], kSmallBytes + 64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess;
        if (ok) memset(sc.asnap[k], 0, kSmallBytes + 64);
    }
    if (!ok) {
        shard_release(h);
        return set_error(h, WQ_E_OOM, "shard exchange vectors / stream / events");
    }
    sc.b1_out.assign(G, 0);
    sc.b1_in.assign(G, 0);
    sc.b2_out.assign(G, 0);
    sc.b2_in.assign(G, 0);
    return WQ_OK;
}

}  // namespace

void shard_release(wq_router* h) {
    if (!h->shard) return;
    ShardCtx* sc = h->shard;
    if (sc->kind == kXRccl && sc->comm) (void)rccl().CommDestroy(sc->comm);
    if (sc->side) (void)hipStreamSynchronize(sc->side);
    for (DevBuf* b : sc->bufs()) b->release();
    if (sc->hsmall) (void)hipHostFree(sc->hsmall);
    for (uint32_t k = 0; k < ShardCtx::kRing; ++k)
        if (sc->asnap[k]) (void)hipHostFree(sc->asnap[k]);
    if (sc->side) (void)hipStreamDestroy(sc->side);
    for (hipEvent_t e : {sc->ev_fork, sc->ev_join, sc->ev_ready, sc->ev_done})
        if (e) (void)hipEventDestroy(e);
    delete sc;
    h->shard = nullptr;
}

}  // namespace wq

using namespace wq;

extern "C" {

int wq_hub_create(uint32_t n_shards, wq_hub** out) {
    if (!out || n_shards == 0 || n_shards > WQ_MAX_SHARDS) return WQ_E_INVALID;
    wq_hub* hub = new (std::nothrow) wq_hub();
    if (!hub) return WQ_E_OOM;
    hub->G = n_shards;
    hub->post.resize(n_shards);
    *out = hub;
    return WQ_OK;
}

int wq_hub_destroy(wq_hub* hub) {
    if (!hub) return WQ_E_INVALID;
    delete hub;
    return WQ_OK;
}

int wq_shard_attach_hub(wq_router* h, wq_hub* hub, uint32_t rank) {
    if (!h || !hub) return WQ_E_INVALID;
    int rc = attach(h, hub->G, rank);
    if (rc) return rc;
    h->shard->kind = kXHub;
    h->shard->hub = hub;
    return WQ_OK;
}

int wq_shard_attach_exchange(wq_router* h, uint32_t n_shards, uint32_t rank, wq_exchange_fn fn, void* ctx) {
    if (!h || !fn) return WQ_E_INVALID;
    int rc = attach(h, n_shards, rank);
    if (rc) return rc;
    h->shard->kind = kXCallback;
    h->shard->fn = fn;
    h->shard->fn_ctx = ctx;
    return WQ_OK;
}

int wq_rccl_unique_id(uint8_t* id_out) {
    if (!id_out) return WQ_E_INVALID;
    RcclApi& api = rccl();
    if (!api.ok) return WQ_E_RCCL;
    ncclUniqueId id;
    if (api.GetUniqueId(&id) != ncclSuccess) return WQ_E_RCCL;
    static_assert(sizeof(id) == WQ_RCCL_ID_BYTES, "ncclUniqueId is 128 bytes");
    memcpy(id_out, &id, sizeof(id));
    return WQ_OK;
}

int wq_shard_attach_rccl(wq_router* h, uint32_t n_shards, uint32_t rank, const uint8_t* id) {
    if (!h || !id) return WQ_E_INVALID;
    RcclApi& api = rccl();
    if (!api.ok) return set_error(h, WQ_E_RCCL, api.why.c_str());
    WQ_HIP(h, hipSetDevice(h->device));
    int rc = attach(h, n_shards, rank);
    if (rc) return rc;
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    const ncclResult_t r = api.CommInitRank(&comm, (int)n_shards, uid, (int)rank);
    if (r != ncclSuccess) {
        shard_release(h);
        h->err = std::string("ncclCommInitRank: ") + api.GetErrorString(r);
        return WQ_E_RCCL;
    }
    h->shard->kind = kXRccl;
    h->shard->comm = comm;
    return WQ_OK;
}

int wq_shard_detach(wq_router* h) {
    if (!h) return WQ_E_INVALID;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    shard_release(h);
    return WQ_OK;
}

int wq_shard_info(wq_router* h, uint32_t* n_shards, uint32_t* rank) {
    if (!h || !n_shards || !rank) return WQ_E_INVALID;
    *n_shards = h->shard ? h->shard->G : 1;
    *rank = h->shard ? h->shard->rank : 0;
    return WQ_OK;
}

int wq_shard_last_bytes(wq_router* h, uint64_t* sent, uint64_t* received) {
    if (!h || !sent || !received) return WQ_E_INVALID;
    *sent = h->shard ? h->shard->last_sent : 0;
    *received = h->shard ? h->shard->last_recv : 0;
    return WQ_OK;
}

int wq_shard_tick_stats(wq_router* h, uint64_t* exact, uint64_t* budgeted) {
    if (!h || !exact || !budgeted) return WQ_E_INVALID;
    *exact = h->shard ? h->shard->n_exact : 0;
    *budgeted = h->shard ? h->shard->n_budget : 0;
    return WQ_OK;
}

int wq_debug_inject_shard_failure(wq_router* h, int step) {
    if (!h || step < 0 || step > 3) return WQ_E_INVALID;
    h->shard_inject = step;
    return WQ_OK;
}

int wq_debug_set_shard_form(wq_router* h, int expanded) {
    if (!h) return WQ_E_INVALID;
    h->shard_expanded = expanded != 0;
    return WQ_OK;
}

}  // extern "C"
