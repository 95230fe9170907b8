// wq_sharded.hip — the multi-GPU tick behind the C ABI (include/wq_router.h
// "multi-GPU: sharded ticks"): the expanded-record form, and the entry points of the CSR forms.
//
// The reference keeps ONE WorldMap owned by one task (worldql_server/src/processing/thread.rs:
// 113-148). Here G router handles — one per GPU, as threads of one process or one process per
// GPU — each own the (world, cube) buckets with shard_of(world, cube) == rank, and a tick of
// LocalMessages ingested anywhere is
//   1. shard    quantise, owner, group by owner into 40-byte records (wq_shard.hip kernels)
//   2. A2A      per-owner record counts (host read 1), then the records
//   3. route    the single-GPU count / scan / emit on what the owner received (wq_route.hip)
//   4. A2A      per-source pair counts (host read 2: the sizes the next exchange needs)
//   5. A2A      per-record recipient counts and the peers, back to the ingesting GPU (one group)
//   6. unshard  the CSR in the ingesting GPU's own message order: offsets[M+1], peers[P], msgs[P]
// so wq_sharded_route_tick_device returns exactly what wq_route_tick_device returns on one GPU
// holding the whole table (local_message.rs:52-86 per message, on the owner).
//
// wq_sharded_route_tick_device runs this form when wq_debug_set_shard_form selects it; its default
// is the slot tick of wq_sharded_slots.hip. The exchanges are wq_shard_exchange.hip's. A rank whose
// local step fails still completes the tick's exchanges with consistent sizes (so no peer is left
// waiting) and reports the error at the end.
#include "shard_ctx.hpp"

namespace wq {
namespace {

// per received record: its recipient count; per source segment: {pair count, status}. A route that
// reported an error (counter bits: 4 spin, 2 > 2^32 pairs, 8 stale table) sends no pairs, and its
// status tells every source so, before any pair is exchanged.
__global__ void k_owner_counts(const uint32_t* __restrict__ off, uint32_t R, SegBounds seg, uint32_t G,
                               uint32_t* __restrict__ e, unsigned long long* __restrict__ pc,
                               const wq_route_counters* __restrict__ cnt, const uint32_t* __restrict__ stale) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < R) e[i] = off[i + 1] - off[i];
    if (blockIdx.x == 0 && threadIdx.x < G) {
        uint32_t err = cnt ? cnt->error : 0u;
        if (stale && *stale) err |= kErrStale;
        const uint32_t d = threadIdx.x;
        pc[2 * d] = err ? 0ull : (unsigned long long)(off[seg.b[d + 1]] - off[seg.b[d]]);
        pc[2 * d + 1] = (unsigned long long)err << 32;
    }
}

// counts in message order: by_msg[rec.msg] = e of the record (every message has one record)
__global__ void k_counts_by_msg(const wq_msg_rec* __restrict__ recs, const uint32_t* __restrict__ e, uint32_t M,
                                uint32_t* __restrict__ by_msg) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < M) by_msg[recs[i].msg] = e[i];
}

__global__ void k_set_last(uint32_t* __restrict__ a, uint32_t at, uint32_t v) { a[at] = v; }

// Block b moves the runs of records [256b, 256b + 256) — record i's e[i] peers at ret_off[i] in
// record order — to offsets[msg_i] in message order. Windows of W = R * 256 of the block's outputs:
// each record marks where its run enters the window in a u16 owner map (index + 1), a block-wide
// max-scan carries each owner over its outputs, and thread t moves outputs t, t + 256, ... of the
// window (contiguous reads; each run written contiguously at its message's offset). C3 on one
// shard: 1,059 us (about 5 GB moved: 4.7 TB/s), 1,088 us with an 8-step binary search over the
// run starts per output instead — the move is bandwidth-bound either way.
template <int R>
__global__ __launch_bounds__(kBlock) void k_unshard(const wq_msg_rec* __restrict__ recs, const uint32_t* __restrict__ ret_off,
                                                    const uint32_t* __restrict__ peers_in, uint32_t M, uint32_t P,
                                                    const uint32_t* __restrict__ offsets, uint32_t* __restrict__ peers,
                                                    uint32_t* __restrict__ msgs) {
    static_assert(R % 8 == 0, "map rows of whole 16-byte words");
    constexpr uint32_t W = R * kBlock;
    __shared__ alignas(16) uint16_t map[W];
    __shared__ uint32_t st[kBlock], dst[kBlock], msg[kBlock];
    __shared__ uint32_t wave_max[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t i0 = blockIdx.x * kBlock, i = i0 + tid;
    const uint32_t base = ret_off[i0];
    const uint32_t end = i0 + kBlock < M ? ret_off[i0 + kBlock] : P;
    const uint32_t T = end - base;
    uint32_t my_st = 0, my_e = 0;
    if (i < M) {
        const uint32_t m = recs[i].msg;
        const uint32_t a = ret_off[i];
        my_st = a - base;
        my_e = (i + 1 < M ? ret_off[i + 1] : P) - a;
        st[tid] = my_st;
        dst[tid] = offsets[m];
        msg[tid] = m;
    }
    uint4* my_map = reinterpret_cast<uint4*>(map) + tid * (R / 8);
    for (uint32_t w0 = 0; w0 < T; w0 += W) {
#pragma unroll
        for (int q = 0; q < R / 8; ++q) my_map[q] = make_uint4(0, 0, 0, 0);
        lds_barrier();
        if (my_e && my_st + my_e > w0 && my_st < w0 + W) map[(my_st > w0 ? my_st : w0) - w0] = (uint16_t)(tid + 1);
        lds_barrier();
        uint4 v[R / 8];
#pragma unroll
        for (int q = 0; q < R / 8; ++q) v[q] = my_map[q];
        uint32_t run = 0;
#pragma unroll
        for (int q = 0; q < R / 8; ++q) {
            uint32_t* w = reinterpret_cast<uint32_t*>(&v[q]);
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                uint32_t lo = w[h] & 0xFFFFu, hi = w[h] >> 16;
                run = lo > run ? lo : run;
                lo = run;
                run = hi > run ? hi : run;
                w[h] = lo | (run << 16);
            }
        }
        const uint32_t incl = wave_incl_scan_max(run, lane);
        uint32_t pre = __shfl_up(incl, 1, 64);
        if (lane == 0) pre = 0;
        if (lane == 63) wave_max[wave] = incl;
        lds_barrier();
#pragma unroll
        for (int u = 0; u < kWaves; ++u)
            if (u < wave) pre = wave_max[u] > pre ? wave_max[u] : pre;
#pragma unroll
        for (int q = 0; q < R / 8; ++q) {
            uint32_t* w = reinterpret_cast<uint32_t*>(&v[q]);
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const uint32_t lo = w[h] & 0xFFFFu, hi = w[h] >> 16;
                w[h] = (lo > pre ? lo : pre) | ((hi > pre ? hi : pre) << 16);
            }
            my_map[q] = v[q];
        }
        lds_barrier();
        const uint32_t last = (T - 1 - w0) < W - 1 ? (T - 1 - w0) : W - 1;
        uint32_t pv[R], oo[R], own[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const uint32_t x = (uint32_t)(u * kBlock + tid) < last ? (uint32_t)(u * kBlock + tid) : last;
            const uint32_t j = (uint32_t)map[x] - 1u;
            const uint32_t r = w0 + x;
            pv[u] = peers_in[base + r];
            oo[u] = dst[j] + (r - st[j]);
            own[u] = j;
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            if (w0 + u * kBlock + tid < T) {
                peers[oo[u]] = pv[u];
                if (msgs) msgs[oo[u]] = msg[own[u]];
            }
        }
        lds_barrier();  // the next window rewrites the map
    }
}

// Steps 1-3 of a sharded tick, shared by the origin and owner forms: shard this rank's messages,
// exchange the counts (host read 1) and the records, route what this shard owns into
// own_off / own_peers. *R_out = records received, *seg = their source segments. A local route
// failure is left in *late (the caller keeps the collective going); a return value != WQ_OK is
// an exchange or argument failure.
int shard_exchange_route(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                         const uint32_t* d_sender, const uint8_t* d_repl, size_t n_msgs, uint64_t* R_out,
                         SegBounds* seg_out, Late* late_out) {
    hipStream_t s = h->stream;
    ShardCtx& sc = *h->shard;
    const uint32_t G = sc.G;
    const size_t M = n_msgs;
    sc.last_ready = false;
    sc.last_slots = false;
    sc.small_zeroed = false;  // this form writes the small vectors its own way
    Late& late = *late_out;   // a local failure, reported once the tick's exchanges are complete
    auto fail = [&](int rc) { return late.fail(h, rc); };

    const int inject = h->shard_inject;
    h->shard_inject = 0;
    // 1. shard (a failure here: this shard sends nothing, and reports the error after the exchanges)
    uint32_t* cnt_send = reinterpret_cast<uint32_t*>(sc.small.as<char>() + kSmallA);
    uint32_t* cnt_recv = cnt_send + G;
    WQ_HIP(h, hipMemsetAsync(cnt_send, 0, 4 * G, s));
    if (inject == 1) fail(set_error(h, WQ_E_INVALID, "injected failure at step 1 (test hook)"));
    // as the slot tick and the single-GPU tick: the radius filter needs the message positions
    if (h->radius > 0.0 && M && !d_pos && !late)
        fail(set_error(h, WQ_E_INVALID, "the radius filter needs message positions"));
    int rc = late ? late.code : sc.recs.ensure((M ? M : 1) * sizeof(wq_msg_rec)) == hipSuccess
                 ? WQ_OK
                 : set_error(h, WQ_E_OOM, "hipMalloc of the sharded tick's records");
    if (!fail(rc))
        fail(launch_shard_messages(h, d_pos, d_keys, d_world, d_sender, d_repl, M, G, sc.recs.as<wq_msg_rec>(),
                                   cnt_send));
    if (late) WQ_HIP(h, hipMemsetAsync(cnt_send, 0, 4 * G, s));
    // 2. counts, then the records
    std::vector<size_t> four(G, 4);
    {
        Xfer x{{cnt_send}, {four.data()}, {cnt_recv}, {four.data()}, 1};
        if ((rc = exchange(h, x))) return rc;
    }
    sc.sc.assign(2 * G, 0);
    WQ_HIP(h, hipMemcpyAsync(sc.sc.data(), cnt_send, 2 * G * 4, hipMemcpyDeviceToHost, s));
    WQ_HIP(h, hipStreamSynchronize(s));  // host read 1
    sc.rc.assign(sc.sc.begin() + G, sc.sc.end());
    sc.sc.resize(G);
    uint64_t R = 0;
    std::vector<size_t> sb(G), rb(G);
    SegBounds seg;
    seg.b[0] = 0;
    for (uint32_t d = 0; d < G; ++d) {
        sb[d] = (size_t)sc.sc[d] * sizeof(wq_msg_rec);
        rb[d] = (size_t)sc.rc[d] * sizeof(wq_msg_rec);
        R += sc.rc[d];
        seg.b[d + 1] = (uint32_t)R;
    }
    if (R >= 0xFFFFFC00ull) return fatal_receive(h, "more than 2^32 - 1024 records on one owner");
    if (sc.recv.ensure((R ? R : 1) * sizeof(wq_msg_rec)) != hipSuccess)
        return fatal_receive(h, "hipMalloc of the received records");
    {
        Xfer x{{sc.recs.p}, {sb.data()}, {sc.recv.p}, {rb.data()}, 1};
        if ((rc = exchange(h, x))) return rc;
    }
    // 3. route what this shard owns (a failure: empty results here, the error after the exchanges)
    if (!sc.own_cap) {
        sc.own_cap = 16 * R + 4096;
        if (sc.own_cap > 0xFFFFFFFFull) sc.own_cap = 0xFFFFFFFFull;
    }
    const bool bufs = sc.own_off.ensure((R + 1) * 4) == hipSuccess && sc.own_peers.ensure(sc.own_cap * 4) == hipSuccess &&
                      sc.own_e.ensure((R ? R : 1) * 4) == hipSuccess;
    if (!bufs) fail(set_error(h, WQ_E_OOM, "hipMalloc of the owner's route buffers"));
    if (inject == 3) fail(set_error(h, WQ_E_INVALID, "injected failure at step 3 (test hook)"));
    if (!late)
        fail(launch_route_records(h, sc.recv.as<wq_msg_rec>(), R, sc.own_off.as<uint32_t>(), sc.own_peers.as<uint32_t>(),
                                  nullptr, sc.own_cap));
    *R_out = R;
    *seg_out = seg;
    return WQ_OK;
}

}  // namespace

// Unshard the latest tick into the caller's buffers (message order).
int copy_out(wq_router* h, uint32_t* d_offsets, uint32_t* d_peers, uint32_t* d_msgs, size_t capacity) {
    ShardCtx& sc = *h->shard;
    sc.small_zeroed = false;  // the scan rewrites the counters in the small vectors
    const uint64_t M = sc.last_M, P = sc.last_P;
    hipStream_t s = h->stream;
    if (sc.last_slots) {
        // the kept rows of this shard's own cubes point into the table: only while it is unchanged
        if (h->table_gen != sc.last_gen)
            return set_error(h, WQ_E_INVALID, "sharded copy-out: the table changed since the tick (route again)");
        if (int rc = slots_copy_out(h, d_offsets, d_peers, d_msgs, capacity)) return rc;
        if (P > capacity) return set_error(h, WQ_E_CAPACITY, "sharded tick: output capacity too small (required size in *n_pairs)");
        return WQ_OK;
    }
    if (M) {
        WQ_ALLOC(h, sc.by_msg, M * 4);
        const unsigned g = (unsigned)((M + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_counts_by_msg, dim3(g), dim3(kBlock), 0, s, sc.recs.as<wq_msg_rec>(),
                           sc.ret_e.as<uint32_t>(), (uint32_t)M, sc.by_msg.as<uint32_t>());
        WQ_HIP(h, hipGetLastError());
        int rc = scan_excl(h, sc.tmp, sc.by_msg.as<uint32_t>(), d_offsets, M);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_set_last, dim3(1), dim3(1), 0, s, d_offsets, (uint32_t)M, (uint32_t)P);
    WQ_HIP(h, hipGetLastError());
    if (P > capacity) return set_error(h, WQ_E_CAPACITY, "sharded tick: output capacity too small (required size in *n_pairs)");
    if (M && P) {
        const unsigned g = (unsigned)((M + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_unshard<16>, dim3(g), dim3(kBlock), 0, s, sc.recs.as<wq_msg_rec>(), sc.ret_off.as<uint32_t>(),
                           sc.ret_peers.as<uint32_t>(), (uint32_t)M, (uint32_t)P, d_offsets, d_peers, d_msgs);
        WQ_HIP(h, hipGetLastError());
    }
    return WQ_OK;
}

}  // namespace wq

using namespace wq;

extern "C" {

int wq_sharded_apply_ops(wq_router* h, const wq_op* ops, size_t n) {
    if (!h || (n && !ops)) return WQ_E_INVALID;
    if (!h->shard || h->shard->G == 1) return wq_apply_ops(h, ops, n);
    if (n >= 0xFFFFFFFFull) return WQ_E_INVALID;
    WQ_HIP(h, hipSetDevice(h->device));
    ShardCtx& sc = *h->shard;
    std::vector<uint32_t> owner(n);
    int rc = wq_shard_ops(h, ops, n, sc.G, owner.data());
    if (rc) return rc;
    std::vector<wq_op> mine;
    mine.reserve(n / sc.G + 16);
    for (size_t i = 0; i < n; ++i)
        if (owner[i] == sc.rank || owner[i] == WQ_SHARD_ALL) mine.push_back(ops[i]);
    return wq_apply_ops(h, mine.data(), mine.size());
}

int wq_sharded_route_tick_device(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                                 const uint32_t* d_sender, const uint8_t* d_repl, size_t n_msgs, uint32_t* d_offsets,
                                 uint32_t* d_peers, uint32_t* d_msgs, size_t capacity, size_t* n_pairs) {
    if (!n_pairs) return WQ_E_INVALID;
    if (int rc = check_csr_tick(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs, d_offsets, d_peers, capacity))
        return rc;
    WQ_HIP(h, hipSetDevice(h->device));
    if (capacity > 0xFFFFFFFFull) capacity = 0xFFFFFFFFull;
    hipStream_t s = h->stream;
    *n_pairs = 0;
    if (h->shard && !h->shard_expanded)
        return sharded_tick_slots(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs, d_offsets, d_peers, d_msgs,
                                  capacity, n_pairs);
    if (!h->shard) {  // G = 1 without an exchange: the single-GPU tick, P read back
        int rc = launch_route(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs, d_offsets, d_peers, d_msgs, capacity);
        if (rc) return rc;
        wq_route_counters c;
        WQ_HIP(h, hipMemcpyAsync(&c, h->rws.last, sizeof(c), hipMemcpyDeviceToHost, s));
        WQ_HIP(h, hipStreamSynchronize(s));
        *n_pairs = n_msgs ? c.n_pairs : 0;
        if (c.error & 4u) return set_error(h, WQ_E_TIMEOUT, "route look-back spin gave up");
        if (c.error) return set_error(h, WQ_E_CAPACITY, "more than 2^32-1 pairs in one tick");
        if (n_msgs && c.n_pairs > capacity) return set_error(h, WQ_E_CAPACITY, "output capacity too small");
        return WQ_OK;
    }
    ShardCtx& sc = *h->shard;
    const uint32_t G = sc.G, me = sc.rank;
    const size_t M = n_msgs;
    Late late;
    uint64_t R = 0;
    SegBounds seg;
    int rc = shard_exchange_route(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs, &R, &seg, &late);
    if (rc) return rc;
    std::vector<size_t> sixteen(G, 16);
    // 4. per-record counts; per source {pair count, status}, exchanged before any pair moves
    unsigned long long* pc_send = reinterpret_cast<unsigned long long*>(sc.small.as<char>() + kSmallC);
    unsigned long long* pc_recv = pc_send + 2 * G;
    if (!late) {
        hipLaunchKernelGGL(k_owner_counts, dim3((unsigned)((R + kBlock - 1) / kBlock) + 1), dim3(kBlock), 0, s,
                           sc.own_off.as<uint32_t>(), (uint32_t)R, seg, G, sc.own_e.as<uint32_t>(), pc_send,
                           R ? h->rws.last : nullptr, h->tab.stale.as<uint32_t>());
        if (hipGetLastError() != hipSuccess) late.fail(h, set_error(h, WQ_E_HIP, "owner counts launch"));
    }
    std::vector<unsigned long long> pc_status(2 * G, 0);  // lives until host read 2 below
    if (late) {
        for (uint32_t d = 0; d < G; ++d) pc_status[2 * d + 1] = status_of(late.code);
        WQ_HIP(h, hipMemcpyAsync(pc_send, pc_status.data(), 16 * G, hipMemcpyHostToDevice, s));
    }
    {
        Xfer x{{pc_send}, {sixteen.data()}, {pc_recv}, {sixteen.data()}, 1};
        if ((rc = exchange(h, x))) return rc;
    }
    std::vector<unsigned long long> hp(4 * G);
    WQ_HIP(h, hipMemcpyAsync(hp.data(), pc_send, 32 * G, hipMemcpyDeviceToHost, s));
    WQ_HIP(h, hipStreamSynchronize(s));  // host read 2
    uint64_t peer_status = 0, P_own = 0;
    uint32_t peer_from = 0;
    for (uint32_t d = 0; d < G; ++d) {
        P_own += hp[2 * d];
        const uint64_t st = hp[2 * G + 2 * d + 1];
        if (st && !peer_status) {
            peer_status = st;
            peer_from = d;
        }
    }
    if (!late && P_own > sc.own_cap) {  // the pair buffer was short: offsets are right, route again
        sc.own_cap = P_own + P_own / 4 + 4096;
        if (sc.own_cap > 0xFFFFFFFFull) sc.own_cap = 0xFFFFFFFFull;
        // the sizes are promised: a shard that cannot keep the promise breaks the collective
        if (sc.own_peers.ensure(sc.own_cap * 4) != hipSuccess) return fatal_receive(h, "hipMalloc of the owner's pairs");
        if ((rc = launch_route_records(h, sc.recv.as<wq_msg_rec>(), R, sc.own_off.as<uint32_t>(),
                                       sc.own_peers.as<uint32_t>(), nullptr, sc.own_cap)))
            return fatal_receive(h, "owner re-route");
    }
    // 5. recipient counts and peers back to the ingesting shards (one exchange group); a shard whose
    // local step failed sends none of either, as its status said
    std::vector<size_t> eb_s(G), eb_r(G), pb_s(G), pb_r(G);
    uint64_t P = 0;
    for (uint32_t d = 0; d < G; ++d) {
        const bool d_failed = (uint32_t)hp[2 * G + 2 * d + 1] != 0;
        eb_s[d] = late ? 0 : (size_t)sc.rc[d] * 4;      // to source d: e of the records it sent here
        eb_r[d] = d_failed ? 0 : (size_t)sc.sc[d] * 4;  // from owner d: e of the records sent there
        pb_s[d] = (size_t)hp[2 * d] * 4;
        pb_r[d] = (size_t)hp[2 * G + 2 * d] * 4;
        P += hp[2 * G + 2 * d];
    }
    if (sc.ret_e.ensure((M ? M : 1) * 4) != hipSuccess || sc.ret_peers.ensure((P ? P : 1) * 4) != hipSuccess)
        return fatal_receive(h, "hipMalloc of the returned pairs");
    sc.last_sent = sc.last_recv = 0;
    for (uint32_t d = 0; d < G; ++d)
        if (d != me) {
            sc.last_sent += 4 + (uint64_t)sc.sc[d] * sizeof(wq_msg_rec) + 16 + eb_s[d] + pb_s[d];
            sc.last_recv += 4 + (uint64_t)sc.rc[d] * sizeof(wq_msg_rec) + 16 + eb_r[d] + pb_r[d];
        }
    {
        Xfer x{{sc.own_e.p, sc.own_peers.p}, {eb_s.data(), pb_s.data()}, {sc.ret_e.p, sc.ret_peers.p},
               {eb_r.data(), pb_r.data()}, 2};
        if ((rc = exchange(h, x))) return rc;
    }
    if (late) return late.report(h);
    if (peer_status) return status_error(h, peer_status, peer_from);
    *n_pairs = P;
    if (P > 0xFFFFFFFFull) return set_error(h, WQ_E_CAPACITY, "more than 2^32-1 pairs in one tick");
    // 6. unshard into the caller's CSR, message order
    WQ_ALLOC(h, sc.ret_off, (M ? M : 1) * 4);
    if ((rc = scan_excl(h, sc.tmp, sc.ret_e.as<uint32_t>(), sc.ret_off.as<uint32_t>(), M))) return rc;
    sc.last_M = M;
    sc.last_P = P;
    sc.last_ready = true;
    return copy_out(h, d_offsets, d_peers, d_msgs, capacity);
}

int wq_sharded_route_owner_device(wq_router* h, const double* d_pos, const int64_t* d_keys, const uint32_t* d_world,
                                  const uint32_t* d_sender, const uint8_t* d_repl, size_t n_msgs, wq_owner_view* out) {
    if (int rc = begin_owner_tick(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs, out)) return rc;
    hipStream_t s = h->stream;
    ShardCtx& sc = *h->shard;
    Late late;
    uint64_t R = 0;
    SegBounds seg;
    int rc = shard_exchange_route(h, d_pos, d_keys, d_world, d_sender, d_repl, n_msgs, &R, &seg, &late);
    if (rc) return rc;
    if (late) return late.report(h);  // nothing else is exchanged in this form: report it now
    // the pairs stay here (first option): only this shard's counters are read
    wq_route_counters c{};
    if (R) {
        WQ_HIP(h, hipMemcpyAsync(&c, h->rws.last, sizeof(c), hipMemcpyDeviceToHost, s));
        WQ_HIP(h, hipStreamSynchronize(s));
        if (c.error & 4u) return set_error(h, WQ_E_TIMEOUT, "owner route: look-back spin gave up");
        if (c.error) return set_error(h, WQ_E_CAPACITY, "owner route: more than 2^32-1 pairs");
        if (c.n_pairs > sc.own_cap) {  // the pair buffer was short: offsets are right, route again
            sc.own_cap = c.n_pairs + c.n_pairs / 4 + 4096;
            if (sc.own_cap > 0xFFFFFFFFull) sc.own_cap = 0xFFFFFFFFull;
            WQ_ALLOC(h, sc.own_peers, sc.own_cap * 4);
            if ((rc = launch_route_records(h, sc.recv.as<wq_msg_rec>(), R, sc.own_off.as<uint32_t>(),
                                           sc.own_peers.as<uint32_t>(), nullptr, sc.own_cap)))
                return rc;
        }
    }
    out->recs = sc.recv.as<wq_msg_rec>();
    out->offsets = sc.own_off.as<uint32_t>();
    out->peers = sc.own_peers.as<uint32_t>();
    out->n_recs = R;
    out->n_pairs = R ? c.n_pairs : 0;
    for (uint32_t d = 0; d <= sc.G; ++d) out->seg[d] = seg.b[d];
    return WQ_OK;
}

int wq_sharded_copy_out(wq_router* h, uint32_t* d_offsets, uint32_t* d_peers, uint32_t* d_msgs, size_t capacity) {
    if (!h || !d_offsets || (capacity && !d_peers)) return WQ_E_INVALID;
    if (!h->shard || !h->shard->last_ready) return set_error(h, WQ_E_INVALID, "no sharded tick to copy out");
    WQ_HIP(h, hipSetDevice(h->device));
    return copy_out(h, d_offsets, d_peers, d_msgs, capacity > 0xFFFFFFFFull ? 0xFFFFFFFFull : capacity);
}

}  // extern "C"
