// wq_follow.hip — follow moving peers: the subscription ops of "peer i is now in world w at p",
// generated on the GPU (include/wq_router.h wq_follow_*).
//
// The handle keeps, per peer id, the world and position it was last followed at. A follow call
// turns that state and the caller's new arrays into UNSUBSCRIBE ops for the cubes a peer's
// neighbourhood left and SUBSCRIBE ops for the cubes it entered, and hands them to the table:
//   count   one lane per peer: the 2r+1 quantised values per axis of the old and of the new
//           position, per axis the "first offset with this value" and "the other list has this
//           value too" bit masks (one packed u64 per peer), and the closed-form op count
//           |O| - prod |O_ax ∩ N_ax| (+ the same for N); block totals by four atomics per block
//   scan    exclusive prefix of the counts (table_prims.hpp scan_u32)
//   --      the totals come to the host (the call's only read): the op buffer gets its exact size
//   emit    one block per 256 peers: lanes map to OPS, not peers (a search in the tile's prefix in
//           LDS), decode (kind, offset) from the op's ordinal and the masks, stage 256 ops in LDS
//           and write them as consecutive 8-byte words — a wave's stores cover one contiguous
//           range whatever the peers' counts are; the same block then stores the new follow state
//   apply   table_apply_segment(on_device) / multi_apply_ops_device, unchanged
// The quantiser runs once per value, in the count pass; the emit pass only adds offsets.
#include <algorithm>

#include "follow_ops.hpp"
#include "table_prims.hpp"

#pragma clang fp contract(off)

namespace wq {

namespace {

constexpr int kTile = 256;             // peers per block, and ops per staging round
constexpr uint32_t kMaxReach = 2;
constexpr int kOpWords = sizeof(wq_op) / 8;  // 5 u64 words per op
static_assert(sizeof(wq_op) == 40, "wq_op is 40 bytes");

// Totals of one call (device, then pinned host memory).
struct FollowTotals {
    unsigned long long n_unsub, n_sub, n_new, n_old;  // ops; peers followed after / before, among [0, n)
};

template <int R>
__global__ __launch_bounds__(kTile) void k_follow_count(const uint32_t* __restrict__ new_w,
                                                        const double* __restrict__ new_p,
                                                        const uint32_t* __restrict__ old_w,
                                                        const double* __restrict__ old_p, uint32_t n, double sf,
                                                        int64_t si, uint32_t* __restrict__ cnt,
                                                        uint64_t* __restrict__ mask, unsigned long long* tot) {
    __shared__ uint32_t part[kTile / 64][4];
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    uint32_t v[4] = {0, 0, 0, 0};  // unsubscribes, subscribes, followed after, followed before
    if (i < n) {
        const uint32_t ow = old_w[i], nw = new_w[i];
        const double po[3] = {old_p[3ull * i], old_p[3ull * i + 1], old_p[3ull * i + 2]};
        const double pn[3] = {new_p[3ull * i], new_p[3ull * i + 1], new_p[3ull * i + 2]};
        const uint64_t m = peer_masks<R>(ow, po, nw, pn, sf, si);
        v[0] = side_count(m, 0);
        v[1] = side_count(m, kFollowNewShift);
        v[2] = nw != kWorldEmpty;
        v[3] = ow != kWorldEmpty;
        mask[i] = m;
        cnt[i] = v[0] + v[1];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) part[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long s = 0;
        for (int w = 0; w < kTile / 64; ++w) s += part[w][threadIdx.x];
        if (s) atomicAdd(tot + threadIdx.x, s);  // integer sums: the order does not matter
    }
}

// fol_w / fol_p: the follow state, read (old) and then rewritten (new) by the block that owns the
// peer. off[i]: first op of peer i; total: the call's op count.
template <int R>
__global__ __launch_bounds__(kTile) void k_follow_emit(const uint32_t* __restrict__ new_w,
                                                       const double* __restrict__ new_p, uint32_t* fol_w,
                                                       double* fol_p, uint32_t n, double sf,
                                                       const uint32_t* __restrict__ off,
                                                       const uint64_t* __restrict__ mask, uint32_t total,
                                                       uint64_t* __restrict__ ops) {
    __shared__ uint32_t s_off[kTile];
    __shared__ uint64_t s_mask[kTile];
    __shared__ uint32_t s_w[2][kTile];
    __shared__ double s_p[2][3][kTile];
    __shared__ uint64_t s_ops[kTile * kOpWords];
    const uint32_t t = threadIdx.x;
    const uint32_t base = blockIdx.x * kTile;
    const uint32_t i = base + t;
    if (i < n) {
        s_off[t] = off[i];
        s_mask[t] = mask[i];
        const uint32_t nw = new_w[i];
        s_w[0][t] = fol_w[i];
        s_w[1][t] = nw;
        fol_w[i] = nw;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double np_ = new_p[3ull * i + ax];
            s_p[0][ax][t] = fol_p[3ull * i + ax];
            s_p[1][ax][t] = np_;
            fol_p[3ull * i + ax] = np_;
        }
    } else {
        s_off[t] = total;
        s_mask[t] = 0;
    }
    __syncthreads();
    const uint32_t begin = s_off[0];
    const uint32_t end = (uint64_t)base + kTile < n ? off[base + kTile] : total;
    for (uint32_t c = begin; c < end; c += kTile) {
        const uint32_t g = c + t;
        if (g < end) {
            // the peer of op g: the last p with s_off[p] <= g (peers without ops share an offset)
            uint32_t lo = 0, hi = kTile;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_off[mid] <= g) lo = mid;
                else hi = mid;
            }
            const uint32_t p = lo;
            const double po[3] = {s_p[0][0][p], s_p[0][1][p], s_p[0][2][p]};
            const double pn[3] = {s_p[1][0][p], s_p[1][1][p], s_p[1][2][p]};
            uint64_t o[kOpWords];
            make_op<R>(s_mask[p], g - s_off[p], base + p, s_w[0][p], po, s_w[1][p], pn, sf, o);
#pragma unroll
            for (int w = 0; w < kOpWords; ++w) s_ops[t * kOpWords + w] = o[w];
        }
        __syncthreads();
        const uint32_t words = (end - c < (uint32_t)kTile ? end - c : (uint32_t)kTile) * kOpWords;
        uint64_t* dst = ops + (uint64_t)c * kOpWords;
        for (uint32_t w = t; w < words; w += kTile) dst[w] = s_ops[w];
        __syncthreads();
    }
}

// One interval of wq_profile_read (an unphased launch): the generator's kernels.
int prof_mark(wq_router* h, bool start) {
    ProfileEvents& pr = h->prof;
    if (!pr.enabled) return WQ_OK;
    if (start) {
        if (pr.used == pr.start.size()) {
            hipEvent_t ev[4];
            for (auto& e : ev) WQ_HIP(h, hipEventCreate(&e));
            pr.start.push_back(ev[0]);
            pr.stop.push_back(ev[1]);
            pr.mid1.push_back(ev[2]);
            pr.mid2.push_back(ev[3]);
            pr.phased.push_back(0);
        }
        pr.phased[pr.used] = 0;
        WQ_HIP(h, hipEventRecord(pr.start[pr.used], h->stream));
    } else {
        WQ_HIP(h, hipEventRecord(pr.stop[pr.used], h->stream));
        pr.used++;
    }
    return WQ_OK;
}

// The follow state covers at least n peers (new ones not followed); contents are kept.
int grow_state(wq_router* h, size_t n) {
    if (n <= h->fol_cap) return WQ_OK;
    const size_t cap = std::max<size_t>(n + n / 4, 1024);
    DevBuf w, p;
    hipError_t e = w.ensure(cap * 4);
    if (e == hipSuccess) e = p.ensure(cap * 24);
    if (e != hipSuccess) {
        w.release();
        p.release();
        return set_error(h, WQ_E_OOM, "hipMalloc follow state", e);
    }
    hipStream_t s = h->stream;
    hipError_t c = hipMemsetAsync(w.p, 0xFF, w.bytes, s);  // WQ_WORLD_INVALID: not followed
    if (c == hipSuccess) c = hipMemsetAsync(p.p, 0, p.bytes, s);
    if (c == hipSuccess && h->fol_cap) {
        c = hipMemcpyAsync(w.p, h->fol_world.p, h->fol_cap * 4, hipMemcpyDeviceToDevice, s);
        if (c == hipSuccess) c = hipMemcpyAsync(p.p, h->fol_pos.p, h->fol_cap * 24, hipMemcpyDeviceToDevice, s);
    }
    if (c == hipSuccess) c = hipStreamSynchronize(s);
    if (c != hipSuccess) {
        w.release();
        p.release();
        return set_error(h, WQ_E_HIP, "follow state copy", c);
    }
    h->fol_world.release();
    h->fol_pos.release();
    h->fol_world = w;
    h->fol_pos = p;
    h->fol_cap = cap;
    return WQ_OK;
}

template <int R>
void launch_count(wq_router* h, const uint32_t* d_world, const double* d_pos, uint32_t n) {
    hipLaunchKernelGGL(k_follow_count<R>, dim3(grid_for(n)), dim3(kTile), 0, h->stream, d_world, d_pos,
                       h->fol_world.as<uint32_t>(), h->fol_pos.as<double>(), n, (double)h->cube_size,
                       (int64_t)h->cube_size, h->fol_cnt.as<uint32_t>(), h->fol_mask.as<uint64_t>(),
                       h->fol_tot.as<unsigned long long>());
}

template <int R>
void launch_emit(wq_router* h, const uint32_t* d_world, const double* d_pos, uint32_t n, uint32_t total) {
    hipLaunchKernelGGL(k_follow_emit<R>, dim3(grid_for(n)), dim3(kTile), 0, h->stream, d_world, d_pos,
                       h->fol_world.as<uint32_t>(), h->fol_pos.as<double>(), n, (double)h->cube_size,
                       h->fol_off.as<uint32_t>(), h->fol_mask.as<uint64_t>(), total, h->fol_ops.as<uint64_t>());
}

// The call on device arrays (the handle's device is current).
int follow_device(wq_router* h, const uint32_t* d_world, const double* d_pos, size_t n, wq_follow_result* out) {
    hipStream_t s = h->stream;
    // the previous batch may still have to be re-applied from the op buffer this call rewrites
    if (!h->multi)
        if (int rc = table_resolve(h, true)) return rc;
    h->fol_n_ops = 0;
    if (out) *out = wq_follow_result{0, 0, h->fol_n};
    if (n == 0) return WQ_OK;
    if (int rc = grow_state(h, n)) return rc;
    h->fol_len = std::max<uint64_t>(h->fol_len, n);
    WQ_ALLOC(h, h->fol_cnt, n * 4);
    WQ_ALLOC(h, h->fol_off, n * 4);
    WQ_ALLOC(h, h->fol_mask, n * 8);
    WQ_ALLOC(h, h->fol_tot, sizeof(FollowTotals));
    if (!h->fol_pinned) WQ_HIP(h, hipHostMalloc(&h->fol_pinned, sizeof(FollowTotals), hipHostMallocDefault));
    WQ_HIP(h, hipMemsetAsync(h->fol_tot.p, 0, sizeof(FollowTotals), s));
    const uint32_t N = (uint32_t)n;
    if (int rc = prof_mark(h, true)) return rc;
    switch (h->fol_reach) {
        case 0: launch_count<1>(h, d_world, d_pos, N); break;
        case 1: launch_count<3>(h, d_world, d_pos, N); break;
        default: launch_count<5>(h, d_world, d_pos, N); break;
    }
    WQ_HIP(h, hipGetLastError());
    if (int rc = scan_u32(h, h->fol_cnt.as<uint32_t>(), h->fol_off.as<uint32_t>(), n, false)) return rc;
    if (int rc = prof_mark(h, false)) return rc;
    // the call's only host read: op totals (the buffer's exact size) and the followed counts
    FollowTotals* tot = static_cast<FollowTotals*>(h->fol_pinned);
    WQ_HIP(h, hipMemcpyAsync(tot, h->fol_tot.p, sizeof(FollowTotals), hipMemcpyDeviceToHost, s));
    WQ_HIP(h, hipStreamSynchronize(s));
    const uint64_t n_ops = tot->n_unsub + tot->n_sub;
    if (n_ops > 0xFFFFFFFFull) return set_error(h, WQ_E_CAPACITY, "more than 2^32-1 follow ops in one call");
    WQ_ALLOC(h, h->fol_ops, (n_ops ? n_ops : 1) * sizeof(wq_op));
    // nothing has changed so far; from here on the state is the new one
    if (int rc = prof_mark(h, true)) return rc;
    switch (h->fol_reach) {
        case 0: launch_emit<1>(h, d_world, d_pos, N, (uint32_t)n_ops); break;
        case 1: launch_emit<3>(h, d_world, d_pos, N, (uint32_t)n_ops); break;
        default: launch_emit<5>(h, d_world, d_pos, N, (uint32_t)n_ops); break;
    }
    WQ_HIP(h, hipGetLastError());
    if (int rc = prof_mark(h, false)) return rc;
    h->fol_n = h->fol_n + tot->n_new - tot->n_old;
    h->fol_n_ops = n_ops;
    if (out) *out = wq_follow_result{tot->n_unsub, tot->n_sub, h->fol_n};
    if (n_ops == 0) return WQ_OK;
    if (h->multi) return multi_apply_ops_device(h, h->fol_ops.as<wq_op>(), n_ops);
    return table_apply_segment(h, h->fol_ops.as<wq_op>(), n_ops, true);
}

}  // namespace

void follow_release(wq_router* h) {
    for (DevBuf* b : {&h->fol_world, &h->fol_pos, &h->fol_cnt, &h->fol_off, &h->fol_mask, &h->fol_tot, &h->fol_ops,
                      &h->fol_in})
        b->release();
    if (h->fol_pinned) (void)hipHostFree(h->fol_pinned);
    h->fol_pinned = nullptr;
}

}  // namespace wq

using namespace wq;

extern "C" {

int wq_follow_set_reach(wq_router* h, uint32_t reach) {
    if (!h) return WQ_E_INVALID;
    if (reach > kMaxReach) return set_error(h, WQ_E_INVALID, "follow reach must be 0, 1 or 2");
    if (h->fol_n) return set_error(h, WQ_E_INVALID, "follow reach can only change while no peer is followed");
    h->fol_reach = reach;
    return WQ_OK;
}

int wq_follow_reset(wq_router* h) {
    if (!h) return WQ_E_INVALID;
    WQ_HIP(h, hipSetDevice(h->device));
    if (h->fol_cap) WQ_HIP(h, hipMemsetAsync(h->fol_world.p, 0xFF, h->fol_cap * 4, h->stream));
    h->fol_n = 0;
    h->fol_len = 0;
    return WQ_OK;
}

int wq_follow_state_read(wq_router* h, uint32_t* world, double* pos, size_t capacity, size_t* n) {
    if (!h || !n || (capacity && (!world || !pos))) return WQ_E_INVALID;
    *n = h->fol_len;
    const size_t m = std::min<size_t>(capacity, h->fol_len);
    if (m) {
        WQ_HIP(h, hipSetDevice(h->device));
        WQ_HIP(h, hipMemcpyAsync(world, h->fol_world.p, m * 4, hipMemcpyDeviceToHost, h->stream));
        WQ_HIP(h, hipMemcpyAsync(pos, h->fol_pos.p, m * 24, hipMemcpyDeviceToHost, h->stream));
        WQ_HIP(h, hipStreamSynchronize(h->stream));
        // the position words of a peer that is not followed hold whatever it was last followed at
        for (size_t i = 0; i < m; ++i)
            if (world[i] == WQ_WORLD_INVALID) pos[3 * i] = pos[3 * i + 1] = pos[3 * i + 2] = 0.0;
    }
    if (h->fol_len > capacity)
        return set_error(h, WQ_E_CAPACITY, "follow state capacity too small (required size in *n)");
    return WQ_OK;
}

int wq_follow_state_load(wq_router* h, const uint32_t* world, const double* pos, size_t n) {
    if (!h || (n && (!world || !pos))) return WQ_E_INVALID;
    if (n >= 0xFFFFFFFFull) return set_error(h, WQ_E_INVALID, "peer ids are below 2^32 - 1");
    if (h->fol_n) return set_error(h, WQ_E_INVALID, "a follow state can only be loaded while no peer is followed");
    WQ_HIP(h, hipSetDevice(h->device));
    // a pending batch may still be re-applied from the op buffer of the follow call that made it
    if (!h->multi)
        if (int rc = table_resolve(h, true)) return rc;
    if (int rc = grow_state(h, n)) return rc;
    if (h->fol_cap) WQ_HIP(h, hipMemsetAsync(h->fol_world.p, 0xFF, h->fol_cap * 4, h->stream));
    uint64_t followed = 0;
    if (n) {
        WQ_HIP(h, hipMemcpyAsync(h->fol_world.p, world, n * 4, hipMemcpyHostToDevice, h->stream));
        WQ_HIP(h, hipMemcpyAsync(h->fol_pos.p, pos, n * 24, hipMemcpyHostToDevice, h->stream));
        for (size_t i = 0; i < n; ++i) followed += world[i] != WQ_WORLD_INVALID;
    }
    WQ_HIP(h, hipStreamSynchronize(h->stream));
    h->fol_n = followed;
    h->fol_len = n;
    return WQ_OK;
}

int wq_follow_peers_device(wq_router* h, const uint32_t* d_world, const double* d_pos, size_t n,
                           wq_follow_result* out) {
    if (!h || (n && (!d_world || !d_pos))) return WQ_E_INVALID;
    if (n >= 0xFFFFFFFFull) return set_error(h, WQ_E_INVALID, "peer ids are below 2^32 - 1");
    WQ_HIP(h, hipSetDevice(h->device));
    return follow_device(h, d_world, d_pos, n, out);
}

int wq_follow_peers(wq_router* h, const uint32_t* world, const double* pos, size_t n, wq_follow_result* out) {
    if (!h || (n && (!world || !pos))) return WQ_E_INVALID;
    if (n >= 0xFFFFFFFFull) return set_error(h, WQ_E_INVALID, "peer ids are below 2^32 - 1");
    WQ_HIP(h, hipSetDevice(h->device));
    const size_t o_w = (n * 24 + 255) & ~size_t(255);
    if (n) {
        // the staging is its own buffer: a multi-GPU handle's apply reuses the shared scratch
        WQ_ALLOC(h, h->fol_in, o_w + n * 4);
        WQ_HIP(h, hipMemcpyAsync(h->fol_in.p, pos, n * 24, hipMemcpyHostToDevice, h->stream));
        WQ_HIP(h, hipMemcpyAsync(h->fol_in.as<char>() + o_w, world, n * 4, hipMemcpyHostToDevice, h->stream));
    }
    int rc = follow_device(h, n ? reinterpret_cast<const uint32_t*>(h->fol_in.as<char>() + o_w) : nullptr,
                           n ? h->fol_in.as<double>() : nullptr, n, out);
    if (rc) return rc;
    // synchronous: the batch is folded in (re-applied through the rebuild if the device could not
    // apply it) before the call returns
    if (!h->multi && (rc = table_resolve(h, true))) return rc;
    WQ_HIP(h, hipStreamSynchronize(h->stream));
    return WQ_OK;
}

int wq_follow_last_ops(wq_router* h, const wq_op** d_ops, size_t* n) {
    if (!h || !d_ops || !n) return WQ_E_INVALID;
    *d_ops = h->fol_n_ops ? h->fol_ops.as<wq_op>() : nullptr;
    *n = h->fol_n_ops;
    return WQ_OK;
}

int wq_follow_read_ops(wq_router* h, wq_op* out, size_t capacity, size_t* n) {
    if (!h || !n || (capacity && !out)) return WQ_E_INVALID;
    *n = h->fol_n_ops;
    if (h->fol_n_ops > capacity) return set_error(h, WQ_E_CAPACITY, "follow op capacity too small (required size in *n)");
    if (!h->fol_n_ops) return WQ_OK;
    WQ_HIP(h, hipSetDevice(h->device));
    WQ_HIP(h, hipMemcpyAsync(out, h->fol_ops.p, h->fol_n_ops * sizeof(wq_op), hipMemcpyDeviceToHost, h->stream));
    WQ_HIP(h, hipStreamSynchronize(h->stream));
    return WQ_OK;
}

}  // extern "C"
