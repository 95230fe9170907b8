// wq_dispatch.hip — the ingest dispatch: a decoded tick split by instruction on the device.
//
// wq_frames_decode_device leaves every frame of a tick in six arrays, whatever its instruction; the
// reference dispatches one message at a time on the host (processing/thread.rs:72-148) and
// processing.SubscriptionProcessor.process_tick restates that as a Python loop. Here one call writes the
// compact inputs of wq_route_tick_device, wq_route_global_device and wq_apply_ops_device, the lists the
// host must see and the table of runs, in arrival order. All arithmetic is dispatch_ops.hpp.
//
//   classify  one lane per frame reads its 10 bytes and writes its class. A wave is a granule of 64
//             frames: ten ballots give its DspSum, and the block's 16 sums are combined in order into
//             one DspSum per 1,024 frames.
//   scan      one block over the block sums: every lane combines a contiguous share, the shares are
//             scanned in LDS, and the share is walked again to leave each block the sum of everything
//             before it. The operator carries counts, run starts and the last effective kind together.
//             Its first lane writes the tick's total, the counters and the closing run.
//   emit      a block rebuilds its granules' ballots from the classes, places them behind its base, and
//             every lane writes its row, list entry, op, stamp or run entry at base + the frames of its
//             class below it.
//
// No lane, wave or block owns a run and none waits for another; there are no atomics. At 10M frames the
// scan reads and writes 9,766 sums of 60 bytes: what the call moves is the rows.
#include "dispatch_ops.hpp"
#include "wq_internal.hpp"

namespace wq {

namespace {

static_assert(sizeof(wq_dispatch_in) == 64, "abi.DispatchIn mirrors this layout");
static_assert(sizeof(wq_dispatch_out) == 120, "abi.DispatchOut mirrors this layout");
static_assert(sizeof(wq_dispatch_run) == 20, "abi.DISPATCH_RUN_DTYPE mirrors this layout");
static_assert(sizeof(wq_dispatch_counters) == 168, "abi.DISPATCH_COUNTERS_DTYPE mirrors this layout");
static_assert(sizeof(wq_op) == 40, "an op is five 8-byte words");
static_assert(kDspGranule == 64, "a granule is one wave64 ballot");

constexpr uint32_t kAbsent = WQ_CLS_COUNT;  // a lane behind the last frame: in no ballot

// The wave's class ballots, and from them the granule's sum (every lane returns it).
__device__ __forceinline__ DspSum granule_sum(uint32_t cls, uint32_t lane, uint32_t base, uint32_t err, uint64_t* m) {
    for (uint32_t c = 0; c < WQ_CLS_COUNT; ++c) m[c] = __ballot(cls == c);
    const uint64_t table = m[WQ_CLS_OP], read = m[WQ_CLS_LOCAL] | m[WQ_CLS_GLOBAL];
    const uint64_t inner = __ballot(cls != kAbsent && dsp_inner_start(table, read, lane, dsp_kind_of(cls)));
    const uint32_t any_err = __ballot(err != 0) ? kDspErrDisagree : 0;
    return dsp_granule_sum(m, inner, base, any_err);
}

__global__ __launch_bounds__(kDspBlock) void k_dispatch_classify(wq_dispatch_in in, uint64_t n, uint8_t* __restrict__ cls_tmp,
                                                                 uint8_t* __restrict__ cls_out,
                                                                 DspSum* __restrict__ sums) {
    __shared__ DspSum gs[kDspGranules];
    const uint64_t i = (uint64_t)blockIdx.x * kDspBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x % kDspGranule, g = threadIdx.x / kDspGranule;
    uint32_t cls = kAbsent, err = 0;
    if (i < n) {
        cls = dsp_classify(in.instruction[i], in.flags[i], in.world[i], in.sender[i], &err);
        cls_tmp[i] = (uint8_t)cls;
        if (cls_out) cls_out[i] = (uint8_t)cls;
    }
    uint64_t m[WQ_CLS_COUNT];
    const DspSum s = granule_sum(cls, lane, (uint32_t)(i - lane), err, m);
    if (lane == 0) gs[g] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        DspSum b = gs[0];
        for (uint32_t k = 1; k < kDspGranules; ++k) b = dsp_combine(b, gs[k]);
        sums[blockIdx.x] = b;
    }
}

// One block. sums[0 .. n_blocks) become exclusive; sums[n_blocks] receives the total.
__global__ __launch_bounds__(kDspScanBlock) void k_dispatch_scan(DspSum* __restrict__ sums, uint32_t n_blocks, uint64_t n,
                                                                 wq_dispatch_out out, wq_dispatch_counters* counters) {
    __shared__ DspSum sh[kDspScanBlock];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_blocks + kDspScanBlock - 1) / kDspScanBlock;
    const uint64_t lo64 = (uint64_t)t * per;
    const uint32_t lo = lo64 < n_blocks ? (uint32_t)lo64 : n_blocks;
    const uint32_t hi = lo64 + per < n_blocks ? (uint32_t)(lo64 + per) : n_blocks;
    DspSum acc = dsp_zero();
    for (uint32_t j = lo; j < hi; ++j) acc = dsp_combine(acc, sums[j]);
    sh[t] = acc;
    __syncthreads();
    for (uint32_t d = 1; d < kDspScanBlock; d *= 2) {
        DspSum v = sh[t];
        if (t >= d) v = dsp_combine(sh[t - d], v);
        __syncthreads();
        sh[t] = v;
        __syncthreads();
    }
    DspSum run = t ? sh[t - 1] : dsp_zero();
    for (uint32_t j = lo; j < hi; ++j) {
        const DspSum own = sums[j];
        sums[j] = run;
        run = dsp_combine(run, own);
    }
    if (t == 0) {
        const DspSum total = sh[kDspScanBlock - 1];
        sums[n_blocks] = total;
        dsp_finish(total, n, out, counters);
    }
}

__global__ __launch_bounds__(kDspBlock) void k_dispatch_emit(wq_dispatch_in in, uint64_t n, const uint8_t* __restrict__ cls_tmp,
                                                             const DspSum* __restrict__ sums, uint32_t n_blocks,
                                                             wq_dispatch_out out) {
    __shared__ DspSum gs[kDspGranules];  // a granule's sum, then the sum of everything before it
    __shared__ DspSum total;
    const uint64_t i = (uint64_t)blockIdx.x * kDspBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x % kDspGranule, g = threadIdx.x / kDspGranule;
    const uint32_t cls = i < n ? cls_tmp[i] : kAbsent;
    uint64_t m[WQ_CLS_COUNT];
    const DspSum s = granule_sum(cls, lane, (uint32_t)(i - lane), 0, m);
    if (lane == 0) gs[g] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        DspSum run = sums[blockIdx.x];
        for (uint32_t k = 0; k < kDspGranules; ++k) {
            const DspSum own = gs[k];
            gs[k] = run;
            run = dsp_combine(run, own);
        }
        total = sums[n_blocks];
    }
    __syncthreads();
    const DspSum gp = gs[g];
    const uint64_t table = m[WQ_CLS_OP], read = m[WQ_CLS_LOCAL] | m[WQ_CLS_GLOBAL];
    const bool starts = cls != kAbsent && dsp_starts_run(gp, table, read, lane, dsp_kind_of(cls));
    const uint64_t start_mask = __ballot(starts);
    if (i >= n) return;
    uint32_t before[WQ_CLS_COUNT];
    dsp_lane_before(gp, m, lane, before);
    dsp_emit(in, out, (uint32_t)i, cls, before, total, starts, dsp_lane_run(gp, start_mask, lane));
}

}  // namespace

void dispatch_release(wq_router* h) {
    h->dsp_cls.release();
    h->dsp_sum.release();
}

// The call on device arrays (the handle's device is current; arguments validated, n_frames < 2^32 - 1).
int launch_ingest_dispatch(wq_router* h, const wq_dispatch_in* in, size_t n_frames, const wq_dispatch_out* out,
                           wq_dispatch_counters* d_counters) {
    hipStream_t s = h->stream;
    const uint32_t n_blocks = (uint32_t)((n_frames + kDspBlock - 1) / kDspBlock);
    WQ_ALLOC(h, h->dsp_cls, n_frames);
    WQ_ALLOC(h, h->dsp_sum, ((size_t)n_blocks + 1) * sizeof(DspSum));
    uint8_t* cls = h->dsp_cls.as<uint8_t>();
    DspSum* sums = h->dsp_sum.as<DspSum>();
    if (n_blocks) {
        hipLaunchKernelGGL(k_dispatch_classify, dim3(n_blocks), dim3(kDspBlock), 0, s, *in, (uint64_t)n_frames, cls,
                           out->cls, sums);
        WQ_HIP(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_dispatch_scan, dim3(1), dim3(kDspScanBlock), 0, s, sums, n_blocks, (uint64_t)n_frames, *out,
                       d_counters);
    WQ_HIP(h, hipGetLastError());
    if (n_blocks) {
        hipLaunchKernelGGL(k_dispatch_emit, dim3(n_blocks), dim3(kDspBlock), 0, s, *in, (uint64_t)n_frames, cls, sums,
                           n_blocks, *out);
        WQ_HIP(h, hipGetLastError());
    }
    return WQ_OK;
}

}  // namespace wq
