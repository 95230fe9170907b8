// wq_recdispatch.hip — the record dispatch: a tick's record frames to store ops and queries on the device.
//
// wq_ingest_dispatch_device lists the RecordCreate / RecordRead / RecordDelete frames and stops there; the
// host restates the reference's handlers as a loop over every record (records.RecordProcessor.process).
// Here one call writes the inputs of wq_records_apply_device and wq_records_read_device and the table of
// runs, in arrival order. All arithmetic is recdispatch_ops.hpp.
//
//   frames   one lane per listed frame: its class, its `after`, where its records vector lies and how many
//            records it holds; wave ballots add the class counts
//   scan     the exclusive prefix of the record counts: the ordinal space of the tick's records
//   records  element-parallel: a wave per granule of 64 ordinals on a grid-stride loop (the total is read
//            on the device); every lane finds its frame (a search narrowed to the frames the granule
//            touches) and walks one record; three ballots are the granule's flag words
//   scan     the exclusive prefixes of the granules' accepted / deferred counts and of their creates
//   scan     over the listed frames: each frame's sum comes from the two prefixes above as the scan reads
//            it; the operator carries rows, deferred entries, run starts and the last barrier kind
//   emit     a wave per granule with a flag set walks its accepted records again and stores the ops as one
//            contiguous run at the granule's prefix; one lane per listed frame writes its query row, its
//            deferred entry and its run entry; the lane behind the frames the closing run and the counters
//
// No lane, wave or block owns a frame's records: a frame of any size is spread over ceil(count / 64)
// granules. Placement comes from the prefix sums alone, so the output is the same bytes every time; the
// only atomics are integer adds and ORs into the counters.
#include "recdispatch_ops.hpp"
#include "send_rows.hpp"

namespace wq {

namespace {

static_assert(sizeof(wq_recdisp_in) == 104, "abi.RecDispatchIn mirrors this layout");
static_assert(sizeof(wq_recdisp_out) == 88, "abi.RecDispatchOut mirrors this layout");
static_assert(sizeof(wq_recdisp_run) == 16 && sizeof(wq_recdisp_defer) == 8 && sizeof(wq_rec_op_ref) == 32,
              "abi.RECDISP_RUN_DTYPE, RECDISP_DEFER_DTYPE and REC_OP_REF_DTYPE mirror these layouts");
static_assert(sizeof(wq_recdisp_counters) == 152, "abi.RECDISP_COUNTERS_DTYPE mirrors this layout");
static_assert(sizeof(wq_rec_op) == 64, "an op is eight 8-byte words");
static_assert(kRdGranule == 64, "a granule is one wave64 ballot");

constexpr int kRdWaves = kBlock / 64;
constexpr unsigned kRdMaxBlocks = 4096;  // 16 blocks of 256 per CU: the persistent grids' size
constexpr uint32_t kRdDead = 0xFFu;      // the status of a lane behind the last ordinal: in no ballot

__device__ __forceinline__ void add64(uint64_t* p, uint64_t v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}
__device__ __forceinline__ void or64(uint64_t* p, uint64_t v) {
    if (v) atomicOr(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

__global__ __launch_bounds__(kBlock) void k_recdisp_frames(wq_recdisp_in in, RdWs ws, uint8_t* __restrict__ cls_out,
                                                           wq_recdisp_counters* ctrl) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t cls = WQ_RCLS_COUNT, err = 0;
    if (j < in.n_db) {
        const RdFrameRes r = rd_frame_eval(in, j);
        cls = r.cls, err = r.err;
        ws.cls[j] = (uint8_t)cls;
        if (cls_out) cls_out[j] = (uint8_t)cls;
        ws.cnt[j] = r.count;
        ws.vec[j] = r.vec;
        ws.after[j] = r.after;
    }
    uint64_t m[WQ_RCLS_COUNT];
    for (uint32_t c = 0; c < WQ_RCLS_COUNT; ++c) m[c] = __ballot(cls == c);
    const uint64_t e0 = __ballot((err & kRdErrWalk) != 0), e1 = __ballot((err & kRdErrList) != 0);
    if ((threadIdx.x & 63u) == 0) {
        for (uint32_t c = 0; c < WQ_RCLS_COUNT; ++c) add64(&ctrl->n_skip + c, dsp_popc(m[c]));
        or64(&ctrl->error, (e0 ? kRdErrWalk : 0u) | (e1 ? kRdErrList : 0u));
    }
}

// The listed entries [rlo, rhi] that the granule starting at ordinal q0 touches (T: the examined total,
// q0 < T): lane 0 searches the first ordinal's entry and lane 63 the last one's, as wq_csr_diff.hip.
__device__ __forceinline__ void granule_frames(const uint64_t* __restrict__ pre, uint32_t n_db, uint32_t T, uint32_t q0,
                                               uint32_t lane, uint32_t& rlo, uint32_t& rhi) {
    const uint32_t r = rd_frame_of(pre, 0, n_db - 1, lane == 63 ? rd_granule_last(T, q0) : q0);
    rlo = __shfl(r, 0);
    rhi = __shfl(r, 63);
}

__global__ __launch_bounds__(kBlock) void k_recdisp_records(wq_recdisp_in in, RdWs ws, DecTables tables, RecCfg cfg,
                                                            wq_recdisp_counters* ctrl) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * kRdWaves + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * kRdWaves;
    const uint32_t n_db = (uint32_t)in.n_db;
    const uint32_t T = rd_examined(ws.pre[n_db], in.max_records);
    const uint32_t nG = T / kRdGranule + (T % kRdGranule ? 1u : 0u);
    for (uint32_t g = wave; g < nG; g += n_waves) {
        const uint32_t q0 = g * kRdGranule, q = q0 + lane;
        uint32_t rlo, rhi, status = kRdDead;
        bool create = false;
        granule_frames(ws.pre, n_db, T, q0, lane, rlo, rhi);
        if (q < T) {
            uint32_t j, f, r;
            status = rd_ordinal_record(in, ws, tables, cfg, rlo, rhi, q, &j, &f, &r).status;
            create = status == kRdAccept && in.msg[f].instruction == kInsRecordCreate;
        }
        const uint64_t acc = __ballot(status == kRdAccept), def = __ballot(status == kRdDefer), crw = __ballot(create);
        uint64_t drop[4];
        for (uint32_t k = 0; k < 4; ++k) drop[k] = __ballot(status == k);
        if (lane == 0) {
            ws.words[(uint64_t)kRdWords * g] = acc;
            ws.words[(uint64_t)kRdWords * g + 1] = def;
            ws.words[(uint64_t)kRdWords * g + 2] = crw;
            add64(&ctrl->n_creates, dsp_popc(crw));
            add64(&ctrl->n_deletes, dsp_popc(acc & ~crw));
            for (uint32_t k = 0; k < 4; ++k) add64(&ctrl->n_drop_walk + k, dsp_popc(drop[k]));
            add64(&ctrl->n_deferred_records, dsp_popc(def));
            or64(&ctrl->error, drop[kRdFail] ? kRdErrWalk : 0u);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_recdisp_emit(wq_recdisp_in in, RdWs ws, DecTables tables, RecCfg cfg,
                                                         wq_recdisp_out out, wq_recdisp_counters* ctrl) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * kRdWaves + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * kRdWaves;
    const uint32_t n_db = (uint32_t)in.n_db;
    const uint32_t T = rd_examined(ws.pre[n_db], in.max_records);
    const uint32_t nG = T / kRdGranule + (T % kRdGranule ? 1u : 0u);
    for (uint32_t g = wave; g < nG; g += n_waves) {
        const uint64_t acc = ws.words[(uint64_t)kRdWords * g], def = ws.words[(uint64_t)kRdWords * g + 1];
        if (!(acc | def)) continue;  // wave-uniform
        uint32_t rlo, rhi;
        granule_frames(ws.pre, n_db, T, g * kRdGranule, lane, rlo, rhi);
        rd_emit_ordinal(in, ws, tables, cfg, out, g, lane, rlo, rhi);
    }
    // the listed frames' own rows, and behind them the closing run and the counters
    const RdFrameTerm own{ws, in.db_src, in.n_db, in.max_records};
    const uint64_t n_threads = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i <= in.n_db; i += n_threads) {
        if (i == in.n_db) {
            rd_finish(in, out, ws.ex[i], ws.pre[i], ctrl);
            break;
        }
        const uint32_t cls = ws.cls[i];
        if (cls != WQ_RCLS_SKIP) rd_emit_frame(in, out, in.db_src ? in.db_src[i] : (uint32_t)i, cls, ws.after[i], ws.ex[i], own(i));
    }
}

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

void recdispatch_release(wq_router* h) {
    h->rdp.release();
    h->rdp_ctrl.release();
}

// The call on device arrays (the handle's device is current; arguments validated: n_db < 2^32 - 1,
// max_records < 2^32 - 64, a record store is open).
int launch_records_dispatch(wq_router* h, const wq_recdisp_in* in, const wq_recdisp_out* out,
                            wq_recdisp_counters* d_counters) {
    hipStream_t s = h->stream;
    const size_t n = in->n_db, nG = in->max_records / kRdGranule + 1;
    RecCfg cfg;
    if (!records_config(h, &cfg)) return set_error(h, WQ_E_INVALID, "records_dispatch: no record store is open");
    DecTables tables;
    ingest_tables(h, &tables);
    // one buffer, every array at 8-byte alignment
    const size_t o_pre = 0, o_after = o_pre + (n + 1) * 8, o_ex = o_after + n * 8, o_cnt = o_ex + (n + 1) * sizeof(RdSum),
                 o_vec = o_cnt + align8(n * 4), o_cls = o_vec + align8(n * 4), o_words = o_cls + align8(n),
                 o_base = o_words + nG * kRdWords * 8, o_cbase = o_base + nG * 8, total = o_cbase + nG * 8;
    WQ_ALLOC(h, h->rdp, total);
    WQ_ALLOC(h, h->rdp_ctrl, sizeof(wq_recdisp_counters));
    uint8_t* p = h->rdp.as<uint8_t>();
    const RdWs ws{reinterpret_cast<uint64_t*>(p + o_pre),   reinterpret_cast<int64_t*>(p + o_after),
                  reinterpret_cast<RdSum*>(p + o_ex),       reinterpret_cast<uint32_t*>(p + o_cnt),
                  reinterpret_cast<uint32_t*>(p + o_vec),   p + o_cls,
                  reinterpret_cast<uint64_t*>(p + o_words), reinterpret_cast<uint64_t*>(p + o_base),
                  reinterpret_cast<uint64_t*>(p + o_cbase)};
    wq_recdisp_counters* ctrl = h->rdp_ctrl.as<wq_recdisp_counters>();
    WQ_HIP(h, hipMemsetAsync(ctrl, 0, sizeof(wq_recdisp_counters), s));
    if (n) {
        hipLaunchKernelGGL(k_recdisp_frames, dim3(grid_for(n)), dim3(kBlock), 0, s, *in, ws, out->cls, ctrl);
        WQ_HIP(h, hipGetLastError());
    }
    if (int rc = scan_terms(h, RdCountTerm{ws.cnt, n}, ws.pre, n + 1)) return rc;
    const unsigned grid_g = std::min<unsigned>(kRdMaxBlocks, (unsigned)((nG + kRdWaves - 1) / kRdWaves));
    if (n) {
        hipLaunchKernelGGL(k_recdisp_records, dim3(grid_g), dim3(kBlock), 0, s, *in, ws, tables, cfg, ctrl);
        WQ_HIP(h, hipGetLastError());
    }
    if (int rc = scan_terms(h, RdGranuleTerm{ws.words, ws.pre + n, in->max_records, false}, ws.base, nG)) return rc;
    if (int rc = scan_terms(h, RdGranuleTerm{ws.words, ws.pre + n, in->max_records, true}, ws.cbase, nG)) return rc;
    if (int rc = scan_terms(h, RdFrameTerm{ws, in->db_src, n, in->max_records}, ws.ex, rd_zero(), n + 1, RdCombine()))
        return rc;
    const unsigned grid_e = std::min<unsigned>(kRdMaxBlocks, std::max(grid_g, grid_for((uint64_t)n + 1)));
    hipLaunchKernelGGL(k_recdisp_emit, dim3(grid_e), dim3(kBlock), 0, s, *in, ws, tables, cfg, *out, ctrl);
    WQ_HIP(h, hipGetLastError());
    if (d_counters)
        WQ_HIP(h, hipMemcpyAsync(d_counters, ctrl, sizeof(wq_recdisp_counters), hipMemcpyDeviceToDevice, s));
    return WQ_OK;
}

}  // namespace wq
