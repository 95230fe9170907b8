// Test-only shim: runs the ingest dispatch's arithmetic (csrc/dispatch_ops.hpp: the classification, the
// granule sums from the class ballots, the scan operator, the ranks and the emit) on the CPU in the
// passes the kernels of csrc/wq_dispatch.hip use — classify block by block and granule by granule,
// the scan with the one block's kDspScanBlock shares (every lane's share combined, the shares scanned,
// the shares walked again), the emit block by block with its granules placed behind the block's base —
// so the result is checked byte for byte against worldql_server_amd/ingest.py (dispatch_np) without a
// GPU (tests/test_ingest_dispatch_cpp_mirror.py). The GPU instance: tests/test_gpu_ingest_dispatch.py.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../worldql_server_amd/csrc/dispatch_ops.hpp"

extern "C" uint32_t wq_test_dispatch_granule() { return wq::kDspGranule; }
extern "C" uint32_t wq_test_dispatch_block() { return wq::kDspBlock; }
extern "C" uint32_t wq_test_dispatch_scan_block() { return wq::kDspScanBlock; }
extern "C" uint32_t wq_test_dispatch_sizes(int which) {
    return which == 0 ? sizeof(wq_dispatch_in) : which == 1 ? sizeof(wq_dispatch_out) : which == 2 ? sizeof(wq_dispatch_run)
                                                                                       : sizeof(wq_dispatch_counters);
}

namespace {

constexpr uint32_t kAbsent = WQ_CLS_COUNT;

// What a wave's ballots give: the class masks of granule [base, base + 64) and its sum.
wq::DspSum granule(const uint8_t* cls, uint64_t n, uint64_t base, const uint32_t* err, uint64_t* m) {
    using namespace wq;
    uint32_t c_of[kDspGranule];
    for (uint32_t c = 0; c < WQ_CLS_COUNT; ++c) m[c] = 0;
    uint32_t any_err = 0;
    for (uint32_t lane = 0; lane < kDspGranule; ++lane) {
        c_of[lane] = base + lane < n ? cls[base + lane] : kAbsent;
        if (c_of[lane] != kAbsent) m[c_of[lane]] |= 1ull << lane;
        if (err && base + lane < n && err[base + lane]) any_err = kDspErrDisagree;
    }
    const uint64_t table = m[WQ_CLS_OP], read = m[WQ_CLS_LOCAL] | m[WQ_CLS_GLOBAL];
    uint64_t inner = 0;
    for (uint32_t lane = 0; lane < kDspGranule; ++lane)
        if (c_of[lane] != kAbsent && dsp_inner_start(table, read, lane, dsp_kind_of(c_of[lane]))) inner |= 1ull << lane;
    return dsp_granule_sum(m, inner, (uint32_t)base, any_err);
}

}  // namespace

// As wq_ingest_dispatch_device, all host memory. Returns 0.
extern "C" int wq_test_ingest_dispatch_host(const wq_dispatch_in* in, uint64_t n, const wq_dispatch_out* out,
                                            wq_dispatch_counters* counters) {
    using namespace wq;
    const uint32_t n_blocks = (uint32_t)((n + kDspBlock - 1) / kDspBlock);
    std::vector<uint8_t> cls(n);       // exactly n: a class too many is a heap overflow
    std::vector<uint32_t> err(n);
    std::vector<DspSum> sums((size_t)n_blocks + 1);
    uint64_t m[WQ_CLS_COUNT];
    // classify
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint64_t b0 = (uint64_t)b * kDspBlock;
        for (uint64_t i = b0; i < b0 + kDspBlock && i < n; ++i) {
            err[i] = 0;
            cls[i] = (uint8_t)dsp_classify(in->instruction[i], in->flags[i], in->world[i], in->sender[i], &err[i]);
            if (out->cls) out->cls[i] = cls[i];
        }
        DspSum gs[kDspGranules];
        for (uint32_t g = 0; g < kDspGranules; ++g) gs[g] = granule(cls.data(), n, b0 + (uint64_t)g * kDspGranule, err.data(), m);
        DspSum s = gs[0];
        for (uint32_t g = 1; g < kDspGranules; ++g) s = dsp_combine(s, gs[g]);
        sums[b] = s;
    }
    // scan: one block of kDspScanBlock lanes
    {
        const uint32_t per = (n_blocks + kDspScanBlock - 1) / kDspScanBlock;
        std::vector<DspSum> sh(kDspScanBlock), nx(kDspScanBlock);
        auto lo_of = [&](uint32_t t) { const uint64_t v = (uint64_t)t * per; return v < n_blocks ? (uint32_t)v : n_blocks; };
        auto hi_of = [&](uint32_t t) { const uint64_t v = (uint64_t)t * per + per; return v < n_blocks ? (uint32_t)v : n_blocks; };
        for (uint32_t t = 0; t < kDspScanBlock; ++t) {
            DspSum acc = dsp_zero();
            for (uint32_t j = lo_of(t); j < hi_of(t); ++j) acc = dsp_combine(acc, sums[j]);
            sh[t] = acc;
        }
        for (uint32_t d = 1; d < kDspScanBlock; d *= 2) {
            for (uint32_t t = 0; t < kDspScanBlock; ++t) nx[t] = t >= d ? dsp_combine(sh[t - d], sh[t]) : sh[t];
            sh.swap(nx);
        }
        for (uint32_t t = 0; t < kDspScanBlock; ++t) {
            DspSum run = t ? sh[t - 1] : dsp_zero();
            for (uint32_t j = lo_of(t); j < hi_of(t); ++j) {
                const DspSum own = sums[j];
                sums[j] = run;
                run = dsp_combine(run, own);
            }
        }
        sums[n_blocks] = sh[kDspScanBlock - 1];
        dsp_finish(sums[n_blocks], n, *out, counters);
    }
    // emit
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint64_t b0 = (uint64_t)b * kDspBlock;
        DspSum gs[kDspGranules];
        for (uint32_t g = 0; g < kDspGranules; ++g) gs[g] = granule(cls.data(), n, b0 + (uint64_t)g * kDspGranule, nullptr, m);
        DspSum run = sums[b];
        for (uint32_t g = 0; g < kDspGranules; ++g) {
            const DspSum own = gs[g];
            gs[g] = run;
            run = dsp_combine(run, own);
        }
        const DspSum total = sums[n_blocks];
        for (uint32_t g = 0; g < kDspGranules; ++g) {
            const uint64_t g0 = b0 + (uint64_t)g * kDspGranule;
            granule(cls.data(), n, g0, nullptr, m);
            const uint64_t table = m[WQ_CLS_OP], read = m[WQ_CLS_LOCAL] | m[WQ_CLS_GLOBAL];
            uint64_t start_mask = 0;
            for (uint32_t lane = 0; lane < kDspGranule && g0 + lane < n; ++lane)
                if (dsp_starts_run(gs[g], table, read, lane, dsp_kind_of(cls[g0 + lane]))) start_mask |= 1ull << lane;
            for (uint32_t lane = 0; lane < kDspGranule && g0 + lane < n; ++lane) {
                uint32_t before[WQ_CLS_COUNT];
                dsp_lane_before(gs[g], m, lane, before);
                dsp_emit(*in, *out, (uint32_t)(g0 + lane), cls[g0 + lane], before, total, (start_mask >> lane) & 1,
                         dsp_lane_run(gs[g], start_mask, lane));
            }
        }
    }
    return 0;
}
