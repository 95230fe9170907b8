// Test-only shim: runs the ingest leaves' arithmetic (csrc/leave_ops.hpp) on the CPU in the passes the
// kernels of csrc/wq_leave.hip use — the listed ids ORed into their bitmap, the flags granule by granule
// over the reserved room with their ballot words, the scan of the words, the decision, the apply lane by
// lane in the grid's order (a leaver's rows, bit, free-list entry and stamp; a kept entry's move and clock),
// the copy back with the live count, the free list's tail — so the result is checked byte for byte against
// worldql_server_amd/ingest.py (leave_peers_np) without a GPU (tests/test_ingest_leave_cpp_mirror.py). The
// GPU instance: tests/test_gpu_ingest_leave.py.
//
// The table arrives as uuid bytes with `cap` slots; the working arrays here have exactly the sizes the
// device call allocates plus eight guard entries each, which must come back untouched (return 2).
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../worldql_server_amd/csrc/leave_ops.hpp"

extern "C" uint32_t wq_test_leave_sizes(int which) {
    return which == 0 ? sizeof(wq_leave_in) : which == 1 ? sizeof(wq_leave_out) : which == 2 ? sizeof(wq_leave_counters)
                                                                                             : sizeof(wq::LvCtrl);
}

// Character k of the text of the uuid whose 16 bytes are given.
extern "C" uint8_t wq_test_leave_text_char(const uint8_t* uuid, uint32_t k) {
    return wq::lv_text_char(wq::jn_be64(uuid), wq::jn_be64(uuid + 8), k);
}

namespace {

constexpr size_t kGuard = 8;
constexpr uint64_t kGuard64 = 0xC5C5C5C5C5C5C5C5ull;
constexpr uint32_t kGuard32 = 0xC5C5C5C5u;

template <typename T>
std::vector<T> guarded(size_t n, T fill) {
    return std::vector<T>(n + kGuard, fill);
}
template <typename T>
bool intact(const std::vector<T>& v, size_t n, T fill) {
    for (size_t i = n; i < v.size(); ++i)
        if (v[i] != fill) return false;
    return true;
}

}  // namespace

// As wq_ingest_leave_device, all host memory; the table as uuids / ids with cap slots and *live entries.
// Returns 0, or 2 when a guard entry was written.
extern "C" int wq_test_ingest_leave_host(const wq_leave_in* in, const wq_leave_out* out, wq_leave_counters* counters,
                                         uint8_t* table_uuids, uint32_t* table_ids, uint32_t* live_word, uint32_t cap,
                                         int reserved) {
    using namespace wq;
    LvCtrl ctrl;
    memset(&ctrl, 0, sizeof(ctrl));
    const size_t n_words = ((size_t)in->n_ids + 31) / 32;
    if (out->gone_bits) memset(out->gone_bits, 0, n_words * 4);
    if (!reserved) {
        lv_no_table(&ctrl, *in);
        if (counters) *counters = ctrl.c;
        return 0;
    }
    auto hi = guarded<uint64_t>(cap, kGuard64), lo = hi, ohi = hi, olo = hi;
    auto id = guarded<uint32_t>(cap, kGuard32), oid = id;
    for (uint32_t e = 0; e < *live_word; ++e)
        hi[e] = jn_be64(table_uuids + 16 * (size_t)e), lo[e] = jn_be64(table_uuids + 16 * (size_t)e + 8), id[e] = table_ids[e];
    const JnTable t{hi.data(), lo.data(), id.data(), live_word, cap};
    const size_t nG = ((size_t)cap + kJnGranule - 1) / kJnGranule;
    auto words = guarded<uint64_t>(nG, kGuard64);
    auto base = guarded<uint32_t>(nG + 1, kGuard32), listed = guarded<uint32_t>(n_words, kGuard32);
    auto reason = guarded<uint8_t>(cap, (uint8_t)0xC5);
    // listed
    if (in->n_leave) {
        for (size_t w = 0; w < n_words; ++w) listed[w] = 0;
        for (uint32_t i = 0; i < in->n_leave; ++i) {
            const uint32_t v = in->leave_ids[i];
            if (v < in->n_ids) listed[v >> 5] |= 1u << (v & 31u);
        }
    }
    // flags: a wave per granule over the reserved room
    for (size_t g = 0; g < nG; ++g) {
        uint64_t word = 0;
        for (uint32_t lane = 0; lane < kJnGranule; ++lane) {
            const size_t e = g * kJnGranule + lane;
            if (e >= cap) break;
            uint32_t r = 0, err = 0;
            if (e < *t.live) r = lv_reason(*in, in->n_leave ? listed.data() : nullptr, t.id[e], &err);
            reason[e] = (uint8_t)r;
            if (r) word |= 1ull << lane;
            ctrl.c.n_listed_found += (r & kLvListed) != 0;
            ctrl.c.n_stale += (r & kLvStale) != 0;
            ctrl.c.error |= err;
        }
        words[g] = word;
    }
    // scan
    uint32_t acc = 0;
    for (size_t g = 0; g <= nG; ++g) {
        base[g] = acc;
        if (g < nG) acc += dsp_popc(words[g]);
    }
    lv_decide(&ctrl, *in, *out, base[nG], *t.live);
    if (ctrl.ok) {
        // apply, in the grid's order
        for (size_t e = 0; e < ctrl.live; ++e) {
            const uint32_t g = (uint32_t)(e / kJnGranule), lane = (uint32_t)(e % kJnGranule);
            const uint32_t below = base[g] + dsp_popc(words[g] & dsp_below(lane));
            if ((words[g] >> lane) & 1ull) {
                const uint32_t v = t.id[e];
                lv_emit(*in, *out, t, (uint32_t)e, below, reason[e], ctrl.k);
                if (out->gone_bits) out->gone_bits[v >> 5] |= 1u << (v & 31u);
            } else if (lv_keep(*in, t, (uint32_t)e, below, ctrl.k != 0, ohi.data(), olo.data(), oid.data())) {
                ctrl.c.n_stamped += 1;
            }
        }
        // back, and the live count
        if (ctrl.k) {
            const uint32_t kept = ctrl.live - ctrl.k;
            for (uint32_t e = 0; e < kept; ++e) hi[e] = ohi[e], lo[e] = olo[e], id[e] = oid[e];
            *t.live = kept;
        }
        // the free list's tail
        if (out->free_out)
            for (uint32_t j = 0; j < in->n_free; ++j) lv_free_tail(*in, *out, ctrl.k, j);
    }
    if (counters) *counters = ctrl.c;
    for (uint32_t e = 0; e < *live_word; ++e) {
        for (int b = 0; b < 8; ++b) {
            table_uuids[16 * (size_t)e + b] = (uint8_t)(hi[e] >> (56 - 8 * b));
            table_uuids[16 * (size_t)e + 8 + b] = (uint8_t)(lo[e] >> (56 - 8 * b));
        }
        table_ids[e] = id[e];
    }
    const bool fine = intact(hi, cap, kGuard64) && intact(lo, cap, kGuard64) && intact(ohi, cap, kGuard64) &&
                      intact(olo, cap, kGuard64) && intact(id, cap, kGuard32) && intact(oid, cap, kGuard32) &&
                      intact(words, nG, kGuard64) && intact(base, nG + 1, kGuard32) && intact(listed, n_words, kGuard32) &&
                      intact(reason, cap, (uint8_t)0xC5);
    return fine ? 0 : 2;
}
