// Test-only shim: runs the ingest joins' arithmetic (csrc/join_ops.hpp) on the CPU in the passes the
// kernels of csrc/wq_join.hip use — the flags granule by granule with their ballot words, the rank scan,
// the compaction with its padding, two stable 64-bit sort passes (low half, then high half) with the
// gathers between them, the heads scattered to frame order, the two scans of the heads, the decision, the
// table's copy, the apply lane by lane (as a sorted position, then as a frame), the merge of the old
// entries and the live count — so the result is checked byte for byte against
// worldql_server_amd/ingest.py (join_peers_np, drop_peers_np) without a GPU
// (tests/test_ingest_join_cpp_mirror.py). The GPU instance: tests/test_gpu_ingest_join.py.
//
// The table arrives as uuid bytes with `cap` slots; the working arrays here have exactly the sizes the
// device call allocates plus eight guard entries each, which must come back untouched (return 2).
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../worldql_server_amd/csrc/join_ops.hpp"

extern "C" uint32_t wq_test_join_sizes(int which) {
    return which == 0 ? sizeof(wq_join_in) : which == 1 ? sizeof(wq_join_out) : which == 2 ? sizeof(wq_join_counters)
                                                                                           : sizeof(wq::JnCtrl);
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

// The table as the handle keeps it.
struct HostTable {
    std::vector<uint64_t> hi, lo, ohi, olo;
    std::vector<uint32_t> id, oid;
    uint32_t cap;
    HostTable(const uint8_t* uuids, const uint32_t* ids, uint32_t live, uint32_t cap_)
        : hi(guarded<uint64_t>(cap_, kGuard64)), lo(guarded<uint64_t>(cap_, kGuard64)), ohi(guarded<uint64_t>(cap_, kGuard64)),
          olo(guarded<uint64_t>(cap_, kGuard64)), id(guarded<uint32_t>(cap_, kGuard32)), oid(guarded<uint32_t>(cap_, kGuard32)),
          cap(cap_) {
        for (uint32_t e = 0; e < live; ++e) hi[e] = wq::jn_be64(uuids + 16 * (size_t)e), lo[e] = wq::jn_be64(uuids + 16 * (size_t)e + 8), id[e] = ids[e];
    }
    bool ok() const {
        return intact(hi, cap, kGuard64) && intact(lo, cap, kGuard64) && intact(ohi, cap, kGuard64) && intact(olo, cap, kGuard64) &&
               intact(id, cap, kGuard32) && intact(oid, cap, kGuard32);
    }
    void store(uint8_t* uuids, uint32_t* ids, uint32_t live) const {
        for (uint32_t e = 0; e < live; ++e) {
            for (int b = 0; b < 8; ++b) {
                uuids[16 * (size_t)e + b] = (uint8_t)(hi[e] >> (56 - 8 * b));
                uuids[16 * (size_t)e + 8 + b] = (uint8_t)(lo[e] >> (56 - 8 * b));
            }
            ids[e] = id[e];
        }
    }
};

// A stable sort of (key, value) pairs by key: what one radix pass over all 64 bits leaves.
void stable_pass(const uint64_t* kin, uint64_t* kout, const uint32_t* vin, uint32_t* vout, size_t n) {
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return kin[a] < kin[b]; });
    for (size_t i = 0; i < n; ++i) kout[i] = kin[order[i]], vout[i] = vin[order[i]];
}

}  // namespace

// As wq_ingest_join_device, all host memory; the table as uuids / ids with cap slots and *live entries.
// Returns 0, or 2 when a guard entry was written.
extern "C" int wq_test_ingest_join_host(const wq_join_in* in, uint64_t n64, const wq_join_out* out, wq_join_counters* counters,
                                        uint8_t* table_uuids, uint32_t* table_ids, uint32_t* live_word, uint32_t cap,
                                        int reserved) {
    using namespace wq;
    const uint32_t n = (uint32_t)n64;
    JnCtrl ctrl;
    memset(&ctrl, 0, sizeof(ctrl));
    if (!reserved) {
        jn_no_table(&ctrl, n, in->id_next);
        if (counters) *counters = ctrl.c;
        return 0;
    }
    HostTable tab(table_uuids, table_ids, *live_word, cap);
    const JnTable t{tab.hi.data(), tab.lo.data(), tab.id.data(), live_word, cap};
    const size_t N = n, nG = (N + kJnGranule - 1) / kJnGranule;
    auto chi = guarded<uint64_t>(N, kGuard64), clo = chi, tmp = chi, chi1 = chi, shi = chi, words = guarded<uint64_t>(nG, kGuard64);
    auto cfr = guarded<uint32_t>(N, kGuard32), iota = cfr, perm1 = cfr, perm2 = cfr, sfr = cfr;
    auto rank = guarded<uint32_t>(N + 1, kGuard32), hb = rank, base = guarded<uint32_t>(nG + 1, kGuard32);
    std::vector<uint8_t> bits(N);
    const JnCand w{chi.data(), clo.data(), cfr.data(), iota.data()};
    const JnSorted s{shi.data(), tmp.data(), sfr.data(), perm2.data()};
    if (n) {
        // flags: a wave per granule
        for (size_t g = 0; g < nG; ++g) {
            uint64_t word = 0;
            for (uint32_t lane = 0; lane < kJnGranule; ++lane) {
                const size_t i = g * kJnGranule + lane;
                if (i >= N) break;
                uint32_t err = 0;
                const uint32_t f = jn_check_new(t, in->sender_uuid, (uint32_t)i,
                                                jn_flags(in->instruction[i], in->flags[i], in->world[i], in->sender[i], &err), &err);
                bits[i] = (uint8_t)f;
                if (f & kJnCand) word |= 1ull << lane;
                if (err) ctrl.c.error |= kJnErrDisagree;
            }
            words[g] = word;
        }
        // scan
        uint32_t acc = 0;
        for (size_t g = 0; g <= nG; ++g) {
            base[g] = acc;
            if (g < nG) acc += dsp_popc(words[g]);
        }
        // compact
        for (size_t i = 0; i < N; ++i)
            jn_compact(w, in->sender_uuid, (uint32_t)i, (bits[i] & kJnCand) != 0, words[i / kJnGranule], base[i / kJnGranule],
                       base[nG]);
        // sort: the low halves, a gather, the high halves, a gather
        stable_pass(clo.data(), tmp.data(), iota.data(), perm1.data(), N);
        for (size_t i = 0; i < N; ++i) chi1[i] = chi[perm1[i]];
        stable_pass(chi1.data(), shi.data(), perm1.data(), perm2.data(), N);
        for (size_t i = 0; i < N; ++i) tmp[i] = clo[perm2[i]], sfr[i] = cfr[perm2[i]];
        // heads, to frame order (iota is free now)
        for (size_t i = 0; i < N; ++i) iota[s.perm[i]] = jn_head(s, (uint32_t)i, base[nG]) ? 1u : 0u;
        acc = 0;
        for (size_t r = 0; r <= N; ++r) {
            rank[r] = acc;
            if (r < N) acc += iota[r];
        }
    }
    jn_decide(&ctrl, *in, *out, n, n ? base[nG] : 0u, n ? rank[N] : 0u, *t.live, t.cap);
    if (n) {
        uint32_t acc = 0;
        for (size_t pos = 0; pos <= N; ++pos) {
            hb[pos] = acc;
            if (pos < N && jn_head(s, (uint32_t)pos, ctrl.n_cand)) acc += 1;
        }
        if (ctrl.ok && ctrl.k) {
            for (uint32_t e = 0; e < ctrl.live; ++e) tab.ohi[e] = t.hi[e], tab.olo[e] = t.lo[e], tab.oid[e] = t.id[e];
            // apply, in the grid's order
            for (size_t i = 0; i < N; ++i) {
                if (jn_head(s, (uint32_t)i, ctrl.n_cand)) {
                    const uint32_t r = rank[s.perm[i]];
                    jn_emit(*in, *out, s, (uint32_t)i, r, &ctrl);
                    jn_merge_new(t, tab.ohi.data(), tab.olo.data(), ctrl.live, s, hb.data(), (uint32_t)i, jn_join_id(*in, r));
                }
                if ((bits[i] & kJnUnknown) && jn_patch(*in, s, rank.data(), ctrl.n_cand, (uint32_t)i)) ctrl.c.n_patched += 1;
            }
            for (uint32_t e = 0; e < ctrl.live; ++e)
                jn_merge_old(t, tab.ohi.data(), tab.olo.data(), tab.oid.data(), e, s, hb.data(), ctrl.n_cand);
            *t.live = ctrl.live + ctrl.k;
        }
    }
    if (counters) *counters = ctrl.c;
    tab.store(table_uuids, table_ids, *live_word);
    const bool fine = tab.ok() && intact(chi, N, kGuard64) && intact(clo, N, kGuard64) && intact(tmp, N, kGuard64) &&
                      intact(chi1, N, kGuard64) && intact(shi, N, kGuard64) && intact(words, nG, kGuard64) &&
                      intact(cfr, N, kGuard32) && intact(iota, N, kGuard32) && intact(perm1, N, kGuard32) &&
                      intact(perm2, N, kGuard32) && intact(sfr, N, kGuard32) && intact(rank, N + 1, kGuard32) &&
                      intact(hb, N + 1, kGuard32) && intact(base, nG + 1, kGuard32);
    return fine ? 0 : 2;
}

// As wq_ingest_drop_peers_device, all host memory. Returns 0, or 2 when a guard entry was written.
extern "C" int wq_test_ingest_drop_host(const uint32_t* ids, uint64_t n, wq_join_counters* counters, uint8_t* table_uuids,
                                        uint32_t* table_ids, uint32_t* live_word, uint32_t cap, int reserved) {
    using namespace wq;
    JnCtrl ctrl;
    memset(&ctrl, 0, sizeof(ctrl));
    if (!reserved) {
        jn_no_table(&ctrl, n, 0);
        if (counters) *counters = ctrl.c;
        return 0;
    }
    HostTable tab(table_uuids, table_ids, *live_word, cap);
    const size_t nG = ((size_t)cap + kJnGranule - 1) / kJnGranule;
    const uint32_t live = *live_word;
    uint32_t kept = live;
    auto words = guarded<uint64_t>(nG, kGuard64);
    auto base = guarded<uint32_t>(nG + 1, kGuard32);
    if (n && cap) {
        std::vector<uint32_t> sorted(ids, ids + n);
        std::sort(sorted.begin(), sorted.end());
        for (size_t g = 0; g < nG; ++g) {
            uint64_t word = 0;
            for (uint32_t lane = 0; lane < kJnGranule; ++lane) {
                const size_t e = g * kJnGranule + lane;
                if (e < cap && jn_drop_keep(tab.id.data(), sorted.data(), (uint32_t)n, live, (uint32_t)e)) word |= 1ull << lane;
            }
            words[g] = word;
        }
        uint32_t acc = 0;
        for (size_t g = 0; g <= nG; ++g) {
            base[g] = acc;
            if (g < nG) acc += dsp_popc(words[g]);
        }
        kept = base[nG];
        if (kept != live) {
            for (size_t e = 0; e < cap; ++e) {
                const uint64_t word = words[e / kJnGranule];
                if (!((word >> (e % kJnGranule)) & 1)) continue;
                const uint32_t d = base[e / kJnGranule] + dsp_popc(word & dsp_below((uint32_t)(e % kJnGranule)));
                tab.ohi[d] = tab.hi[e], tab.olo[d] = tab.lo[e], tab.oid[d] = tab.id[e];
            }
            for (uint32_t e = 0; e < kept; ++e) tab.hi[e] = tab.ohi[e], tab.lo[e] = tab.olo[e], tab.id[e] = tab.oid[e];
        }
    }
    jn_drop_finish(&ctrl, n, live, kept);
    *live_word = kept;
    if (counters) *counters = ctrl.c;
    tab.store(table_uuids, table_ids, kept);
    return tab.ok() && intact(words, nG, kGuard64) && intact(base, nG + 1, kGuard32) ? 0 : 2;
}
