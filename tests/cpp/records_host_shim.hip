// Test-only shim: runs the record store's arithmetic (csrc/record_ops.hpp: the two quantisers, the
// packed keys, the total order on rows, the range bounds, the winner test and the output offset of a
// query) on the CPU in the shape the kernels of wq_records.hip use it — rows appended in op order, a
// batch sorted and merged into both views by rank, deletes over their (region, uuid) range, then per
// read the ranges, their saturating prefix, a flag word and a count per granule of 64 ordinals, the
// counts' prefix, every winner placed from its granule's prefix, every query's offset derived from
// the same prefix, and the dedupe over each winner's (table, uuid) range — so the result is checked
// byte for byte against worldql_server_amd/records.py without a GPU
// (tests/test_records_cpp_mirror.py). The GPU instance is checked in tests/test_gpu_records.py.
//
// With -DWQ_RECORDS_SHIM_MAIN the file is a program of its own: a random stream against a
// brute-force model over exactly sized heap buffers, the truncated capacities included, for a host
// build under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/wq_router.h"
#include "../../worldql_server_amd/csrc/record_ops.hpp"

namespace {

using namespace wq;

struct HostStore {
    RecCfg cfg;
    std::vector<uint32_t> k_hi[2], handle, live, view[2], dead;
    std::vector<uint64_t> k_lo[2], uuid_hi, uuid_lo, seq;
    std::vector<int64_t> ts;
    uint64_t n_rows = 0, ops_seen = 0, n_live = 0;

    RecRows rows() {
        RecRows r;
        for (int v = 0; v < 2; ++v) {
            r.k_hi[v] = k_hi[v].data();
            r.k_lo[v] = k_lo[v].data();
        }
        r.uuid_hi = uuid_hi.data();
        r.uuid_lo = uuid_lo.data();
        r.ts = ts.data();
        r.seq = seq.data();
        r.handle = handle.data();
        r.live = live.data();
        return r;
    }

    uint32_t kill(uint32_t row) {
        if (!rec_kill(live.data(), row)) return 0;
        dead.push_back(handle[row]);
        --n_live;
        return 1;
    }

    template <int V>
    void merge(const std::vector<uint32_t>& batch) {
        const RecRows r = rows();
        const std::vector<uint32_t>& old = view[V];
        std::vector<uint32_t> out(old.size() + batch.size());
        for (size_t t = 0; t < old.size(); ++t)
            out[t + rec_lower_bound<V>(r, batch.data(), (uint32_t)batch.size(), rec_key<V>(r, old[t]))] = old[t];
        for (size_t j = 0; j < batch.size(); ++j)
            out[j + rec_lower_bound<V>(r, old.data(), (uint32_t)old.size(), rec_key<V>(r, batch[j]))] = batch[j];
        view[V].swap(out);
    }

    void apply(const wq_rec_op* ops, size_t n, wq_rec_apply_result* res) {
        *res = wq_rec_apply_result{0, 0, 0, 0};
        std::vector<RecPacked> rk(n), tk(n);
        std::vector<uint8_t> ok(n);
        std::vector<uint32_t> batch;
        for (size_t i = 0; i < n; ++i) {
            ok[i] = ops[i].kind <= WQ_RECORD_DELETE && rec_pack_position(cfg, ops[i].world, ops[i].pos, &rk[i], &tk[i]);
            if (!ok[i]) res->rejected++;
            if (!ok[i] || ops[i].kind != WQ_RECORD_CREATE) continue;
            const uint32_t row = (uint32_t)n_rows++;
            k_hi[0].push_back(rk[i].hi);
            k_lo[0].push_back(rk[i].lo);
            k_hi[1].push_back(tk[i].hi);
            k_lo[1].push_back(tk[i].lo);
            uuid_hi.push_back(ops[i].uuid_hi);
            uuid_lo.push_back(ops[i].uuid_lo);
            ts.push_back(ops[i].ts_us);
            seq.push_back(ops_seen + i);
            handle.push_back(ops[i].handle);
            if ((row & 3u) == 0) live.push_back(0);
            live[row >> 2] |= 1u << ((row & 3u) * 8u);
            batch.push_back(row);
            res->created++;
            ++n_live;
        }
        {
            const RecRows r = rows();
            std::vector<uint32_t> b0 = batch, b1 = batch;
            std::sort(b0.begin(), b0.end(), [&](uint32_t a, uint32_t b) { return rec_less(rec_key<0>(r, a), rec_key<0>(r, b)); });
            std::sort(b1.begin(), b1.end(), [&](uint32_t a, uint32_t b) { return rec_less(rec_key<1>(r, a), rec_key<1>(r, b)); });
            merge<0>(b0);
            merge<1>(b1);
        }
        const RecRows r = rows();
        for (size_t i = 0; i < n; ++i) {
            if (!ok[i] || ops[i].kind != WQ_RECORD_DELETE) continue;
            uint32_t lo, hi;
            rec_uuid_range<0>(r, view[0].data(), (uint32_t)view[0].size(), rk[i], ops[i].uuid_hi, ops[i].uuid_lo, 0, true,
                              &lo, &hi);
            for (uint32_t e = lo; e < hi; ++e)
                if (seq[view[0][e]] < ops_seen + i) res->deleted_rows += kill(view[0][e]);
        }
        ops_seen += n;
        res->rows_live = n_live;
    }

    void compact() {
        for (int v = 0; v < 2; ++v) {
            std::vector<uint32_t> out;
            for (uint32_t row : view[v])
                if (rec_is_live(live.data(), row)) out.push_back(row);
            view[v].swap(out);
        }
    }

    int read(size_t n_q, const uint32_t* world, const double* pos, const int64_t* after, uint32_t flags_in,
              uint32_t* offsets, uint32_t* handles, int64_t* ts_out, size_t capacity, wq_rec_read_result* res) {
        *res = wq_rec_read_result{0, 0, 0, 0, 0, 0};
        compact();
        const RecRows r = rows();
        const uint32_t n = (uint32_t)n_q, nv = (uint32_t)view[0].size();
        const uint32_t* v0 = view[0].data();
        std::vector<uint32_t> q_lo(n + 1, 0), q_len(n + 1, 0), pre(n + 1, 0);
        for (uint32_t i = 0; i < n; ++i) {
            RecPacked rk, tk;
            uint32_t lo = 0, hi = 0;
            if (rec_pack_position(cfg, world[i], pos + 3ull * i, &rk, &tk))
                rec_key_range<0>(r, v0, nv, rk, &lo, &hi);
            else
                res->rejected++;
            q_lo[i] = lo;
            q_len[i] = hi - lo;
        }
        for (uint32_t i = 0; i < n; ++i) pre[i + 1] = rec_sat_add(pre[i], q_len[i]);
        // the first walk is sized without the ranges' total, as on the device; a call whose total is
        // above that walks again with it, and a cut walk kills nothing
        struct Win {
            uint32_t row;
        };
        std::vector<Win> winners;
        uint32_t lim = rec_ordinal_guess(nv, n);
        for (;;) {
            const uint32_t nG = lim / kRecGranule + 1;
            const uint32_t T = pre[n] < lim ? pre[n] : lim;
            std::vector<uint64_t> fl(nG, 0);
            std::vector<uint32_t> cnt(nG, 0), base(nG, 0);
            winners.clear();
            for (uint32_t g = 0; g < nG; ++g) {
                const uint64_t q0 = (uint64_t)g * kRecGranule;
                uint64_t word = 0;
                if (q0 < T) {
                    const uint32_t last = T - (uint32_t)q0 > kRecGranule ? (uint32_t)q0 + kRecGranule - 1 : T - 1;
                    const uint32_t rlo = rec_query_of(pre.data(), 0, n - 1, (uint32_t)q0);
                    const uint32_t rhi = rec_query_of(pre.data(), 0, n - 1, last);
                    for (uint32_t lane = 0; lane < kRecGranule; ++lane) {
                        const uint32_t q = (uint32_t)q0 + lane;
                        if (q >= T) break;
                        const uint32_t i = rec_query_of(pre.data(), rlo, rhi, q);
                        const uint32_t e = q_lo[i] + (q - pre[i]), hi = q_lo[i] + q_len[i];
                        if (e < hi && hi <= nv && rec_is_winner(r, v0, e, hi, after ? after[i] : INT64_MIN)) {
                            word |= 1ull << lane;
                            winners.push_back(Win{v0[e]});
                        }
                    }
                    fl[g] = word;
                }
                cnt[g] = (uint32_t)__builtin_popcountll(word);
            }
            for (uint32_t g = 1; g < nG; ++g) base[g] = base[g - 1] + cnt[g - 1];
            size_t w = 0;
            for (uint32_t g = 0; g < nG; ++g) {
                for (uint32_t lane = 0; lane < kRecGranule; ++lane) {
                    if (!((fl[g] >> lane) & 1ull)) continue;
                    const uint64_t p = (uint64_t)base[g] + (uint32_t)__builtin_popcountll(fl[g] & ((1ull << lane) - 1ull));
                    const uint32_t row = winners[w++].row;
                    if (p < capacity) {
                        handles[p] = handle[row];
                        ts_out[p] = ts[row];
                    }
                }
            }
            for (uint32_t i = 0; i <= n; ++i) offsets[i] = rec_kept_before(base.data(), fl.data(), pre[i] < T ? pre[i] : T);
            res->returned = offsets[n];
            res->scanned = T;
            res->overflow = res->returned > capacity ? 1u : 0u;
            if (pre[n] <= lim) break;
            if (pre[n] > kRecMaxOrdinals) return WQ_E_CAPACITY;
            lim = (pre[n] + (kRecGranule - 1)) & ~(kRecGranule - 1);
        }
        if (flags_in & WQ_RECORD_READ_DEDUPE) {
            const uint32_t* v1 = view[1].data();
            for (const Win& wn : winners) {
                uint32_t a, b;
                rec_older_range<1>(r, v1, nv, wn.row, &a, &b);
                for (uint32_t e = a; e < b; ++e) res->deduped_rows += kill(v1[e]);
            }
        }
        return WQ_OK;
    }
};

}  // namespace

extern "C" {

void* wq_test_rec_open(uint16_t rx, uint16_t ry, uint16_t rz, uint32_t table_size) {
    HostStore* s = new HostStore();
    s->cfg = RecCfg{{rx, ry, rz}, table_size};
    return s;
}
void wq_test_rec_close(void* s) { delete static_cast<HostStore*>(s); }
void wq_test_rec_apply(void* s, const wq_rec_op* ops, size_t n, wq_rec_apply_result* res) {
    static_cast<HostStore*>(s)->apply(ops, n, res);
}
int wq_test_rec_read(void* s, size_t n, const uint32_t* world, const double* pos, const int64_t* after, uint32_t flags,
                      uint32_t* offsets, uint32_t* handles, int64_t* ts, size_t capacity, wq_rec_read_result* res) {
    return static_cast<HostStore*>(s)->read(n, world, pos, after, flags, offsets, handles, ts, capacity, res);
}
// The dead list ascending into out[capacity] (drained only when it fits); returns its length.
size_t wq_test_rec_drain(void* sp, uint32_t* out, size_t capacity) {
    HostStore* s = static_cast<HostStore*>(sp);
    const size_t n = s->dead.size();
    if (n > capacity) return n;
    std::sort(s->dead.begin(), s->dead.end());
    std::copy(s->dead.begin(), s->dead.end(), out);
    s->dead.clear();
    return n;
}
void wq_test_rec_stats(void* sp, uint64_t* out3) {
    HostStore* s = static_cast<HostStore*>(sp);
    out3[0] = s->n_live;
    out3[1] = s->n_rows;
    out3[2] = s->ops_seen;
}
void wq_test_rec_quantize(const double* c, size_t n, uint16_t size, int64_t* region, uint32_t table_size, int64_t* table) {
    for (size_t i = 0; i < n; ++i) {
        region[i] = clamp_region_coord_dev(c[i], size);
        table[i] = clamp_table_size_dev(region[i], (int64_t)table_size);
    }
}

}  // extern "C"

#ifdef WQ_RECORDS_SHIM_MAIN
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <tuple>

namespace {

// The model: every row in a flat list, every call a scan of it (the semantics of records.py).
struct ModelRow {
    uint32_t world;
    int64_t reg[3], tab[3];
    uint64_t uh, ul, seq;
    int64_t ts;
    uint32_t handle;
    bool live;
};

struct Model {
    RecCfg cfg;
    std::vector<ModelRow> rows;
    std::vector<uint32_t> dead;
    uint64_t ops_seen = 0;
    bool key(uint32_t world, const double* p, int64_t* reg, int64_t* tab) const {
        if (world > kMaxPackedWorld) return false;
        for (int d = 0; d < 3; ++d) {
            if (p[d] != p[d]) return false;
            reg[d] = clamp_region_coord_dev(p[d], cfg.size[d]);
            const int64_t idx = reg[d] / cfg.size[d];
            if (idx < -(1 << 23) || idx >= (1 << 23)) return false;
            tab[d] = clamp_table_size_dev(reg[d], cfg.table_size);
        }
        return true;
    }
};

uint64_t g_rng = 0x2545F4914F6CDD1Dull;
uint32_t rnd(uint32_t n) {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 33) % n);
}

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

}  // namespace

int main() {
    HostStore st;
    st.cfg = RecCfg{{16, 256, 16}, 1024};
    Model md;
    md.cfg = st.cfg;
    const double xs[] = {-40.0, -16.0, -15.5, -0.0, 3.0, 17.0, 1010.0, 1030.0, -1010.0, -1030.0, NAN, 16.0 * (1 << 23)};
    uint32_t next_handle = 0;
    uint64_t reads = 0, returned = 0, deduped = 0, deleted = 0, rejected = 0, overflows = 0;
    for (int round = 0; round < 60; ++round) {
        const size_t n = round % 7 == 6 ? 0 : 1 + rnd(400);
        wq_rec_op* ops = new wq_rec_op[n ? n : 1];
        for (size_t i = 0; i < n; ++i) {
            wq_rec_op& o = ops[i];
            o.kind = rnd(10) == 0 ? WQ_RECORD_DELETE : WQ_RECORD_CREATE;
            o.world = rnd(50) == 0 ? (1u << 24) - 1 : rnd(2);
            o.pos[0] = xs[rnd(rnd(20) ? 10 : 12)];
            o.pos[1] = rnd(2) ? 5.0 : -5.0;
            o.pos[2] = xs[rnd(6)];
            o.uuid_hi = rnd(3);
            o.uuid_lo = rnd(40);
            o.ts_us = (int64_t)rnd(20) - 5;
            o.handle = o.kind == WQ_RECORD_CREATE ? next_handle++ : 0;
            o.reserved = 0;
        }
        wq_rec_apply_result ar;
        st.apply(ops, n, &ar);
        uint64_t m_created = 0, m_deleted = 0, m_rejected = 0;
        for (size_t i = 0; i < n; ++i) {
            ModelRow r{};
            const uint64_t seq = md.ops_seen + i;
            if (!md.key(ops[i].world, ops[i].pos, r.reg, r.tab)) {
                ++m_rejected;
                continue;
            }
            if (ops[i].kind == WQ_RECORD_CREATE) {
                r.world = ops[i].world, r.uh = ops[i].uuid_hi, r.ul = ops[i].uuid_lo, r.seq = seq, r.ts = ops[i].ts_us;
                r.handle = ops[i].handle, r.live = true;
                md.rows.push_back(r);
                ++m_created;
            } else {
                for (ModelRow& x : md.rows)
                    if (x.live && x.world == ops[i].world && x.uh == ops[i].uuid_hi && x.ul == ops[i].uuid_lo &&
                        std::equal(x.reg, x.reg + 3, r.reg)) {
                        x.live = false;
                        md.dead.push_back(x.handle);
                        ++m_deleted;
                    }
            }
        }
        md.ops_seen += n;
        CHECK(ar.created == m_created && ar.deleted_rows == m_deleted && ar.rejected == m_rejected);
        deleted += m_deleted;
        rejected += m_rejected;
        delete[] ops;

        // a read of a few queries: exactly sized outputs at the full, a truncated and a zero capacity
        const size_t nq = round % 5 == 4 ? 0 : 1 + rnd(12);
        uint32_t* world = new uint32_t[nq ? nq : 1];
        double* pos = new double[nq ? 3 * nq : 1];
        int64_t* after = new int64_t[nq ? nq : 1];
        for (size_t i = 0; i < nq; ++i) {
            world[i] = rnd(2);
            pos[3 * i] = xs[rnd(rnd(10) ? 10 : 12)];
            pos[3 * i + 1] = rnd(2) ? 5.0 : -5.0;
            pos[3 * i + 2] = xs[rnd(6)];
            after[i] = rnd(3) ? INT64_MIN : (int64_t)rnd(20) - 5;
        }
        // the model's answer
        std::vector<uint32_t> m_off(nq + 1, 0), m_h;
        std::vector<int64_t> m_ts;
        std::vector<const ModelRow*> m_win;
        uint64_t mq_rejected = 0;
        for (size_t i = 0; i < nq; ++i) {
            int64_t reg[3], tab[3];
            if (md.key(world[i], pos + 3 * i, reg, tab)) {
                std::map<std::pair<uint64_t, uint64_t>, const ModelRow*> best;
                for (const ModelRow& x : md.rows) {
                    if (!x.live || x.world != world[i] || !std::equal(x.reg, x.reg + 3, reg) || !(x.ts > after[i])) continue;
                    const ModelRow*& b = best[{x.uh, x.ul}];
                    if (!b || std::make_pair(x.ts, x.seq) > std::make_pair(b->ts, b->seq)) b = &x;
                }
                for (auto& kv : best) m_win.push_back(kv.second);
            } else {
                ++mq_rejected;
            }
            m_off[i + 1] = (uint32_t)m_win.size();
        }
        const size_t P = m_win.size();
        const bool dedupe = round % 3 != 0;
        const size_t caps[3] = {0, P ? P - 1 : 0, P};
        for (int c = 0; c < 3; ++c) {
            const size_t cap = caps[c];
            uint32_t* off = new uint32_t[nq + 1];
            uint32_t* hd = new uint32_t[cap ? cap : 1];
            int64_t* tso = new int64_t[cap ? cap : 1];
            wq_rec_read_result rr;
            // only the last of the three dedupes: the first two must leave the store as it is
            st.read(nq, world, pos, after, dedupe && c == 2 ? WQ_RECORD_READ_DEDUPE : 0, off, hd, tso, cap, &rr);
            CHECK(rr.returned == P && rr.rejected == mq_rejected && rr.error == 0 && rr.overflow == (P > cap ? 1u : 0u));
            for (size_t i = 0; i <= nq; ++i) CHECK(off[i] == m_off[i]);
            for (size_t p = 0; p < std::min(P, cap); ++p) CHECK(hd[p] == m_win[p]->handle && tso[p] == m_win[p]->ts);
            overflows += rr.overflow;
            if (dedupe && c == 2) {
                uint64_t m_deduped = 0;
                for (const ModelRow* w : m_win)
                    for (ModelRow& x : md.rows)
                        if (x.live && x.world == w->world && x.uh == w->uh && x.ul == w->ul &&
                            std::equal(x.tab, x.tab + 3, w->tab) && x.ts < w->ts) {
                            x.live = false;
                            md.dead.push_back(x.handle);
                            ++m_deduped;
                        }
                CHECK(rr.deduped_rows == m_deduped);
                deduped += m_deduped;
            } else {
                CHECK(rr.deduped_rows == 0);
            }
            delete[] off;
            delete[] hd;
            delete[] tso;
        }
        ++reads;
        returned += P;
        rejected += mq_rejected;
        delete[] world;
        delete[] pos;
        delete[] after;
        // the dead list and the counts
        std::sort(md.dead.begin(), md.dead.end());
        uint32_t* dl = new uint32_t[md.dead.size() ? md.dead.size() : 1];
        CHECK(wq_test_rec_drain(&st, dl, md.dead.size()) == md.dead.size());
        CHECK(std::equal(md.dead.begin(), md.dead.end(), dl));
        delete[] dl;
        md.dead.clear();
        uint64_t live = 0;
        for (const ModelRow& x : md.rows) live += x.live;
        CHECK(st.n_live == live && st.n_rows == md.rows.size() && st.ops_seen == md.ops_seen);
    }
    CHECK(returned > 500 && deduped > 500 && deleted > 100 && rejected > 50 && overflows > 50);
    printf("records shim ok: %llu reads, %llu rows returned, %llu deduped, %llu deleted, %llu rejected, %llu truncated reads\n",
           (unsigned long long)reads, (unsigned long long)returned, (unsigned long long)deduped,
           (unsigned long long)deleted, (unsigned long long)rejected, (unsigned long long)overflows);
    return 0;
}
#endif
