// Test-only shim: the vacuum, export and import of the record store on the CPU, built from the
// functions csrc/record_ops.hpp adds for them (rec_row_move, rec_row_export, rec_row_import,
// rec_adjacent_equal) in the shape of the kernels of wq_records.hip — flag / scan / move / remap for
// the vacuum and the export, classify / scan / append / eight stable sort passes / check for the
// import — over the host store of records_host_shim.hip, whose apply and read run between them. Every
// array a vacuum or an export writes is followed by canary words that must survive. The result is
// checked byte for byte against worldql_server_amd/records.py (tests/test_records_vacuum_cpp_mirror.py);
// the GPU instance in tests/test_gpu_records_vacuum.py.
//
// With -DWQ_RECORDS_VACUUM_SHIM_MAIN the file is a program of its own: a seeded random stream of
// applies, reads, vacuums and export / import round trips against a brute-force model over exactly
// sized heap buffers, for a host build under -fsanitize=address,undefined.
#include "records_host_shim.hip"

namespace {

constexpr size_t kCanary = 8;
constexpr int kCanaryDied = -100;  // no WQ_E_* code
constexpr uint32_t kMark32 = 0xA5A5A5A5u;
constexpr uint64_t kMark64 = 0xA5A5A5A5A5A5A5A5ull;

// The arrays of a store sized for n rows, each with canary words behind it.
struct Fresh {
    HostStore s;
    size_t n, words;
    explicit Fresh(size_t rows) : n(rows), words((rows + 3) / 4) {
        for (int v = 0; v < 2; ++v) {
            s.k_hi[v].assign(n + kCanary, kMark32);
            s.k_lo[v].assign(n + kCanary, kMark64);
            s.view[v].assign(n + kCanary, kMark32);
        }
        s.handle.assign(n + kCanary, kMark32);
        s.uuid_hi.assign(n + kCanary, kMark64);
        s.uuid_lo.assign(n + kCanary, kMark64);
        s.seq.assign(n + kCanary, kMark64);
        s.ts.assign(n + kCanary, (int64_t)kMark64);
        s.live.assign(words + kCanary, kMark32);
        std::fill(s.live.begin(), s.live.begin() + words, 0u);
    }
    template <typename T>
    static bool tail(std::vector<T>& a, size_t keep, T mark) {
        for (size_t i = keep; i < a.size(); ++i)
            if (a[i] != mark) return false;
        a.resize(keep);
        return true;
    }
    // Are the canaries intact? Cuts them off.
    bool trim() {
        bool ok = true;
        for (int v = 0; v < 2; ++v) {
            ok &= tail(s.k_hi[v], n, kMark32);
            ok &= tail(s.k_lo[v], n, kMark64);
            ok &= tail(s.view[v], n, kMark32);
        }
        ok &= tail(s.handle, n, kMark32) && tail(s.uuid_hi, n, kMark64) && tail(s.uuid_lo, n, kMark64);
        ok &= tail(s.seq, n, kMark64) && tail(s.ts, n, (int64_t)kMark64) && tail(s.live, words, kMark32);
        return ok;
    }
};

// flag / scan: map[t] is live row t's index among the live rows; returns their number.
uint32_t rows_map(HostStore& s, std::vector<uint32_t>& flag, std::vector<uint32_t>& map) {
    const uint32_t S = (uint32_t)s.n_rows;
    flag.assign(S, 0);
    map.assign(S, 0);
    for (uint32_t t = 0; t < S; ++t) flag[t] = rec_is_live(s.live.data(), t) ? 1u : 0u;
    uint32_t sum = 0;
    for (uint32_t t = 0; t < S; ++t) {
        map[t] = sum;
        sum += flag[t];
    }
    return sum;
}

// 0, or kCanaryDied.
int vacuum(HostStore& s, wq_rec_vacuum_result* res) {
    s.compact();
    const uint32_t S = (uint32_t)s.n_rows;
    *res = wq_rec_vacuum_result{S, S, 0, 0};
    if (s.n_live == S) return 0;
    std::vector<uint32_t> flag, map;
    const uint32_t L = rows_map(s, flag, map);
    if (s.view[0].size() != L || s.view[1].size() != L) return kCanaryDied;  // (or the views are out of step)
    Fresh f(L);
    f.s.cfg = s.cfg;
    const RecRows from = s.rows(), to = f.s.rows();
    for (uint32_t t = 0; t < S; ++t)
        if (rec_is_live(from.live, t)) rec_row_move(from, t, to, map[t]);
    for (int v = 0; v < 2; ++v)
        for (uint32_t t = 0; t < L; ++t) f.s.view[v][t] = map[s.view[v][t]];
    if (!f.trim()) return kCanaryDied;
    for (int v = 0; v < 2; ++v) {
        s.k_hi[v].swap(f.s.k_hi[v]);
        s.k_lo[v].swap(f.s.k_lo[v]);
        s.view[v].swap(f.s.view[v]);
    }
    s.handle.swap(f.s.handle);
    s.uuid_hi.swap(f.s.uuid_hi);
    s.uuid_lo.swap(f.s.uuid_lo);
    s.seq.swap(f.s.seq);
    s.ts.swap(f.s.ts);
    s.live.swap(f.s.live);
    s.n_rows = L;  // the dead list and ops_seen stay
    res->rows_after = L;
    return 0;
}

int export_rows(HostStore& s, wq_rec_row* out, size_t capacity, size_t* n) {
    std::vector<uint32_t> flag, map;
    const uint32_t L = rows_map(s, flag, map);
    *n = L;
    if (L > capacity) return WQ_E_CAPACITY;
    const RecRows r = s.rows();
    for (uint32_t t = 0; t < (uint32_t)s.n_rows; ++t)
        if (rec_is_live(r.live, t)) out[map[t]] = rec_row_export(s.cfg, r, t);
    return WQ_OK;
}

int import_rows(HostStore& s, const wq_rec_row* rows, size_t n, uint64_t ops_seen, wq_rec_import_result* res) {
    *res = wq_rec_import_result{0, 0};
    if (s.ops_seen != 0 || s.n_rows != 0) return WQ_E_INVALID;
    // classify, scan
    std::vector<RecPacked> rk(n), tk(n);
    std::vector<uint32_t> flag(n), pos(n);
    uint32_t m = 0;
    for (size_t i = 0; i < n; ++i) {
        flag[i] = rec_row_import(s.cfg, rows[i], ops_seen, &rk[i], &tk[i]) ? 1u : 0u;
        pos[i] = m;
        m += flag[i];
    }
    // append
    Fresh f(m);
    f.s.cfg = s.cfg;
    const RecRows r = f.s.rows();
    for (size_t i = 0; i < n; ++i) {
        if (!flag[i]) continue;
        const uint32_t row = pos[i];
        r.k_hi[0][row] = rk[i].hi;
        r.k_lo[0][row] = rk[i].lo;
        r.k_hi[1][row] = tk[i].hi;
        r.k_lo[1][row] = tk[i].lo;
        r.uuid_hi[row] = rows[i].uuid_hi;
        r.uuid_lo[row] = rows[i].uuid_lo;
        r.ts[row] = rows[i].ts_us;
        r.seq[row] = rows[i].seq;
        r.handle[row] = rows[i].handle;
        reinterpret_cast<uint8_t*>(r.live)[row] = 1;
    }
    // the stable passes from the last key word up; a row that was not accepted sorts to the end
    auto word = [&](int w, uint32_t i) -> uint64_t {
        switch (w) {
            case 0: return (uint64_t)rows[i].ts_us ^ (1ull << 63);
            case 1: return rows[i].uuid_lo;
            case 2: return rows[i].uuid_hi;
            case 3: return rk[i].lo;
            case 4: return flag[i] ? rk[i].hi : 1ull << 32;
            case 5: return tk[i].lo;
            case 6: return flag[i] ? tk[i].hi : 1ull << 32;
            default: return rows[i].seq;
        }
    };
    auto pass = [&](std::vector<uint32_t>& idx, int w) {
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return word(w, a) < word(w, b); });
    };
    std::vector<uint32_t> idx(n);
    for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)i;
    for (int w : {7, 0, 1, 2}) pass(idx, w);
    std::vector<uint32_t> s0 = idx, s1 = idx;
    pass(s0, 3);
    pass(s0, 4);
    pass(s1, 5);
    pass(s1, 6);
    for (uint32_t j = 0; j < m; ++j) {
        f.s.view[0][j] = pos[s0[j]];
        f.s.view[1][j] = pos[s1[j]];
    }
    if (!f.trim()) return kCanaryDied;
    res->rejected = n - m;
    // check
    bool dup = false;
    for (uint32_t t = 1; t < m; ++t) dup |= rec_adjacent_equal(f.s.rows(), f.s.view[0].data(), t);
    if (dup) return WQ_E_INVALID;  // the store stays empty
    s = f.s;
    s.n_rows = s.n_live = m;
    s.ops_seen = ops_seen;
    res->imported = m;
    return WQ_OK;
}

}  // namespace

extern "C" {

int wq_test_rec_vacuum(void* s, wq_rec_vacuum_result* res) { return vacuum(*static_cast<HostStore*>(s), res); }
int wq_test_rec_export(void* s, wq_rec_row* out, size_t capacity, size_t* n, uint64_t* ops_seen) {
    *ops_seen = static_cast<HostStore*>(s)->ops_seen;
    return export_rows(*static_cast<HostStore*>(s), out, capacity, n);
}
int wq_test_rec_import(void* s, const wq_rec_row* rows, size_t n, uint64_t ops_seen, wq_rec_import_result* res) {
    return import_rows(*static_cast<HostStore*>(s), rows, n, ops_seen, res);
}

}  // extern "C"

#ifdef WQ_RECORDS_VACUUM_SHIM_MAIN
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>

namespace {

// The model: every live or dead row in a flat list, every call a scan of it (records.py).
struct MRow {
    uint32_t world;
    int64_t reg[3], tab[3];
    uint64_t uh, ul, seq;
    int64_t ts;
    uint32_t handle;
    bool live;
};

struct VModel {
    RecCfg cfg;
    std::vector<MRow> rows;
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
    size_t live() const {
        size_t n = 0;
        for (const MRow& x : rows) n += x.live;
        return n;
    }
};

uint64_t v_rng = 0x9E3779B97F4A7C15ull;
uint32_t vrnd(uint32_t n) {
    v_rng ^= v_rng << 13;
    v_rng ^= v_rng >> 7;
    v_rng ^= v_rng << 17;
    return (uint32_t)((v_rng >> 33) % n);
}

#define VCHECK(c)                                                         \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

}  // namespace

int main() {
    HostStore* st = new HostStore();
    st->cfg = RecCfg{{16, 256, 16}, 1024};
    VModel md;
    md.cfg = st->cfg;
    const double xs[] = {-40.0, -16.0, -15.5, -0.0, 3.0, 17.0, 1010.0, 1030.0, -1010.0, -1030.0, NAN, 16.0 * (1 << 23)};
    uint32_t next_handle = 0;
    uint64_t reads = 0, returned = 0, deduped = 0, deleted = 0, vacuums = 0, dropped = 0, trips = 0, carried = 0,
             refused = 0, import_rejected = 0;
    for (int round = 0; round < 90; ++round) {
        const size_t n = round % 7 == 6 ? 0 : 1 + vrnd(300);
        wq_rec_op* ops = new wq_rec_op[n ? n : 1];
        for (size_t i = 0; i < n; ++i) {
            wq_rec_op& o = ops[i];
            o.kind = vrnd(8) == 0 ? WQ_RECORD_DELETE : WQ_RECORD_CREATE;
            o.world = vrnd(50) == 0 ? (1u << 24) - 1 : vrnd(2);
            o.pos[0] = xs[vrnd(vrnd(20) ? 10 : 12)];
            o.pos[1] = vrnd(2) ? 5.0 : -5.0;
            o.pos[2] = xs[vrnd(6)];
            o.uuid_hi = vrnd(3);
            o.uuid_lo = vrnd(40);
            o.ts_us = (int64_t)vrnd(20) - 5;
            o.handle = o.kind == WQ_RECORD_CREATE ? next_handle++ : 0;
            o.reserved = 0;
        }
        wq_rec_apply_result ar;
        st->apply(ops, n, &ar);
        uint64_t m_created = 0, m_deleted = 0;
        for (size_t i = 0; i < n; ++i) {
            MRow r{};
            if (!md.key(ops[i].world, ops[i].pos, r.reg, r.tab)) continue;
            if (ops[i].kind == WQ_RECORD_CREATE) {
                r.world = ops[i].world, r.uh = ops[i].uuid_hi, r.ul = ops[i].uuid_lo, r.seq = md.ops_seen + i;
                r.ts = ops[i].ts_us, r.handle = ops[i].handle, r.live = true;
                md.rows.push_back(r);
                ++m_created;
            } else {
                for (MRow& x : md.rows)
                    if (x.live && x.world == ops[i].world && x.uh == ops[i].uuid_hi && x.ul == ops[i].uuid_lo &&
                        std::equal(x.reg, x.reg + 3, r.reg)) {
                        x.live = false;
                        md.dead.push_back(x.handle);
                        ++m_deleted;
                    }
            }
        }
        md.ops_seen += n;
        VCHECK(ar.created == m_created && ar.deleted_rows == m_deleted && ar.rows_live == md.live());
        deleted += m_deleted;
        delete[] ops;

        // between the apply and the read (views still dirty): a vacuum, a round trip, or nothing
        const int what = round % 3;
        if (what == 0) {
            const size_t before = st->n_rows;
            wq_rec_vacuum_result vr;
            VCHECK(vacuum(*st, &vr) == 0);
            VCHECK(vr.rows_before == before && vr.rows_after == md.live() && st->n_rows == md.live());
            ++vacuums;
            dropped += before - st->n_rows;
        } else if (what == 1) {
            // the dead list is drained before the switch: it is no part of a snapshot
            std::sort(md.dead.begin(), md.dead.end());
            uint32_t* dl = new uint32_t[md.dead.size() ? md.dead.size() : 1];
            VCHECK(wq_test_rec_drain(st, dl, md.dead.size()) == md.dead.size());
            VCHECK(std::equal(md.dead.begin(), md.dead.end(), dl));
            delete[] dl;
            md.dead.clear();
            const size_t L = md.live();
            size_t cnt = 0;
            if (L) {  // one short: nothing written (the buffer is exactly that long)
                wq_rec_row* shorter = new wq_rec_row[L - 1 ? L - 1 : 1];
                VCHECK(export_rows(*st, shorter, L - 1, &cnt) == WQ_E_CAPACITY && cnt == L);
                delete[] shorter;
            }
            wq_rec_row* snap = new wq_rec_row[L ? L : 1];
            VCHECK(export_rows(*st, snap, L, &cnt) == WQ_OK && cnt == L);
            size_t j = 0;
            for (const MRow& x : md.rows) {
                if (!x.live) continue;
                const wq_rec_row& e = snap[j++];
                VCHECK(e.world == x.world && e.handle == x.handle && e.uuid_hi == x.uh && e.uuid_lo == x.ul);
                VCHECK(e.ts_us == x.ts && e.seq == x.seq && std::equal(x.reg, x.reg + 3, e.region));
            }
            VCHECK(j == L);
            HostStore* nx = new HostStore();
            nx->cfg = st->cfg;
            wq_rec_import_result ir;
            if (L >= 2 && trips % 4 == 3) {  // a snapshot with one row twice is refused, the store stays empty
                wq_rec_row* bad = new wq_rec_row[L + 1];
                std::copy(snap, snap + L, bad);
                bad[L] = snap[vrnd((uint32_t)L)];
                bad[L].handle ^= 1u;  // no part of the key
                VCHECK(import_rows(*nx, bad, L + 1, md.ops_seen, &ir) == WQ_E_INVALID && nx->n_rows == 0 && nx->ops_seen == 0);
                delete[] bad;
                ++refused;
            }
            if (L >= 1 && trips % 4 == 1) {  // a row past the op counter and one off the grid are counted
                wq_rec_row* more = new wq_rec_row[L + 2];
                std::copy(snap, snap + L, more + 1);
                more[0] = snap[0];
                more[0].seq = md.ops_seen;
                more[L + 1] = snap[0];
                more[L + 1].region[2] += 1;
                VCHECK(import_rows(*nx, more, L + 2, md.ops_seen, &ir) == WQ_OK && ir.imported == L && ir.rejected == 2);
                delete[] more;
                import_rejected += 2;
            } else {
                VCHECK(import_rows(*nx, snap, L, md.ops_seen, &ir) == WQ_OK && ir.imported == L && ir.rejected == 0);
            }
            VCHECK(nx->n_rows == L && nx->n_live == L && nx->ops_seen == md.ops_seen);
            delete[] snap;
            delete st;
            st = nx;
            std::vector<MRow> kept;
            for (const MRow& x : md.rows)
                if (x.live) kept.push_back(x);
            carried += kept.size();
            md.rows.swap(kept);
            ++trips;
        }

        // a read of a few queries into exactly sized outputs, with and without the dedupe
        const size_t nq = round % 5 == 4 ? 0 : 1 + vrnd(12);
        uint32_t* world = new uint32_t[nq ? nq : 1];
        double* pos = new double[nq ? 3 * nq : 1];
        int64_t* after = new int64_t[nq ? nq : 1];
        for (size_t i = 0; i < nq; ++i) {
            world[i] = vrnd(2);
            pos[3 * i] = xs[vrnd(vrnd(10) ? 10 : 12)];
            pos[3 * i + 1] = vrnd(2) ? 5.0 : -5.0;
            pos[3 * i + 2] = xs[vrnd(6)];
            after[i] = vrnd(3) ? INT64_MIN : (int64_t)vrnd(20) - 5;
        }
        std::vector<uint32_t> m_off(nq + 1, 0);
        std::vector<const MRow*> m_win;
        for (size_t i = 0; i < nq; ++i) {
            int64_t reg[3], tab[3];
            if (md.key(world[i], pos + 3 * i, reg, tab)) {
                std::map<std::pair<uint64_t, uint64_t>, const MRow*> best;
                for (const MRow& x : md.rows) {
                    if (!x.live || x.world != world[i] || !std::equal(x.reg, x.reg + 3, reg) || !(x.ts > after[i])) continue;
                    const MRow*& b = best[{x.uh, x.ul}];
                    if (!b || std::make_pair(x.ts, x.seq) > std::make_pair(b->ts, b->seq)) b = &x;
                }
                for (auto& kv : best) m_win.push_back(kv.second);
            }
            m_off[i + 1] = (uint32_t)m_win.size();
        }
        const size_t P = m_win.size();
        const bool dedupe = round % 4 != 0;
        uint32_t* off = new uint32_t[nq + 1];
        uint32_t* hd = new uint32_t[P ? P : 1];
        int64_t* tso = new int64_t[P ? P : 1];
        wq_rec_read_result rr;
        VCHECK(st->read(nq, world, pos, after, dedupe ? WQ_RECORD_READ_DEDUPE : 0, off, hd, tso, P, &rr) == WQ_OK);
        VCHECK(rr.returned == P && rr.overflow == 0);
        for (size_t i = 0; i <= nq; ++i) VCHECK(off[i] == m_off[i]);
        for (size_t p = 0; p < P; ++p) VCHECK(hd[p] == m_win[p]->handle && tso[p] == m_win[p]->ts);
        uint64_t m_deduped = 0;
        if (dedupe)
            for (const MRow* w : m_win)
                for (MRow& x : md.rows)
                    if (x.live && x.world == w->world && x.uh == w->uh && x.ul == w->ul &&
                        std::equal(x.tab, x.tab + 3, w->tab) && x.ts < w->ts) {
                        x.live = false;
                        md.dead.push_back(x.handle);
                        ++m_deduped;
                    }
        VCHECK(rr.deduped_rows == m_deduped);
        deduped += m_deduped;
        delete[] off;
        delete[] hd;
        delete[] tso;
        delete[] world;
        delete[] pos;
        delete[] after;
        ++reads;
        returned += P;
        if (round % 2) {  // every other round the handles stay undrained across the next vacuum
            std::sort(md.dead.begin(), md.dead.end());
            uint32_t* dl = new uint32_t[md.dead.size() ? md.dead.size() : 1];
            VCHECK(wq_test_rec_drain(st, dl, md.dead.size()) == md.dead.size());
            VCHECK(std::equal(md.dead.begin(), md.dead.end(), dl));
            delete[] dl;
            md.dead.clear();
        }
        VCHECK(st->n_live == md.live() && st->ops_seen == md.ops_seen);
    }
    delete st;
    VCHECK(returned > 500 && deduped > 300 && deleted > 100 && dropped > 1000 && carried > 1000 && refused >= 3 &&
           import_rejected >= 6);
    printf("records vacuum shim ok: %llu vacuums dropped %llu rows, %llu round trips carried %llu rows (%llu refused, "
           "%llu rows rejected), %llu reads, %llu rows returned, %llu deduped, %llu deleted\n",
           (unsigned long long)vacuums, (unsigned long long)dropped, (unsigned long long)trips,
           (unsigned long long)carried, (unsigned long long)refused, (unsigned long long)import_rejected,
           (unsigned long long)reads, (unsigned long long)returned, (unsigned long long)deduped,
           (unsigned long long)deleted);
    return 0;
}
#endif
