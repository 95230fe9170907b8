// Test-only shim: runs the record dispatch's arithmetic (csrc/recdispatch_ops.hpp: the frame rules, the
// record walk, the granules' flag words, the three scans' terms and the emit) on the CPU in the passes the
// kernels of csrc/wq_recdispatch.hip use — frames lane by lane, the count scan, the records granule by
// granule in the striding waves' order with every lane's search narrowed to the entries lanes 0 and 63
// found, the granule scans, the frame scan bracketed block by block (the operator does not commute), the
// emit — so the result is checked byte for byte against worldql_server_amd/ingest.py
// (records_dispatch_np) without a GPU (tests/test_records_dispatch_cpp_mirror.py). The GPU instance:
// tests/test_gpu_records_dispatch.py. Every scratch array is sized exactly: an entry too many is a heap
// overflow. With -DWQ_RECORDS_DISPATCH_SHIM_MAIN the file is a stand-alone program that replays random and
// hostile cases on exactly sized heap buffers, for a sanitizer build.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../worldql_server_amd/csrc/recdispatch_ops.hpp"

extern "C" uint32_t wq_test_recdisp_granule() { return wq::kRdGranule; }
extern "C" uint32_t wq_test_recdisp_sizes(int which) {
    switch (which) {
    case 0: return sizeof(wq_recdisp_in);
    case 1: return sizeof(wq_recdisp_out);
    case 2: return sizeof(wq_recdisp_run);
    case 3: return sizeof(wq_recdisp_defer);
    case 4: return sizeof(wq_rec_op_ref);
    case 5: return sizeof(wq_recdisp_counters);
    default: return sizeof(wq_rec_op);
    }
}
extern "C" int wq_test_parse_after(const uint8_t* s, uint32_t len, int64_t* out) { return wq::rd_parse_after(s, len, out) ? 1 : 0; }

// The handle's side of the call: the world table of wq_frames_set_worlds and the open store's configuration.
struct wq_test_recdisp_env {
    const uint8_t* world_bytes;
    const uint32_t* world_off;
    uint32_t n_worlds;
    uint16_t size[3];
    uint16_t pad_;
    uint32_t table_size;
    uint32_t n_waves;  // the striding waves of the record and emit passes (0: 7)
    uint32_t scan_block;  // entries per bracket of the frame scan (0: 5)
};

// As wq_records_dispatch_device, all host memory. Returns 0.
extern "C" int wq_test_records_dispatch_host(const wq_recdisp_in* in, const wq_test_recdisp_env* env, const wq_recdisp_out* out,
                                             wq_recdisp_counters* counters) {
    using namespace wq;
    std::vector<uint64_t> whash;
    std::vector<uint32_t> wid;
    if (env->n_worlds) dec_world_index(env->world_bytes, env->world_off, env->n_worlds, &whash, &wid);
    DecTables tables;
    memset(&tables, 0, sizeof(tables));
    tables.world_bytes = env->world_bytes, tables.world_off = env->world_off, tables.world_hash = whash.data();
    tables.world_id = wid.data(), tables.n_worlds = env->n_worlds;
    const RecCfg cfg{{env->size[0], env->size[1], env->size[2]}, env->table_size};
    const uint64_t n = in->n_db, nG = in->max_records / kRdGranule + 1;
    const uint32_t n_waves = env->n_waves ? env->n_waves : 7, blk = env->scan_block ? env->scan_block : 5;

    std::vector<uint64_t> pre(n + 1), words(kRdWords * nG), base(nG), cbase(nG);
    std::vector<int64_t> after(n);
    std::vector<RdSum> ex(n + 1);
    std::vector<uint32_t> cnt(n), vec(n);
    std::vector<uint8_t> cls(n);
    const RdWs ws{pre.data(), after.data(), ex.data(), cnt.data(), vec.data(), cls.data(), words.data(), base.data(), cbase.data()};
    wq_recdisp_counters ctrl;
    memset(&ctrl, 0, sizeof(ctrl));

    // frames
    for (uint64_t j = 0; j < n; ++j) {
        const RdFrameRes r = rd_frame_eval(*in, j);
        cls[j] = (uint8_t)r.cls;
        if (out->cls) out->cls[j] = (uint8_t)r.cls;
        cnt[j] = r.count, vec[j] = r.vec, after[j] = r.after;
        (&ctrl.n_skip)[r.cls] += 1;
        ctrl.error |= r.err;
    }
    // scan: the counts
    {
        const RdCountTerm term{cnt.data(), n};
        uint64_t run = 0;
        for (uint64_t j = 0; j <= n; ++j) pre[j] = run, run += term(j);
    }
    const uint32_t T = rd_examined(pre[n], in->max_records);
    const uint32_t nGa = T / kRdGranule + (T % kRdGranule ? 1u : 0u);
    // records: wave w takes granules w, w + n_waves, ...
    for (uint32_t w = 0; w < n_waves && n; ++w) {
        for (uint32_t g = w; g < nGa; g += n_waves) {
            const uint32_t q0 = g * kRdGranule;
            const uint32_t rlo = rd_frame_of(pre.data(), 0, (uint32_t)n - 1, q0);
            const uint32_t rhi = rd_frame_of(pre.data(), 0, (uint32_t)n - 1, rd_granule_last(T, q0));
            uint64_t acc = 0, def = 0, crw = 0;
            for (uint32_t lane = 0; lane < kRdGranule && q0 + lane < T; ++lane) {
                uint32_t j, f, r;
                const uint32_t status = rd_ordinal_record(*in, ws, tables, cfg, rlo, rhi, q0 + lane, &j, &f, &r).status;
                if (status == kRdAccept) {
                    acc |= 1ull << lane;
                    if (in->msg[f].instruction == kInsRecordCreate) crw |= 1ull << lane, ctrl.n_creates += 1;
                    else ctrl.n_deletes += 1;
                } else if (status == kRdDefer) {
                    def |= 1ull << lane;
                    ctrl.n_deferred_records += 1;
                } else {
                    (&ctrl.n_drop_walk)[status] += 1;
                    if (status == kRdFail) ctrl.error |= kRdErrWalk;
                }
            }
            words[kRdWords * (uint64_t)g] = acc, words[kRdWords * (uint64_t)g + 1] = def, words[kRdWords * (uint64_t)g + 2] = crw;
        }
    }
    // scans: the granules
    for (int creates = 0; creates < 2; ++creates) {
        const RdGranuleTerm term{words.data(), &pre[n], in->max_records, creates != 0};
        uint64_t run = 0;
        for (uint64_t g = 0; g < nG; ++g) (creates ? cbase : base)[g] = run, run += term(g);
    }
    // scan: the frames, bracketed block by block — each block's sum first, the blocks' prefix, then the
    // entries behind their block's prefix
    {
        const RdFrameTerm term{ws, in->db_src, n, in->max_records};
        const RdCombine op;
        const uint64_t nb = (n + 1 + blk - 1) / blk;
        std::vector<RdSum> bsum(nb);
        for (uint64_t b = 0; b < nb; ++b) {
            RdSum s = term(b * blk);
            for (uint64_t j = b * blk + 1; j < (b + 1) * blk && j <= n; ++j) s = op(s, term(j));
            bsum[b] = s;
        }
        RdSum before = rd_zero();
        for (uint64_t b = 0; b < nb; ++b) {
            RdSum local = rd_zero();
            for (uint64_t j = b * blk; j < (b + 1) * blk && j <= n; ++j) {
                ex[j] = op(before, local);
                local = op(local, term(j));
            }
            before = op(before, bsum[b]);
        }
    }
    // emit
    for (uint32_t w = 0; w < n_waves && n; ++w) {
        for (uint32_t g = w; g < nGa; g += n_waves) {
            if (!(words[kRdWords * (uint64_t)g] | words[kRdWords * (uint64_t)g + 1])) continue;
            const uint32_t q0 = g * kRdGranule;
            const uint32_t rlo = rd_frame_of(pre.data(), 0, (uint32_t)n - 1, q0);
            const uint32_t rhi = rd_frame_of(pre.data(), 0, (uint32_t)n - 1, rd_granule_last(T, q0));
            for (uint32_t lane = 0; lane < kRdGranule; ++lane) rd_emit_ordinal(*in, ws, tables, cfg, *out, g, lane, rlo, rhi);
        }
    }
    const RdFrameTerm own{ws, in->db_src, n, in->max_records};
    for (uint64_t i = 0; i < n; ++i)
        if (cls[i] != WQ_RCLS_SKIP)
            rd_emit_frame(*in, *out, in->db_src ? in->db_src[i] : (uint32_t)i, cls[i], after[i], ex[i], own(i));
    rd_finish(*in, *out, ex[n], pre[n], &ctrl);
    if (counters) *counters = ctrl;
    return 0;
}

#ifdef WQ_RECORDS_DISPATCH_SHIM_MAIN
// The stand-alone program: frames built here (a minimal Message writer: records with uuid, position, world,
// data and flex), random and hostile variations, every input and output on an exactly sized heap buffer.
#include <stdio.h>

#include <random>
#include <string>

namespace {

struct Builder {
    std::vector<uint8_t> b;
    void pad(size_t a) {
        while (b.size() % a) b.push_back(0);
    }
    void u16(uint16_t v) { b.push_back((uint8_t)v), b.push_back((uint8_t)(v >> 8)); }
    void u32(uint32_t v) {
        for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(v >> (8 * k)));
    }
    void put32(size_t at, uint32_t v) {
        for (int k = 0; k < 4; ++k) b[at + k] = (uint8_t)(v >> (8 * k));
    }
    // a string or byte vector at the end; the slot at `slot` points to it
    void bytes(size_t slot, const std::string& s) {
        pad(4);
        put32(slot, (uint32_t)(b.size() - slot));
        u32((uint32_t)s.size());
        b.insert(b.end(), s.begin(), s.end());
        b.push_back(0);
    }
    // a table: vtable of n_slots u16 entries, then the fields in slot order: 'o' an offset, 'p' 24 bytes, 'b' a byte
    // returns the table's position; field_at[k] receives where field k lies (0: absent)
    size_t table(const std::string& kinds, const std::vector<bool>& present, std::vector<size_t>* field_at) {
        pad(2);
        const size_t vt = b.size(), n = kinds.size();
        u16((uint16_t)(4 + 2 * n));
        u16(0);
        for (size_t k = 0; k < n; ++k) u16(0);
        pad(4);
        const size_t t = b.size();
        u32((uint32_t)(t - vt));  // soffset: the vtable precedes
        field_at->assign(n, 0);
        for (size_t k = 0; k < n; ++k) {
            if (!present[k]) continue;
            if (kinds[k] == 'o') pad(4);
            (*field_at)[k] = b.size();
            const uint16_t off = (uint16_t)(b.size() - t);
            b[vt + 4 + 2 * k] = (uint8_t)off, b[vt + 5 + 2 * k] = (uint8_t)(off >> 8);
            if (kinds[k] == 'o') u32(0);
            else if (kinds[k] == 'p') b.insert(b.end(), 24, 0);
            else b.push_back(0);
        }
        const uint16_t size = (uint16_t)(b.size() - t);
        b[vt + 2] = (uint8_t)size, b[vt + 3] = (uint8_t)(size >> 8);
        return t;
    }
};

struct Rec {
    std::string uuid, world, data, flex;
    bool has_pos, has_data, has_flex;
    double pos[3];
};

std::vector<uint8_t> frame(uint8_t ins, const std::string& param, bool has_param, const std::string& world, bool has_pos,
                           const double* pos, const std::vector<Rec>& recs) {
    Builder f;
    f.u32(0);
    std::vector<size_t> at;
    // Message: instruction, parameter, sender, world, replication, records, entities, position, flex
    const size_t root = f.table("boooboopo", {true, has_param, true, true, false, !recs.empty(), false, has_pos, false}, &at);
    f.put32(0, (uint32_t)root);
    f.b[at[0]] = ins;
    if (has_pos) memcpy(&f.b[at[7]], pos, 24);
    if (has_param) f.bytes(at[1], param);
    f.bytes(at[2], "00000000-0000-0000-0000-000000000001");
    f.bytes(at[3], world);
    if (!recs.empty()) {
        f.pad(4);
        f.put32(at[5], (uint32_t)(f.b.size() - at[5]));
        f.u32((uint32_t)recs.size());
        const size_t slots = f.b.size();
        for (size_t k = 0; k < recs.size(); ++k) f.u32(0);
        for (size_t k = 0; k < recs.size(); ++k) {
            const Rec& r = recs[k];
            std::vector<size_t> ra;
            const size_t t = f.table("opooo", {true, r.has_pos, true, r.has_data, r.has_flex}, &ra);
            f.put32(slots + 4 * k, (uint32_t)(t - (slots + 4 * k)));
            if (r.has_pos) memcpy(&f.b[ra[1]], r.pos, 24);
            f.bytes(ra[0], r.uuid);
            f.bytes(ra[2], r.world);
            if (r.has_data) f.bytes(ra[3], r.data);
            if (r.has_flex) f.bytes(ra[4], r.flex);
        }
    }
    f.pad(4);
    return f.b;
}

template <class T>
T* exact(const std::vector<T>& v) {  // a heap copy of exactly v.size() elements: one past is an overflow
    T* p = new T[v.size()];
    for (size_t k = 0; k < v.size(); ++k) p[k] = v[k];
    return p;
}

}  // namespace

int main() {
    using namespace wq;
    std::mt19937_64 rng(20241);
    const std::string names[] = {"world", "w00", "chat/server_1", "a b", "0bad", "", "@global", "elsewhere", std::string(70, 'x')};
    const std::string table_names = "worldw00chat_fs_server_1a_b";
    const uint32_t table_off[] = {0, 5, 8, 24, 27};
    const double coords[] = {0.0, -0.5, 17.0, 1e12, -40.0, 3.5};
    const std::string params[] = {"5", "+5", "", "+", "-1", "18446744073709551615", "8210298412799999", std::string(300, '0') + "7", "1 "};
    uint64_t runs = 0, ops = 0, errors = 0;
    for (int round = 0; round < 400; ++round) {
        const uint32_t n_frames = (uint32_t)(rng() % 70);
        std::vector<uint8_t> data;
        std::vector<uint64_t> fo{0};
        std::vector<wq_decoded_msg> msg(n_frames);
        std::vector<uint32_t> world(n_frames);
        std::vector<uint8_t> flags(n_frames);
        const DecList no_list{nullptr, nullptr, 0};
        for (uint32_t i = 0; i < n_frames; ++i) {
            std::vector<Rec> recs(rng() % 4 == 0 ? rng() % 150 : rng() % 5);
            for (Rec& r : recs) {
                char u[40];
                snprintf(u, sizeof(u), "%032llx", (unsigned long long)(rng() % 50));
                r.uuid = u, r.world = names[rng() % 9], r.data = "payload", r.flex = std::string(rng() % 9, '\x07');
                r.has_pos = rng() % 8 != 0, r.has_data = rng() % 2, r.has_flex = rng() % 2;
                for (double& c : r.pos) c = coords[rng() % 6];
            }
            const uint8_t ins = (uint8_t)(rng() % 5 == 0 ? 7 : (rng() % 3 == 0 ? 9 : rng() % 2 ? 8 : 11));
            double pos[3] = {coords[rng() % 6], 1.0, 2.0};
            const bool has_param = rng() % 2;
            const std::vector<uint8_t> f = frame(ins, params[rng() % 9], has_param, names[rng() % 9], rng() % 6 != 0, pos,
                                                 ins == 9 ? std::vector<Rec>() : recs);
            data.insert(data.end(), f.begin(), f.end());
            fo.push_back(data.size());
        }
        // hostile variations: a tick cut short, bytes overwritten, offsets that descend
        const int hostile = round % 4;
        if (hostile == 1 && !data.empty()) data.resize(data.size() - rng() % (data.size() < 64 ? data.size() : 64)), fo.back() = data.size();
        if (hostile == 2)
            for (int k = 0; k < 6 && !data.empty(); ++k) data[rng() % data.size()] = (uint8_t)rng();
        if (hostile == 3 && n_frames > 2) fo[1 + rng() % (n_frames - 1)] = rng() % (data.size() + 9);
        uint8_t* d_frames = exact(data);
        for (uint32_t i = 0; i < n_frames; ++i) {  // the decoder's arrays; a hostile tick keeps "OK" on frames that are not
            DecFrame df;
            uint64_t lo, size;
            uint32_t e = 0;
            memset(&df, 0, sizeof(df));
            df.m.status = WQ_DEC_INVALID_FLATBUFFER;
            if (dec_frame_span(fo.data(), i, n_frames, data.size(), &lo, &size, &e)) dec_frame(d_frames + lo, size, no_list, lo, i, &df);
            msg[i] = df.m;
            flags[i] = (uint8_t)((df.m.status == WQ_DEC_OK || hostile ? kDecOk : 0u) | (df.m.has_position ? kDecHasPos : 0u) |
                                 (df.m.has_parameter ? kDecHasParam : 0u) | (rng() % 9 == 0 ? kDecGlobal : 0u) |
                                 (rng() % 4 ? kDecWorldKnown : 0u));
            world[i] = rng() % 7 == 0 ? WQ_WORLD_INVALID : (uint32_t)(rng() % 4);
            if (hostile == 2 && rng() % 3 == 0) msg[i].param_off = (uint32_t)rng(), msg[i].world_len = (uint32_t)rng();
            if (hostile && rng() % 5 == 0) msg[i].instruction = (uint8_t)(8 + rng() % 4);
        }
        std::vector<uint32_t> db;
        for (uint32_t i = 0; i < n_frames; ++i)
            if (rng() % 8) db.push_back(hostile == 3 && rng() % 9 == 0 ? (uint32_t)rng() : i);
        std::vector<uint32_t> free_handles(rng() % 6);
        for (uint32_t& v : free_handles) v = (uint32_t)(rng() % 1000);
        wq_recdisp_in in;
        memset(&in, 0, sizeof(in));
        uint64_t* d_fo = exact(fo);
        wq_decoded_msg* d_msg = exact(msg);
        uint32_t* d_world = exact(world);
        uint8_t* d_flags = exact(flags);
        uint32_t* d_db = exact(db);
        uint32_t* d_free = exact(free_handles);
        in.frames = d_frames, in.frame_offsets = d_fo, in.n_frames = n_frames, in.n_frame_bytes = data.size();
        in.msg = d_msg, in.world = d_world, in.flags = d_flags;
        in.db_src = round % 7 == 0 ? nullptr : d_db, in.n_db = round % 7 == 0 ? n_frames : db.size();
        in.now_us = 1700000000000000ll, in.free_handles = d_free, in.n_free = (uint32_t)free_handles.size(), in.handle_next = 1000;
        in.max_records = round % 5 == 0 ? rng() % 40 : data.size() / 4;
        wq_test_recdisp_env env;
        memset(&env, 0, sizeof(env));
        uint8_t* d_names = exact(std::vector<uint8_t>(table_names.begin(), table_names.end()));
        uint32_t* d_off = exact(std::vector<uint32_t>(table_off, table_off + 5));
        env.world_bytes = d_names, env.world_off = d_off, env.n_worlds = round % 11 == 0 ? 0 : 4;
        env.size[0] = env.size[1] = env.size[2] = 16, env.table_size = 1024;
        env.n_waves = 1 + (uint32_t)(rng() % 9), env.scan_block = 1 + (uint32_t)(rng() % 9);
        // a sizing call, then exactly sized outputs
        wq_recdisp_out out;
        memset(&out, 0, sizeof(out));
        wq_recdisp_counters c;
        if (wq_test_records_dispatch_host(&in, &env, &out, &c)) return 1;
        const uint32_t n_ops = (uint32_t)(c.n_creates + c.n_deletes), n_def = (uint32_t)(c.n_deferred_records + c.n_read_deferred);
        out.ops_capacity = round % 3 == 0 ? n_ops / 2 : n_ops, out.defer_capacity = round % 3 == 1 ? n_def / 2 : n_def;
        out.runs_capacity = (uint32_t)c.n_runs + (round % 3 == 2 ? 0 : 1);
        out.cls = new uint8_t[in.n_db];
        out.ops = new wq_rec_op[out.ops_capacity], out.op_ref = new wq_rec_op_ref[out.ops_capacity];
        out.q_src = new uint32_t[c.n_read], out.q_world = new uint32_t[c.n_read];
        out.q_pos = new double[3 * c.n_read], out.q_after = new int64_t[c.n_read];
        out.defer = new wq_recdisp_defer[out.defer_capacity], out.runs = new wq_recdisp_run[out.runs_capacity];
        wq_recdisp_counters c2;
        if (wq_test_records_dispatch_host(&in, &env, &out, &c2)) return 1;
        c.overflow = c2.overflow;
        if (memcmp(&c, &c2, sizeof(c))) {
            fprintf(stderr, "round %d: the sizing call's counters differ\n", round);
            return 1;
        }
        runs += c.n_runs, ops += n_ops, errors += c.error != 0;
        delete[] out.cls, delete[] out.ops, delete[] out.op_ref, delete[] out.q_src, delete[] out.q_world, delete[] out.q_pos;
        delete[] out.q_after, delete[] out.defer, delete[] out.runs;
        delete[] d_frames, delete[] d_fo, delete[] d_msg, delete[] d_world, delete[] d_flags, delete[] d_db, delete[] d_free;
        delete[] d_names, delete[] d_off;
    }
    printf("400 rounds, %llu runs, %llu ops, %llu rounds with error bits\n", (unsigned long long)runs, (unsigned long long)ops,
           (unsigned long long)errors);
    return 0;
}
#endif
