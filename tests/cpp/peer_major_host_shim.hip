// Test-only shim: runs the per-peer send lists' arithmetic (csrc/peer_major_ops.hpp: the row that
// covers an element, the clamped row bounds, the connected test, the key of an element with its
// sentinel, the key width and the per-peer lower bound) on the CPU in the shape the kernels use it —
// one key and one message per element of [0, n_pairs), a stable sort by key over the key's bits, one
// lower bound per peer — with std::stable_sort in place of rocPRIM, so the result is checked byte for
// byte against worldql_server_amd/interest.py without a GPU (tests/test_peer_major_cpp_mirror.py).
// The GPU instance is checked in tests/test_gpu_peers.py.
//
// With -DWQ_PEER_MAJOR_SHIM_MAIN the file is a program of its own: random and hostile offsets on
// exactly sized vectors, for a host build under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../worldql_server_amd/csrc/peer_major_ops.hpp"

// As wq_peer_major_device: offsets[n_msgs + 1] (not read when n_msgs == 0), peers[n_pairs],
// connected nullable; writes peer_offsets[n_peers + 1] and msgs_out[n_pairs].
extern "C" void wq_test_peer_major_host(const uint32_t* offsets, const uint32_t* peers, size_t n_msgs, size_t n_pairs,
                                        const uint32_t* connected, uint32_t n_peers, uint32_t* peer_offsets,
                                        uint32_t* msgs_out) {
    const uint32_t M = (uint32_t)n_msgs, P = (uint32_t)n_pairs;
    std::vector<uint32_t> key(P), msg(P), order(P), skey(P);
    for (uint32_t j = 0; j < P; ++j) key[j] = wq::pm_key(offsets, peers, M, P, connected, n_peers, j, &msg[j]);
    // the radix sort sees the low pm_key_bits of a key only
    const int bits = wq::pm_key_bits(n_peers);
    const uint32_t mask = bits >= 32 ? 0xFFFFFFFFu : (1u << bits) - 1u;
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t x, uint32_t y) { return (key[x] & mask) < (key[y] & mask); });
    for (uint32_t i = 0; i < P; ++i) {
        skey[i] = key[order[i]];
        msgs_out[i] = msg[order[i]];
    }
    for (uint64_t p = 0; p <= n_peers; ++p) peer_offsets[p] = wq::pm_lower_bound(skey.data(), P, (uint32_t)p);
}

#ifdef WQ_PEER_MAJOR_SHIM_MAIN
#include <stdio.h>

#include <map>
#include <random>

namespace {

// The contract for ascending offsets, restated with a map: per peer the rows that hold it.
int check_exact(const std::vector<uint32_t>& off, const std::vector<uint32_t>& peers, const std::vector<uint32_t>& conn,
                bool with_conn, uint32_t n_peers, const std::vector<uint32_t>& po, const std::vector<uint32_t>& mo) {
    const size_t M = off.empty() ? 0 : off.size() - 1, P = peers.size();
    std::map<uint32_t, std::vector<uint32_t>> want;
    for (size_t m = 0; m < M; ++m) {
        const size_t a = std::min<size_t>(off[m], P), b = std::min<size_t>(off[m + 1], P);
        for (size_t j = a; j < b; ++j) {
            const uint32_t p = peers[j];
            if (p < n_peers && (!with_conn || ((conn[p >> 5] >> (p & 31)) & 1u))) want[p].push_back((uint32_t)m);
        }
    }
    int bad = 0;
    uint32_t at = 0;
    for (uint64_t p = 0; p < n_peers; ++p) {
        bad += po[p] != at;
        const auto it = want.find((uint32_t)p);
        if (it == want.end()) continue;
        for (uint32_t m : it->second) bad += at >= P || mo[at++] != m;
    }
    bad += po[n_peers] != at;
    return bad;
}

// The clauses that hold whatever the offsets are.
int check_formed(size_t M, size_t P, uint32_t n_peers, const std::vector<uint32_t>& po,
                 const std::vector<uint32_t>& mo) {
    int bad = po[0] != 0 || po[n_peers] > P;
    for (uint64_t p = 0; p < n_peers; ++p) bad += po[p + 1] < po[p];
    for (size_t i = 0; i < std::min<size_t>(po[n_peers], P); ++i) bad += mo[i] >= M;
    for (size_t i = 0; i < P; ++i) bad += mo[i] >= std::max<size_t>(M, 1);
    return bad;
}

struct Run {
    std::vector<uint32_t> po, mo;
};

// Exactly sized buffers: the address sanitizer sees any read or write past an array.
Run run(const std::vector<uint32_t>& off, const std::vector<uint32_t>& peers, const std::vector<uint32_t>& conn,
        bool with_conn, uint32_t n_peers) {
    const size_t M = off.empty() ? 0 : off.size() - 1;
    Run r{std::vector<uint32_t>((size_t)n_peers + 1, 0xDEADBEEFu), std::vector<uint32_t>(peers.size(), 0xDEADBEEFu)};
    wq_test_peer_major_host(M ? off.data() : nullptr, peers.data(), M, peers.size(), with_conn ? conn.data() : nullptr,
                            n_peers, r.po.data(), r.mo.data());
    return r;
}

}  // namespace

int main() {
    std::mt19937_64 rng(11);
    const uint32_t lens[] = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 3000};
    const uint32_t npeers[] = {0, 1, 2, 31, 32, 33, 255, 256, 257, 1000, 65535, 65536};
    int bad = 0, runs = 0;
    for (int round = 0; round < 60; ++round) {
        const size_t M = round % 10 == 0 ? 0 : 1 + rng() % 300;
        const uint32_t n_peers = npeers[rng() % 12];
        std::vector<uint32_t> off{0}, peers;
        for (size_t m = 0; m < M; ++m) {
            const uint32_t n = lens[rng() % (round % 8 == 1 ? 11 : 10)];
            for (uint32_t i = 0; i < n; ++i) {
                const uint64_t r = rng();
                peers.push_back(r % 16 == 0 ? 0xFFFFFFFFu - (uint32_t)(r >> 8) % 2 : (uint32_t)(r >> 8) % (n_peers + 9));
            }
            off.push_back((uint32_t)peers.size());
        }
        if (M == 0) off.clear();
        const uint32_t full = (uint32_t)peers.size();
        // exactly ceil(n_peers / 32) words: a read past the last word is a read past the vector
        std::vector<uint32_t> conn((n_peers + 31) / 32);
        for (auto& w : conn) w = (uint32_t)rng();
        for (int with_conn = 0; with_conn < 2; ++with_conn) {
            // as routed, padded (elements behind offsets[M], also with M == 0), cut
            std::vector<uint32_t> padded = peers;
            for (int i = 0; i < 1000; ++i) padded.push_back((uint32_t)rng() % (n_peers + 1));
            std::vector<uint32_t> cut(peers.begin(), peers.begin() + (full ? rng() % full : 0));
            for (const auto* pv : {&peers, &padded, &cut}) {
                const Run r = run(off, *pv, conn, with_conn, n_peers);
                bad += check_exact(off, *pv, conn, with_conn, n_peers, r.po, r.mo);
                bad += check_formed(M, pv->size(), n_peers, r.po, r.mo);
                runs++;
            }
            if (M < 2) continue;
            // hostile offsets: descending, one descending pair, all 2^32 - 1, offsets[M] far past
            // n_pairs, sums wrapped mod 2^32, junk
            std::vector<std::vector<uint32_t>> hostile;
            std::vector<uint32_t> o = off;
            std::reverse(o.begin(), o.end());
            hostile.push_back(o);
            o = off;
            o[1 + rng() % (M - 1)] = full ? (uint32_t)(rng() % full) : 0u;
            hostile.push_back(o);
            hostile.push_back(std::vector<uint32_t>(M + 1, 0xFFFFFFFFu));
            o = off;
            o[M] = 0xFFFFFFF0u;
            hostile.push_back(o);
            o.assign(M + 1, 0u);
            for (size_t m = 0; m < M; ++m) o[m + 1] = o[m] + (uint32_t)(rng() % 40000000);  // wraps every ~200 rows
            hostile.push_back(o);
            for (auto& x : o) x = (uint32_t)rng() % (2 * full + 2);
            hostile.push_back(o);
            for (const auto& ho : hostile)
                for (const auto* pv : {&peers, &cut}) {
                    const Run r1 = run(ho, *pv, conn, with_conn, n_peers), r2 = run(ho, *pv, conn, with_conn, n_peers);
                    bad += check_formed(M, pv->size(), n_peers, r1.po, r1.mo);
                    bad += r1.po != r2.po || r1.mo != r2.mo;
                    runs++;
                }
        }
    }
    printf("peer_major host check: %d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
