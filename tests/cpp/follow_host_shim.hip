// Test-only shim: runs the follow path's per-peer arithmetic (csrc/follow_ops.hpp: axis masks,
// closed-form counts, ordinal -> op decode) on the CPU in the shape the kernels use it — count per
// peer, exclusive prefix, then every op found from its index by a search in the prefix — so the op
// stream is checked byte for byte against worldql_server_amd/follow.py without a GPU
// (tests/test_follow_cpp_mirror.py). The GPU instance is checked in tests/test_gpu_follow.py.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../worldql_server_amd/csrc/follow_ops.hpp"

namespace {

template <int R>
size_t run(const uint32_t* ow, const double* po, const uint32_t* nw, const double* pn, size_t n, uint16_t s,
           uint64_t* out, size_t capacity, uint64_t* n_unsub) {
    const double sf = (double)s;
    std::vector<uint64_t> mask(n);
    std::vector<size_t> off(n + 1, 0);
    uint64_t un = 0;
    for (size_t i = 0; i < n; ++i) {
        mask[i] = wq::peer_masks<R>(ow[i], po + 3 * i, nw[i], pn + 3 * i, sf, (int64_t)s);
        const uint32_t u = wq::side_count(mask[i], 0), v = wq::side_count(mask[i], wq::kFollowNewShift);
        un += u;
        off[i + 1] = off[i] + u + v;
    }
    *n_unsub = un;
    const size_t total = off[n];
    if (total > capacity) return total;
    for (size_t g = 0; g < total; ++g) {
        size_t lo = 0, hi = n;  // the last peer with off[p] <= g
        while (hi - lo > 1) {
            const size_t mid = (lo + hi) / 2;
            if (off[mid] <= g) lo = mid;
            else hi = mid;
        }
        wq::make_op<R>(mask[lo], (uint32_t)(g - off[lo]), (uint32_t)lo, ow[lo], po + 3 * lo, nw[lo], pn + 3 * lo, sf,
                       out + 5 * g);
    }
    return total;
}

}  // namespace

// Returns the op count (ops written only if it fits `capacity`); out: 5 u64 words per op.
extern "C" size_t wq_test_follow_ops_host(const uint32_t* ow, const double* po, const uint32_t* nw, const double* pn,
                                          size_t n, uint16_t s, uint32_t reach, uint64_t* out, size_t capacity,
                                          uint64_t* n_unsub) {
    switch (reach) {
        case 0: return run<1>(ow, po, nw, pn, n, s, out, capacity, n_unsub);
        case 1: return run<3>(ow, po, nw, pn, n, s, out, capacity, n_unsub);
        default: return run<5>(ow, po, nw, pn, n, s, out, capacity, n_unsub);
    }
}
