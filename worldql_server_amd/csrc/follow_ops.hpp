// follow_ops.hpp — the per-peer arithmetic of the follow path (wq_follow.hip): the packed axis
// masks of one peer's old and new neighbourhood, the closed-form op counts, and the decode of an
// op's ordinal into its offset. __host__ __device__, so tests/cpp/follow_host_shim.hip runs the
// same code on the CPU against worldql_server_amd/follow.py.
#pragma once

#include "../../include/wq_router.h"
#include "wq_device.hpp"

#pragma clang fp contract(off)

namespace wq {

// Packed masks of one peer: axis a at bits [20a, 20a + 20) = old distinct | old present << 5 |
// new distinct << 10 | new present << 15, one bit per offset index j = d + r (r <= 2: 5 bits).
// distinct: the first offset of its list with this quantised value; present (a subset of distinct):
// the other list holds the value too, and both states are in the same world.
constexpr int kFollowNewShift = 10;  // axis_bits >> 10: the new side's {distinct, present}

__host__ __device__ __forceinline__ uint32_t axis_bits(uint64_t m, int ax) {
    return (uint32_t)(m >> (20 * ax)) & 0xFFFFFu;
}

template <int R>
__host__ __device__ __forceinline__ uint32_t axis_masks(double po, double pn, bool old_ok, bool new_ok, bool same,
                                                         double sf, int64_t si) {
    constexpr int r = R / 2;
    int64_t vo[R], vn[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const double off = sf * (double)(j - r);  // exact
        vo[j] = coord_clamp_dev(po + off, sf, si);
        vn[j] = coord_clamp_dev(pn + off, sf, si);
    }
    uint32_t d_o = 0, d_n = 0, i_o = 0, i_n = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        bool first_o = true, first_n = true, in_n = false, in_o = false;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (k < j) {
                first_o = first_o && vo[k] != vo[j];
                first_n = first_n && vn[k] != vn[j];
            }
            in_n = in_n || vo[j] == vn[k];
            in_o = in_o || vn[j] == vo[k];
        }
        d_o |= (uint32_t)(first_o && old_ok) << j;
        d_n |= (uint32_t)(first_n && new_ok) << j;
        i_o |= (uint32_t)(first_o && old_ok && in_n && same) << j;
        i_n |= (uint32_t)(first_n && new_ok && in_o && same) << j;
    }
    return d_o | (i_o << 5) | (d_n << 10) | (i_n << 15);
}

template <int R>
__host__ __device__ __forceinline__ uint64_t peer_masks(uint32_t ow, const double* po, uint32_t nw, const double* pn,
                                                         double sf, int64_t si) {
    const bool old_ok = ow != kWorldEmpty, new_ok = nw != kWorldEmpty, same = old_ok && new_ok && ow == nw;
    uint64_t m = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
        m |= (uint64_t)axis_masks<R>(po[ax], pn[ax], old_ok, new_ok, same, sf, si) << (20 * ax);
    return m;
}

// Ops of one side (shift 0: the unsubscribes, from the old masks; kFollowNewShift: the subscribes):
// |side| - |side ∩ other| = prod |distinct_ax| - prod |present_ax|.
__host__ __device__ __forceinline__ uint32_t side_count(uint64_t m, int shift) {
    uint32_t all = 1, both = 1;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const uint32_t b = axis_bits(m, ax) >> shift;
        all *= (uint32_t)__builtin_popcount(b & 31u);
        both *= (uint32_t)__builtin_popcount((b >> 5) & 31u);
    }
    return all - both;
}

// The k-th op of one side of one peer -> its offset indices (jx, jy, jz): lexicographic order over
// the distinct offsets, skipping the cubes the other side holds too (present on all three axes).
// Selects only, no indexed arrays: nothing goes to scratch.
template <int R>
__host__ __device__ __forceinline__ void decode_op(uint64_t m, int shift, uint32_t k, int (&j)[3]) {
    uint32_t D[3], I[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const uint32_t b = axis_bits(m, ax) >> shift;
        D[ax] = b & 31u;
        I[ax] = (b >> 5) & 31u;
    }
    const uint32_t ny = (uint32_t)__builtin_popcount(D[1]), nz = (uint32_t)__builtin_popcount(D[2]);
    const uint32_t iy = (uint32_t)__builtin_popcount(I[1]), iz = (uint32_t)__builtin_popcount(I[2]);
    bool done = false, xin = false, yin = false;
    j[0] = j[1] = j[2] = 0;
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const bool in = (I[0] >> t) & 1u;
        const uint32_t c = ((D[0] >> t) & 1u) ? ny * nz - (in ? iy * iz : 0u) : 0u;
        const bool take = !done && k < c;
        j[0] = take ? t : j[0];
        xin = take ? in : xin;
        k -= (done || take) ? 0u : c;
        done = done || take;
    }
    done = false;
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const bool in = (I[1] >> t) & 1u;
        const uint32_t c = ((D[1] >> t) & 1u) ? nz - ((xin && in) ? iz : 0u) : 0u;
        const bool take = !done && k < c;
        j[1] = take ? t : j[1];
        yin = take ? in : yin;
        k -= (done || take) ? 0u : c;
        done = done || take;
    }
    const uint32_t Z = (xin && yin) ? (D[2] & ~I[2]) : D[2];
    done = false;
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const uint32_t c = (Z >> t) & 1u;
        const bool take = !done && k < c;
        j[2] = take ? t : j[2];
        k -= (done || take) ? 0u : c;
        done = done || take;
    }
}

// Op ordinal k of a peer (unsubscribes first) -> the five 8-byte words of its wq_op: world | peer
// << 32, kind (key_is_raw 0 and the padding zero), the offset position p + s*d.
template <int R>
__host__ __device__ __forceinline__ void make_op(uint64_t m, uint32_t k, uint32_t peer, uint32_t ow, const double* po,
                                                 uint32_t nw, const double* pn, double sf, uint64_t* o) {
    constexpr int r = R / 2;
    const uint32_t n_un = side_count(m, 0);
    const bool sub = k >= n_un;
    int j[3];
    decode_op<R>(m, sub ? kFollowNewShift : 0, sub ? k - n_un : k, j);
    o[0] = (uint64_t)(sub ? nw : ow) | ((uint64_t)peer << 32);
    o[1] = sub ? (uint64_t)WQ_OP_SUBSCRIBE : (uint64_t)WQ_OP_UNSUBSCRIBE;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const double v = (sub ? pn[ax] : po[ax]) + sf * (double)(j[ax] - r);
        uint64_t bits;
        __builtin_memcpy(&bits, &v, 8);
        o[2 + ax] = bits;
    }
}

}  // namespace wq
