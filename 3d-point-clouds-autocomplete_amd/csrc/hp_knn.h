// What the two neighbour searches share (knn.hip: brute force; knn_grid.hip: the same law behind a uniform grid): the squared
// distance of the law as its bit pattern, the mark of an empty slot / an absent candidate, and the sorted insertion.
#pragma once
#include "hp_common.h"

namespace hp_knn {

constexpr int kMaxK = 32;
constexpr unsigned kEmpty = 0xFFFFFFFFu;   // an empty slot, and the mask of an absent candidate

// The bits of d2 = ((dx*dx + dy*dy) + dz*dz) with d = q - p: every operation one fp32 rounding, no contraction.  With finite
// coordinates d2 is never NaN, so the bits order as unsigned integers, +inf (an overflow) included.
__device__ __forceinline__ unsigned d2_bits(float qx, float qy, float qz, float px, float py, float pz) {
    const float dx = __fsub_rn(qx, px), dy = __fsub_rn(qy, py), dz = __fsub_rn(qz, pz);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    return (unsigned)__float_as_int(d2);
}

// The mask a candidate carries in its fourth component: 0 for a present row, all ones for an absent one.
__device__ __forceinline__ float absent_mask(float x, float y, float z) {
    const bool ok = hp::finite_bits(x) && hp::finite_bits(y) && hp::finite_bits(z);
    return __int_as_float(ok ? 0 : (int)kEmpty);
}

// (nd, nj) into the sorted list behind every entry with d <= nd; the caller has seen nd < d[K-1].  For candidates that arrive
// in ascending row order: equal distances then stay in row order.
template <int K>
__device__ __forceinline__ void insert(unsigned (&d)[K], int (&j)[K], unsigned nd, int nj) {
#pragma unroll
    for (int t = K - 1; t > 0; --t) {
        if (d[t] > nd) {                                   // slot t takes its lower neighbour, or the newcomer
            const bool up = d[t - 1] > nd;
            d[t] = up ? d[t - 1] : nd;
            j[t] = up ? j[t - 1] : nj;
        }
    }
    if (d[0] > nd) {
        d[0] = nd;
        j[0] = nj;
    }
}

// The same chain on the full key (d, j) for candidates in any order; the caller has seen (nd, nj) < (d[K-1], j[K-1]).  An
// empty slot (kEmpty, -1) lies behind every key: no distance has these bits.
__device__ __forceinline__ bool key_above(unsigned d, int j, unsigned nd, int nj) { return d > nd || (d == nd && j > nj); }

template <int K>
__device__ __forceinline__ void insert_key(unsigned (&d)[K], int (&j)[K], unsigned nd, int nj) {
#pragma unroll
    for (int t = K - 1; t > 0; --t) {
        if (key_above(d[t], j[t], nd, nj)) {
            const bool up = key_above(d[t - 1], j[t - 1], nd, nj);
            d[t] = up ? d[t - 1] : nd;
            j[t] = up ? j[t - 1] : nj;
        }
    }
    if (key_above(d[0], j[0], nd, nj)) {
        d[0] = nd;
        j[0] = nj;
    }
}

// m_i of the outlier law from a sorted list: the fp64 sum of the roots in slot order over the valid slots among the first k,
// divided by their number, as fp32; +inf without a valid slot (or with an overflowed distance among them).
template <int K>
__device__ __forceinline__ float mean_root(const unsigned (&d)[K], int k) {
    double sum = 0.0;
    int c = 0;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        if (t < k && d[t] != kEmpty) {
            sum = __dadd_rn(sum, __dsqrt_rn((double)__int_as_float((int)d[t])));
            ++c;
        }
    }
    float m = __int_as_float((int)hp::kInfBits);
    if (c > 0) m = __double2float_rn(__ddiv_rn(sum, (double)c));
    return m;
}

}  // namespace hp_knn
