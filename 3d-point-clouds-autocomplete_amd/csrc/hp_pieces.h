// The device primitives of the split-f16 scheme: an fp32 operand as two f16 pieces under a power-of-two scale,
//   hi = f16(x 2^e), lo = f16(x 2^e - hi),  x = (hi + lo) 2^-e,
// three products per MFMA step on the f16 matrix pipe, operands staged global -> LDS by LDS-DMA.  Stated once, for conv_split.hip,
// conv_pp.hip, target_fused.hip, enc_bwd.hip, enc_bwd_f16.hip (with hp_enc_bwd_wprep.h) and the other 32x32 MFMA kernels'
// row map.  Internal; callers say `using namespace hp_pieces;` inside their own namespace.
#pragma once
#include <hip/hip_runtime.h>
#include "hp_conv_split.h"

// nothing moves across: pins a prefetch in front of the MFMA block that is to cover it
#define HP_SB() __builtin_amdgcn_sched_barrier(0)

namespace hp_pieces {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// The C/D row of accumulator register e (0..15) in lane half h (lane >> 5) of a 32x32 MFMA; the column is lane & 31.  A
// contraction may visit k in any order, so the same map is the k-permutation under which a finished accumulator tile is, as it
// stands, the next layer's B fragments (the chains of target_fused.hip and enc_bwd_f16.hip, the weight stream laid out for them).
__device__ __forceinline__ int cd_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// ---- scale exponents ------------------------------------------------------------------------------------------------
constexpr int kPieceTarget = 14;   // scaled maxima land in [2^13, 2^14): hi cannot overflow (f16 max 65504)

// exponent e of a float's frexp form v = f 2^e, f in [0.5, 1), from its bits (0 for zero / subnormal inputs)
__device__ __forceinline__ int frexp_exp(unsigned bits) {
    const int E = (int)((bits >> 23) & 0xff);
    return E ? E - 126 : 0;
}
// e with m 2^e in [2^13, 2^14) for the maximum m of what shares a scale (m = 0 or subnormal: the target itself).  Three policies:
// unclamped (conv_split.hip, target_fused.hip): `kPieceTarget - frexp_exp(bits)` as it stands, on the maximum's bits; 2^e and
// 2^-e go through pow2_clamped.  (Spelled at its sites: wrapped in a function, the compiler folds the constant the other way.)
// capped (conv_pp.hip): the exponent is stored with its P-format block; a block whose maximum is below 2^-40 keeps
// HP_PP_EXP_MAX (it only loses bits below 2^-79), so the readers' 2^-e is a normal float
__device__ __forceinline__ int block_exp(float m) { return min(kPieceTarget - frexp_exp(__float_as_uint(m)), HP_PP_EXP_MAX); }
// +-100 (hp_wprep, enc_bwd_f16.hip): 2^e and 2^-e are both normal floats, and sums of two exponents stay in pow2_exact's range
__device__ __forceinline__ int scale_exp(float m) { return max(-100, min(100, kPieceTarget - frexp_exp(__float_as_uint(m)))); }

// 2^e, e clamped into the normal range
__device__ __forceinline__ float pow2_clamped(int e) {
    e = max(-126, min(127, e));
    return __uint_as_float((unsigned)(e + 127) << 23);
}
// 2^e for an e the caller knows to be in [-126, 127]
__device__ __forceinline__ float pow2_exact(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }

// ---- pieces ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pack2(_Float16 a, _Float16 b) { return __builtin_bit_cast(unsigned, f16x2{a, b}); }
// the lo pieces of two values whose hi pieces are packed in `hpk`: lo = f16(x - f32(hi)) in ONE instruction each (v_fma_mix
// takes the f16 operand as it is; through C++ the compiler emits cvt + sub + cvt: 3 of the ~9 vector instructions per output
// element of a store epilogue that the matrix cores sit idle behind)
__device__ __forceinline__ unsigned lo_pair(float x0, float x1, unsigned hpk) {
    unsigned d;
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(d)
        : "v"(x0), "v"(x1), "v"(hpk));
    return d;
}
// the same under the scale sc (a power of two), the multiply folded in: hi = f16(x sc), then lo = f16(x sc - hi)
__device__ __forceinline__ unsigned hi_pair_s(float x0, float x1, float sc) {
    unsigned d;
    asm("v_fma_mixlo_f16 %0, %1, %3, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %2, %3, 0 op_sel_hi:[0,0,0]"
        : "=&v"(d)
        : "v"(x0), "v"(x1), "v"(sc));
    return d;
}
__device__ __forceinline__ unsigned lo_pair_s(float x0, float x1, float sc, unsigned hpk) {
    unsigned d;
    asm("v_fma_mixlo_f16 %0, %1, %3, -%4 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %0, %2, %3, -%4 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(d)
        : "v"(x0), "v"(x1), "v"(sc), "v"(hpk));
    return d;
}
// 8 scaled values -> the hi and the lo fragment of a lane
__device__ __forceinline__ void split8(const float (&y)[8], f16x8& hi, f16x8& lo) {
    u32x4 H, L;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        H[i] = pack2((_Float16)y[2 * i], (_Float16)y[2 * i + 1]);
        L[i] = lo_pair(y[2 * i], y[2 * i + 1], H[i]);
    }
    hi = __builtin_bit_cast(f16x8, H);
    lo = __builtin_bit_cast(f16x8, L);
}
// the hi and lo fragments of 8 values under the scale sc: one v_fma_mix per piece and value
__device__ __forceinline__ void split8s(const float (&x)[8], float sc, f16x8& hi, f16x8& lo) {
    u32x4 H, L;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned hh = hi_pair_s(x[2 * i], x[2 * i + 1], sc);
        H[i] = hh;
        L[i] = lo_pair_s(x[2 * i], x[2 * i + 1], sc, hh);
    }
    hi = __builtin_bit_cast(f16x8, H);
    lo = __builtin_bit_cast(f16x8, L);
}
// hi / lo pieces of 4 values under sc, packed: 8 bytes each
__device__ __forceinline__ void split4s(const f32x4& x, float sc, uint2& hi, uint2& lo) {
    unsigned hh[2], ll[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        hh[i] = hi_pair_s(x[2 * i], x[2 * i + 1], sc);
        ll[i] = lo_pair_s(x[2 * i], x[2 * i + 1], sc, hh[i]);
    }
    hi = make_uint2(hh[0], hh[1]);
    lo = make_uint2(ll[0], ll[1]);
}

// ---- LDS-DMA, 16 bytes per lane, the LDS destination wave-uniform + 16 * lane ---------------------------------------
// Through inline asm: with the builtin, hipcc orders every later ds_read behind the pending LDS write with an
// s_waitcnt vmcnt(0), i.e. it drains the prefetch the moment it is issued (measured in round 2, tools/micro/gemm_glds.hip).
// The asm form is invisible to that analysis; the explicit vmcnt(0) + barrier at the top of a k-tile orders the reads.
// glds16s: the address as a wave-uniform base + a 32-bit lane offset, and the LDS destination as an SGPR base + a LITERAL: the
// sum is formed into m0 inside the asm (a compiler-visible sum gets hoisted out of the k-loop as a loop invariant, runs out of
// SGPRs, is spilled to VGPR lanes and comes back as a v_readlane — a VALU instruction in a load phase, see conv_pp_kernel)
template <int LIT>
__device__ __forceinline__ void glds16s(const void* sbase, unsigned voff, unsigned lds_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_add_u32 m0, %3, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_base), "n"(LIT)
                 : "memory", "scc");
}
// glds16v: a full address per lane (a VGPR pair), the LDS destination in an SGPR
__device__ __forceinline__ void glds16v(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst)
                 : "memory");
}
// glds16u: a wave-uniform base + a 32-bit lane offset, the LDS destination in an SGPR
__device__ __forceinline__ void glds16u(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst)
                 : "memory");
}

}  // namespace hp_pieces
