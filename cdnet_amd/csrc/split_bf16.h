// The fp32 precision mode's operand split and its three-MFMA product (conv32.hip:1-7 is the long explanation).  Device code only.
//     hi = bf16(x), lo = bf16(x - hi), both round to nearest even: |x - hi| <= 2^-9 |x| and |x - hi - lo| <= 2^-18 |x|
//     a b ~= a_lo b_hi + a_hi b_lo + a_hi b_hi: the dropped a_lo b_lo is at most 2^-18 |a b|, the two operands' own errors another
//     2^-18 |a b| each - below 2^-16 |a b| per product, before the fp32 accumulation of the MFMA.
#pragma once
#include <hip/hip_runtime.h>
#include "vec.h"

namespace cdnet {

// 8 fp32 values -> hi / lo bf16 words (packed pairs: v_cvt_pk_bf16_f32; the pair's subtraction is one v_pk_add_f32)
__device__ __forceinline__ void split8(const float *v, u32x4 &hi, u32x4 &lo) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const f32x2 x = {v[2 * k], v[2 * k + 1]};
        const bf16x2 h = __builtin_convertvector(x, bf16x2);
        const unsigned hb = __builtin_bit_cast(unsigned, h);
        const f32x2 hf = {__builtin_bit_cast(float, hb << 16), __builtin_bit_cast(float, hb & 0xffff0000u)};
        const bf16x2 l = __builtin_convertvector(x - hf, bf16x2);
        hi[k] = hb;
        lo[k] = __builtin_bit_cast(unsigned, l);
    }
}

// The same values with the two subtractions of a pair kept scalar (inline assembly): left to the compiler they become one v_pk_add_f32,
// and a packed fp32 instruction costs a mover wave far more than two plain ones beside the consumers' MFMA stream (wgrad_ws32_kernel:
// 257 -> 241 us on the 64 -> 64 layer at 256 x 256 x 16).  For the kernels whose staging waves run next to MFMA waves: conv32ws.hip's
// movers and the fp32 weight-gradient kernels of wgrad.hip.
__device__ __forceinline__ void split8_scalar(const float *v, u32x4 &hi, u32x4 &lo) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const f32x2 x = {v[2 * k], v[2 * k + 1]};
        const bf16x2 h = __builtin_convertvector(x, bf16x2);
        const unsigned hb = __builtin_bit_cast(unsigned, h);
        float d0, d1;
        asm("v_sub_f32 %0, %1, %2" : "=v"(d0) : "v"(x[0]), "v"(__builtin_bit_cast(float, hb << 16)));
        asm("v_sub_f32 %0, %1, %2" : "=v"(d1) : "v"(x[1]), "v"(__builtin_bit_cast(float, hb & 0xffff0000u)));
        const f32x2 d = {d0, d1};
        hi[k] = hb;
        lo[k] = __builtin_bit_cast(unsigned, __builtin_convertvector(d, bf16x2));
    }
}

// acc + a b in the canonical order, small terms first: a_lo b_hi, a_hi b_lo, a_hi b_hi.  Kernels that spread the three MFMAs over other
// work on purpose (conv32ws.hip's consumers, wgrad_ws32_kernel) keep the order and write them out.
__device__ __forceinline__ f32x16 mfma3(f32x16 acc, bf16x8 a_hi, bf16x8 a_lo, bf16x8 b_hi, bf16x8 b_lo) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, acc, 0, 0, 0);
}

}  // namespace cdnet
