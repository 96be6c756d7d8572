// The clang vector types of the kernels, once.  Register staging types: HIP's float4 / uint4 structs defeat SROA, these do not.
#pragma once

namespace cdnet {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;      // one MFMA operand (v_mfma_f32_32x32x16_bf16)
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;      // one MFMA accumulator
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;     // 16 bytes of operand words
typedef __attribute__((ext_vector_type(4))) float f32x4;

// 16-bit integer and half views of the same words (xform.h's packed ReLU / fp16 loads, the transposing LDS reads of wgrad.hip and conv.hip)
typedef __attribute__((ext_vector_type(2))) short s16x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 h16x2;

}  // namespace cdnet
