// The bf16x3 operand split, shared by the f32 GEMM's SPLIT = 1 main loop (gemm_f32.inc) and
// the resident f32 attention's "high" kernels (attention.hip):
//   hi = bf16_rne(x),  lo = bf16_rne(x - float(hi))     (the subtraction is exact in f32)
#pragma once
#include "common.hpp"

// two f32 -> packed bf16 pair (RNE)
__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float sub_f32(float a, float b) {  // one v_sub_f32, never SLP-packed
  float r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
typedef uint32_t u32x4_ __attribute__((ext_vector_type(4)));
// the 8 values x0[0..3], x1[0..3] -> hi / lo bf16x8 operands, element j = 4h + t of x_h[t].
// PAD = 1: the wait states the compiler does not insert around an asm statement, whose instructions it does not
// model -- one between a transcendental (v_exp_f32) writing a value and the first conversion reading it, two
// between the last conversion and an MFMA reading the packs.  For callers whose inputs come straight from exp2 and
// whose packs feed an MFMA at once (attention's P); the GEMM's fragments come from LDS reads, which are waited for
// through the operands, and its form (PAD = 0) is the code it has always had.
template <int PAD = 0>
__device__ __forceinline__ void split8(const f32x4& x0, const f32x4& x1, bf16x8& hi, bf16x8& lo) {
  f32x4 y0 = x0, y1 = x1;
  if constexpr (PAD) asm("s_nop 0" : "+v"(y0), "+v"(y1));
  const float x[8] = {y0[0], y0[1], y0[2], y0[3], y1[0], y1[1], y1[2], y1[3]};
  u32x4_ H, L;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float a = x[2 * p], b = x[2 * p + 1];
    H[p] = cvt_pk_bf16(a, b);
    const float ah = __uint_as_float(H[p] << 16), bh = __uint_as_float(H[p] & 0xffff0000u);
    L[p] = cvt_pk_bf16(sub_f32(a, ah), sub_f32(b, bh));
  }
  if constexpr (PAD) asm("s_nop 1" : "+v"(H), "+v"(L));
  hi = __builtin_bit_cast(bf16x8, H);
  lo = __builtin_bit_cast(bf16x8, L);
}
