// OCP-MX FP8 quantization helpers shared by the MXFP8 kernels (pair_heads_mx.hip, gemm_mx.hip): blocks of 32 consecutive elements,
// scale 2^e with e = floor(log2 amax) - 8 clamped to [-127, 127] (E8M0 byte e + 127; an all-zero block gets byte 0), elements
// e4m3fn(RNE(clamp(v / 2^e, -448, 448))).  See the comment block of pair_heads_mx.hip for the measured converter behaviour.
#pragma once
#include "common.h"

namespace peneo {

typedef int i32x8_t __attribute__((ext_vector_type(8)));

// E8M0 byte of a block with maximum magnitude amax (>= 0): max(floor(log2 amax) - 8, -127) + 127, read off the exponent field
__device__ __forceinline__ uint32_t mx_scale_byte(float amax) {
  const int e = (int)((__float_as_uint(amax) >> 23) & 255u) - 8;
  return (uint32_t)(e < 0 ? 0 : e);
}
// 1 / 2^(byte - 127), exact (byte <= 247)
__device__ __forceinline__ float mx_inv_scale(uint32_t byte) { return __uint_as_float((254u - byte) << 23); }
// four values (already divided by the block scale) -> four e4m3 bytes, little-endian in order
__device__ __forceinline__ uint32_t mx_e4m3x4(float v0, float v1, float v2, float v3) {
  v0 = fminf(fmaxf(v0, -448.f), 448.f); v1 = fminf(fmaxf(v1, -448.f), 448.f);
  v2 = fminf(fmaxf(v2, -448.f), 448.f); v3 = fminf(fmaxf(v3, -448.f), 448.f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(v0, v1, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(v2, v3, w, true);
  return (uint32_t)w;
}
// one block of 32 values -> 8 dwords of e4m3 + its E8M0 byte
__device__ __forceinline__ uint32_t mx_quantize32(const float (&v)[32], uint32_t (&q)[8]) {
  float amax = 0.f;
#pragma unroll
  for (int t = 0; t < 32; ++t) amax = fmaxf(amax, fabsf(v[t]));
  const uint32_t sb = mx_scale_byte(amax);
  const float inv = mx_inv_scale(sb);
#pragma unroll
  for (int w = 0; w < 8; ++w) q[w] = mx_e4m3x4(v[4 * w] * inv, v[4 * w + 1] * inv, v[4 * w + 2] * inv, v[4 * w + 3] * inv);
  return sb;
}

}  // namespace peneo
