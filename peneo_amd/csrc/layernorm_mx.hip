// LayerNorm forward that also emits the MX FP8 copy of its output (peneo_layernorm_fwd_mxfp8): the bf16 fast path of layernorm.hip
// (ln_fwd32_kernel: a 32-lane half-wave per row, lane hl holds the 8 consecutive columns (hl + 32 k) * 8 .. + 7, k < NV; the same
// arithmetic in the same order, so y, mean and rstd are bit for bit those of peneo_layernorm_fwd) followed by the row quantizer on the
// values AS ROUNDED TO bf16: an MX block of 32 columns is held by four consecutive lanes, its amax takes two exchanges, and a lane
// writes its 8 e4m3 bytes as one 8-byte store.  Used by the MXFP8 encoder-layer composite in place of peneo_layernorm_fwd +
// peneo_mxfp8_quantize_rows_bf16: the same bytes with one launch and one pass over the row less.
#include "common.h"
#include "mx_common.h"

namespace peneo {
namespace {

__device__ __forceinline__ float lnmx_half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int NV>
__global__ __launch_bounds__(256) void ln_fwd32_mx_kernel(const bf16_t* x, bf16_t* y, const float* gamma, const float* beta, float eps,
                                                          float* mean, float* rstd, int64_t rows, uint8_t* yq, uint8_t* ys) {
  constexpr int VEC = 8;
  constexpr int H = 32 * NV * VEC;
  const int hl = threadIdx.x & 31;
  const int64_t r = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (r >= rows) return;
  const bf16_t* xr = x + r * H;
  bf16_t* yr = y + r * H;
  float v[NV][VEC];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    unpack16<bf16_t>(*reinterpret_cast<const uint4*>(xr + (hl + 32 * k) * VEC), v[k]);
#pragma unroll
    for (int e = 0; e < VEC; ++e) s += v[k][e];
  }
  const float mu = lnmx_half_sum(s) * (1.0f / (float)H);
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int e = 0; e < VEC; ++e) { float d = v[k][e] - mu; q += d * d; }
  const float rs = rsqrtf(lnmx_half_sum(q) * (1.0f / (float)H) + eps);
  if (hl == 0) {
    if (mean) mean[r] = mu;
    if (rstd) rstd[r] = rs;
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c0 = (hl + 32 * k) * VEC;
    float gm[VEC], bt[VEC], o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; e += 4) {
      *reinterpret_cast<float4*>(gm + e) = *reinterpret_cast<const float4*>(gamma + c0 + e);
      *reinterpret_cast<float4*>(bt + e) = *reinterpret_cast<const float4*>(beta + c0 + e);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = (v[k][e] - mu) * rs * gm[e] + bt[e];
    *reinterpret_cast<uint4*>(yr + c0) = pack16<bf16_t>(o);
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < VEC; ++e) { o[e] = Elem<bf16_t>::round(o[e]); amax = fmaxf(amax, fabsf(o[e])); }
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    const uint32_t sb = mx_scale_byte(amax);
    const float inv = mx_inv_scale(sb);
    *reinterpret_cast<uint2*>(yq + r * H + c0) = make_uint2(mx_e4m3x4(o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv),
                                                            mx_e4m3x4(o[4] * inv, o[5] * inv, o[6] * inv, o[7] * inv));
    if ((hl & 3) == 0) ys[r * (H / 32) + (c0 >> 5)] = (uint8_t)sb;
  }
}

template <int NV>
void launch(hipStream_t st, const void* x, void* y, const float* gamma, const float* beta, float eps, float* mean, float* rstd,
            int64_t rows, void* yq, void* ys) {
  hipLaunchKernelGGL(ln_fwd32_mx_kernel<NV>, dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, st, static_cast<const bf16_t*>(x),
                     static_cast<bf16_t*>(y), gamma, beta, eps, mean, rstd, rows, static_cast<uint8_t*>(yq), static_cast<uint8_t*>(ys));
}

}  // namespace
}  // namespace peneo

using namespace peneo;

extern "C" int peneo_layernorm_mxfp8_supported(int H) { return H > 0 && H % 256 == 0 && H / 256 <= 4 ? 1 : 0; }

extern "C" int peneo_layernorm_fwd_mxfp8(const void* x, void* y, const float* gamma, const float* beta, float eps, float* mean,
                                         float* rstd, int64_t rows, int H, void* y_q, void* y_s, peneo_stream_t stream) {
  PENEO_REQUIRE(x && y && gamma && beta && y_q && y_s && rows > 0, "peneo_layernorm_fwd_mxfp8: bad arguments");
  PENEO_REQUIRE(peneo_layernorm_mxfp8_supported(H), "peneo_layernorm_fwd_mxfp8: H=%d not supported (peneo_layernorm_mxfp8_supported)", H);
  PENEO_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gamma) |
                  reinterpret_cast<uintptr_t>(beta)) & 15) == 0 && (reinterpret_cast<uintptr_t>(y_q) & 7) == 0,
                "peneo_layernorm_fwd_mxfp8: x / y / gamma / beta must be 16-byte aligned, y_q 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  switch (H / 256) {
    case 1: launch<1>(st, x, y, gamma, beta, eps, mean, rstd, rows, y_q, y_s); break;
    case 2: launch<2>(st, x, y, gamma, beta, eps, mean, rstd, rows, y_q, y_s); break;
    case 3: launch<3>(st, x, y, gamma, beta, eps, mean, rstd, rows, y_q, y_s); break;
    default: launch<4>(st, x, y, gamma, beta, eps, mean, rstd, rows, y_q, y_s); break;
  }
  return check_launch("peneo_layernorm_fwd_mxfp8");
}
