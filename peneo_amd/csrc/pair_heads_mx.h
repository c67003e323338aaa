// What the MXFP8 forward kernels of the pair-classifier heads share (pair_heads_mx.hip: D <= 512, eight waves;
// pair_heads_mx_wide.hip: 512 < D <= 1024, four waves): the packed slab and its two pack kernels, the launch parameters, and the
// epilogue that turns a logits^T accumulator of 32 pairs into logits and the workgroup's row of class-weighted CE partial sums.
// Everything is a template over the number of waves that share a slab (it sets the slab's padding) or has internal linkage, so
// each of the two files gets its own copy.
#pragma once
#include <type_traits>

#include "common.h"
#include "mx_common.h"

namespace peneo {
namespace {

constexpr int MX_NCP = 16;
constexpr float NEG_INF_MX = -3.0e38f;

// Packed slab (32 hidden rows of W1cat, 16-byte aligned parts):
//   KS8 = D / 64 first-layer fragments of 2 KiB: byte (c * 1024 + lane * 16 + t) of fragment ks =
//        e4m3(W1cat[slab * 32 + (lane & 31)][64 ks + 32 c + 16 (lane >> 5) + t])        (c = K-block of the step, t = 0..15)
//   NSW = ceil(KS8 / 4) scale words of 256 B: byte (ks & 3) of word [ks >> 2][lane] = E8M0 of row slab * 32 + (lane & 31),
//        block 2 ks + (lane >> 5)
//   2 bf16 second-layer fragments of 1 KiB (the bf16 pack's fragments KS, KS + 1: pack_weights_kernel)
// padded to a whole number of 1 KiB DMA pieces per wave of the NW-wave workgroup that streams it.
__host__ __device__ constexpr int mx_scale_words(int ks8) { return (ks8 + 3) / 4; }
__host__ __device__ constexpr int mx_payload(int ks8) { return ks8 * 2048 + mx_scale_words(ks8) * 256 + 2048; }
template <int NW> __host__ __device__ constexpr int mx_upw_t(int ks8) { return (mx_payload(ks8) + NW * 1024 - 1) / (NW * 1024); }
template <int NW> __host__ __device__ constexpr int mx_slab_bytes_t(int ks8) { return mx_upw_t<NW>(ks8) * NW * 1024; }

struct MxPackSrc {
  const float* w1[PENEO_MAX_HEADS];
  const float* w2[PENEO_MAX_HEADS];
  int classes[PENEO_MAX_HEADS];
  int num_heads, D;
};

// first layer: one thread per (row of W1cat, 32-element block); the buffer has been zeroed (padding, unused scale bytes)
template <int NW>
__global__ __launch_bounds__(256) void mx_pack_w1_kernel(MxPackSrc s, char* out) {
  const int D = s.D, ks8 = D / 64, nblk = D / 32;
  const int64_t total = (int64_t)s.num_heads * D * nblk;
  const int64_t slab_bytes = mx_slab_bytes_t<NW>(ks8);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / nblk), kb = (int)(i % nblk);
    const int h = row / D;
    const float* src = s.w1[h] + (int64_t)(row - h * D) * D + 32 * kb;
    float v[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) v[t] = src[t];
    uint32_t w[8];
    const uint32_t sb = mx_quantize32(v, w);
    char* slab = out + (int64_t)(row >> 5) * slab_bytes;
    const int ks = kb >> 1, c = kb & 1, r = row & 31;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)   // elements 16 hh .. 16 hh + 15 of the block sit in lane r + 32 hh
      *reinterpret_cast<uint4*>(slab + ks * 2048 + c * 1024 + (r + 32 * hh) * 16) = make_uint4(w[4 * hh], w[4 * hh + 1], w[4 * hh + 2], w[4 * hh + 3]);
    slab[ks8 * 2048 + (ks >> 2) * 256 + (r + 32 * c) * 4 + (ks & 3)] = (char)sb;
  }
}

// second layer: the bf16 pack's two W2 fragments per slab (pack_weights_kernel, fragments KS and KS + 1)
template <int NW>
__global__ __launch_bounds__(256) void mx_pack_w2_kernel(MxPackSrc s, char* out) {
  const int D = s.D, ks8 = D / 64;
  const int nslab = s.num_heads * D / 32;
  const int64_t slab_bytes = mx_slab_bytes_t<NW>(ks8);
  const int64_t total = (int64_t)nslab * 2 * 64 * 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63), kk = (int)((i >> 9) & 1), slab = (int)(i >> 10);
    const int cls = lane & 31;
    const int hidden = slab * 32 + 16 * kk + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
    const int h = hidden / D;
    int off = 0;
    for (int q = 0; q < h; ++q) off += s.classes[q];
    float v = 0.f;
    if (cls >= off && cls < off + s.classes[h]) v = s.w2[h][(int64_t)(cls - off) * D + (hidden - h * D)];
    bf16_t* dst = reinterpret_cast<bf16_t*>(out + slab * slab_bytes + ks8 * 2048 + mx_scale_words(ks8) * 256 + kk * 1024 + lane * 16);
    dst[e] = f32_to_bf16(v);
  }
}

inline unsigned mx_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

struct MxFwdParams {
  const bf16_t* ab; int B, N, D; int64_t P;
  int num_heads; int classes[PENEO_MAX_HEADS];
  const char* wp; const float* b1; const float* b2;
  float* logits[PENEO_MAX_HEADS];
  const int64_t* tags[PENEO_MAX_HEADS];
  const float* cw[PENEO_MAX_HEADS];
  float* partials;   // [B * gridDim.x][32]: num[8] | den[8] | dl_sum[16] per workgroup (peneo_loss_finish)
};

template <int I, int N, typename F>
__device__ __forceinline__ void mx_static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); mx_static_for<I + 1, N>(f); }
}
__device__ __forceinline__ float mx_cls_at(const float (&cls)[MX_NCP], int idx) {
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < MX_NCP; ++c) v = (c == idx) ? cls[c] : v;
  return v;
}

// logits^T accumulator -> per-pair logits and the class-weighted CE partial row of the workgroup (the bf16 kernel's epilogue
// without dropout scale and dlogits stores; dl_sum is still summed, so peneo_loss_finish reads the same row format).
// NW: waves of the workgroup.  ADD (a constant: the plain form keeps its statements): the row receives a further 32 pairs per wave
// of the same workgroup (the four-wave kernel holds two groups of 32 pairs a wave): the row's own writers add to what they stored
// the call before.  (Adding the two groups' terms in registers in front of ONE reduction was tried: with the lane part and the row
// part as two functions the eight-wave kernels came out with another register allocation, and they are to stay as they were.)
template <int NW, bool ADD = false>
__device__ __forceinline__ void mx_epilogue(const MxFwdParams& p, const f32x16_t& lg, char* smem, int tid, int lane, int wave,
                                            int half, int b, int64_t mypair, bool pair_ok) {
  float mine[8], other[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) { mine[r] = lg[r]; other[r] = __shfl_xor(lg[r], 32, 64); }
  float cls[MX_NCP];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    cls[c] = half == 0 ? mine[c] : other[c];
    cls[4 + c] = half == 0 ? other[c] : mine[c];
    cls[8 + c] = half == 0 ? mine[4 + c] : other[4 + c];
    cls[12 + c] = half == 0 ? other[4 + c] : mine[4 + c];
  }
  float num[PENEO_MAX_HEADS], den[PENEO_MAX_HEADS], dls[MX_NCP];
#pragma unroll
  for (int h = 0; h < PENEO_MAX_HEADS; ++h) { num[h] = 0.f; den[h] = 0.f; }
#pragma unroll
  for (int c = 0; c < MX_NCP; ++c) dls[c] = 0.f;
  const bool writer = pair_ok && half == 0;
  int off = 0;
#pragma unroll
  for (int h = 0; h < PENEO_MAX_HEADS; ++h) {
    if (h < p.num_heads) {
      const int C = p.classes[h];
      float l[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) l[c] = (c < C) ? mx_cls_at(cls, off + c) + p.b2[off + c] : NEG_INF_MX;
      if (writer && p.logits[h]) {
        float* dst = p.logits[h] + ((int64_t)b * p.P + mypair) * C;
        for (int c = 0; c < C; ++c) dst[c] = l[c];
      }
      if (writer && p.tags[h]) {
        const int tag = (int)p.tags[h][(int64_t)b * p.P + mypair];
        const float mx = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3]));
        float e[4], se = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) { e[c] = (c < C) ? __expf(l[c] - mx) : 0.f; se += e[c]; }
        const float lse = mx + __logf(se);
        float lt = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) lt = (c == tag) ? l[c] : lt;
        const float w = (tag < 0 || tag >= C) ? 0.f : (p.cw[h] ? p.cw[h][tag] : 1.f);
        num[h] = w * (lse - lt);
        den[h] = w;
        const float inv = 1.f / se;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float g = (c < C) ? w * (e[c] * inv - (c == tag ? 1.f : 0.f)) : 0.f;
#pragma unroll
          for (int q = 0; q < MX_NCP; ++q) dls[q] += (q == off + c) ? g : 0.f;
        }
      }
      off += C;
    }
  }
  if (p.partials) {
    float* sRed = reinterpret_cast<float*>(smem);  // [NW waves][32] (the weight ring is dead)
    __syncthreads();
#pragma unroll
    for (int h = 0; h < PENEO_MAX_HEADS; ++h) {
      const float a = wave_sum(num[h]), d2 = wave_sum(den[h]);
      if (lane == 0) { sRed[wave * 32 + h] = a; sRed[wave * 32 + 8 + h] = d2; }
    }
#pragma unroll
    for (int c = 0; c < MX_NCP; ++c) {
      const float a = wave_sum(dls[c]);
      if (lane == 0) sRed[wave * 32 + 16 + c] = a;
    }
    __syncthreads();
    if (tid < 32) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += sRed[w * 32 + tid];
      if constexpr (ADD) {
        float* row = p.partials + ((int64_t)b * gridDim.x + blockIdx.x) * 32;
        row[tid] += t;
      } else {
        p.partials[((int64_t)b * gridDim.x + blockIdx.x) * 32 + tid] = t;
      }
    }
  }
}

}  // namespace
}  // namespace peneo
