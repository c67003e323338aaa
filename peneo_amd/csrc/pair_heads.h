// What the forward kernels of the pair-classifier heads share (pair_heads.hip: D <= 512; pair_heads_wide.hip: 512 < D <= 1024):
// the launch parameters and the pieces of the epilogue that turns the logits^T accumulator of 32 pairs into logits, class-weighted
// CE, the un-normalised dlogits and the workgroup's row of partial sums.
#pragma once
#include "common.h"

namespace peneo {

constexpr int NCP = 16;                   // padded class rows that are ever non-zero (<= 16)

struct PairFwdParams {
  const void* ab; int B, N, D; int64_t P;
  int num_heads; int classes[PENEO_MAX_HEADS]; int total_classes;
  const void* wp; const float* b1; const float* b2;
  float* logits[PENEO_MAX_HEADS];
  const int64_t* tags[PENEO_MAX_HEADS];
  const float* cw[PENEO_MAX_HEADS];
  float* partials;   // [B * gridDim.x][32]: num[8] | den[8] | dl_sum[16] per workgroup
  float* dlogits[PENEO_MAX_HEADS];
  uint32_t drop_thr16, drop_seed; float drop_scale;   // K12 dropout (common.h: pair_drop_*): threshold 0 = off, scale = 1 / (1 - p)
  // saving form (hand kernel only): the pairs are walked in the backward's blocks and the kernel leaves q / y records (common.h:
  // PB_REC_BYTES) and x = SiLU(a_i + b_j) in block-row order for peneo_pair_bwd_saved; NULL = the plain walk, nothing saved
  // length-aware walk (peneo_pair_heads_fwd_lens; the LENS instantiations only, which save nothing): [B] token counts, clamped to
  // [0, N] by the kernel; document b is walked as the n_b-token document it is, everything indexed by the pair keeps the N-packed
  // index.  It shares the slot of x_save (which of the two the slot holds is the launcher's `lens_walk` argument, not a field):
  // the kernel arguments of every other instantiation keep their size and offsets
  char* act; union { bf16_t* x_save; const int32_t* lens; }; int ntiles;
  int act_e4m3;      // the records are the 1 KiB e4m3 form (common.h: PB_REC8_BYTES; peneo_pair_heads_fwd_save_e4m3)
};
static_assert(sizeof(PairFwdParams) == 400, "kernel-argument layout of the pair-head forward kernels");

// the LENS walk: n_b, and what a workgroup without a live pair does before it leaves (peneo_loss_finish reads every row)
__device__ __forceinline__ int pair_lens_doc(const PairFwdParams& p, int b) { return min(max(p.lens[b], 0), p.N); }
__device__ __forceinline__ void pair_lens_zero_row(const PairFwdParams& p, int b, int tid) {
  if (p.partials && tid < 32) p.partials[((int64_t)b * gridDim.x + blockIdx.x) * 32 + tid] = 0.f;
}

constexpr float NEG_INF_F = -3.0e38f;
// register arrays must only ever be indexed by compile-time constants (dynamic indices go to scratch)
__device__ __forceinline__ float cls_at(const float (&cls)[NCP], int idx) {
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < NCP; ++c) v = (c == idx) ? cls[c] : v;
  return v;
}
__device__ __forceinline__ void dls_add(float (&dls)[NCP], int idx, float g) {
#pragma unroll
  for (int c = 0; c < NCP; ++c) dls[c] += (c == idx) ? g : 0.f;
}

// logits^T accumulator -> per-pair logits, soft-max CE, un-normalised dlogits and the workgroup's partial sums: pair_epilogue of
// pair_heads.hip (the statement of record, which the eight-wave kernels keep calling: routed through this template their code
// came out 450 instructions different per kernel, and they are left instruction for instruction as they were) for a workgroup of
// NW waves that may come back.  Keep the two texts equal.
// NW: waves of the workgroup.  add: the workgroup's row of partial sums receives a further round of pairs of the same workgroup
// (pair_heads_wide.hip walks its 256 pairs as 2 x 128): the row's own writers add to what they stored the round before.
template <int NW>
__device__ __forceinline__ void pair_epilogue_t(const PairFwdParams& p, const f32x16_t& lg, char* smem, int tid, int lane, int wave,
                                                int half, int b, int64_t mypair, bool pair_ok, bool add) {
  // ---- logits: rows 0..15 of lg live in regs 0..7 (half 0: rows 0-3, 8-11; half 1: rows 4-7, 12-15) ----
  float mine[8], other[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) { mine[r] = lg[r]; other[r] = __shfl_xor(lg[r], 32, 64); }
  float cls[NCP];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    cls[c] = half == 0 ? mine[c] : other[c];
    cls[4 + c] = half == 0 ? other[c] : mine[c];
    cls[8 + c] = half == 0 ? mine[4 + c] : other[4 + c];
    cls[12 + c] = half == 0 ? other[4 + c] : mine[4 + c];
  }
  float num[PENEO_MAX_HEADS], den[PENEO_MAX_HEADS], dls[NCP];
#pragma unroll
  for (int h = 0; h < PENEO_MAX_HEADS; ++h) { num[h] = 0.f; den[h] = 0.f; }
#pragma unroll
  for (int c = 0; c < NCP; ++c) dls[c] = 0.f;
  const bool writer = pair_ok && half == 0;
  {
    int off = 0;
#pragma unroll
    for (int h = 0; h < PENEO_MAX_HEADS; ++h) {
      if (h < p.num_heads) {
        const int C = p.classes[h];
        float l[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) l[c] = (c < C) ? cls_at(cls, off + c) * p.drop_scale + p.b2[off + c] : NEG_INF_F;
        if (writer && p.logits[h]) {
          float* dst = p.logits[h] + ((int64_t)b * p.P + mypair) * C;
          for (int c = 0; c < C; ++c) dst[c] = l[c];
        }
        if (writer && p.tags[h]) {
          const int tag = (int)p.tags[h][(int64_t)b * p.P + mypair];
          float mx = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3]));
          float e[4], se = 0.f;
#pragma unroll
          for (int c = 0; c < 4; ++c) { e[c] = (c < C) ? __expf(l[c] - mx) : 0.f; se += e[c]; }
          const float lse = mx + __logf(se);
          float lt = 0.f;
#pragma unroll
          for (int c = 0; c < 4; ++c) lt = (c == tag) ? l[c] : lt;
          // labels outside [0, C) (the reference's ignore_index = -100 among them) carry zero weight: no loss, no gradient
          const float w = (tag < 0 || tag >= C) ? 0.f : (p.cw[h] ? p.cw[h][tag] : 1.f);
          num[h] = w * (lse - lt);
          den[h] = w;
          const float inv = 1.f / se;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (c < C) {
              float g = w * (e[c] * inv - (c == tag ? 1.f : 0.f));
              if (p.dlogits[h]) p.dlogits[h][((int64_t)b * p.P + mypair) * C + c] = g;
              dls_add(dls, off + c, g);
            }
          }
        }
        off += C;
      }
    }
  }
  if (p.partials) {
    // one row of partial sums per workgroup (plain stores; peneo_loss_finish reduces them): contended atomics
    // on a handful of addresses cost more than the whole MFMA phase
    float* sRed = reinterpret_cast<float*>(smem);  // [NW waves][32] (the weight ring is dead)
    __syncthreads();
#pragma unroll
    for (int h = 0; h < PENEO_MAX_HEADS; ++h) {
      float a = wave_sum(num[h]), d2 = wave_sum(den[h]);
      if (lane == 0) { sRed[wave * 32 + h] = a; sRed[wave * 32 + 8 + h] = d2; }
    }
#pragma unroll
    for (int c = 0; c < NCP; ++c) {
      float a = wave_sum(dls[c]);
      if (lane == 0) sRed[wave * 32 + 16 + c] = a;
    }
    __syncthreads();
    if (tid < 32) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += sRed[w * 32 + tid];
      float* row = p.partials + ((int64_t)b * gridDim.x + blockIdx.x) * 32;
      row[tid] = add ? row[tid] + t : t;
    }
  }
}

// pair_heads_wide.hip (bf16, D % 64 == 0, 512 < D <= 1024), reached through the entry points in pair_heads.hip.
// Its packed image has the slabs of pack_weights_kernel (D / 16 first-layer + 2 second-layer fragments of 1 KiB per 32 hidden units)
// at a stride of a whole number of 4 KiB: one 1 KiB DMA piece per wave of the four-wave workgroup and round.
__host__ __device__ inline int64_t pair_wide_slab_bytes(int D) { return (int64_t)((D / 16 + 2 + 3) / 4) * 4096; }
bool pair_wide_supported(int dtype, int D, int num_heads);
int pair_wide_fwd(const PairFwdParams& p, hipStream_t st, bool lens_walk = false);   // lens_walk: peneo_pair_heads_fwd_lens (p.lens set)

// peneo_pair_dz_fused: the launch parameters of pair_dz_fused_kernel (pair_heads.hip: D <= 512, eight waves) and of
// pair_dz_wide_kernel (pair_dz_wide.hip: 512 < D <= 1024, four waves, the packed image and slab stride of the wide forward).
struct DzFusedParams {
  const bf16_t* abd; int N, D; int64_t pbase, npairs;
  const void* wp; const float* b1;
  peneo_pair_dz_args a;
  bf16_t* out; float* ws;
  bf16_t* x_out; bf16_t* pre_out;   // optional [npairs, D]: SiLU(a_i + b_j) and a_i + b_j for the dW1 / dx GEMMs
  int ws_own;                       // deterministic mode: workspace row = workgroup (one add per address and launch), else % DZF_SLOTS
};
constexpr int DZF_SLOTS = 256;
bool pair_dz_wide_supported(int dtype, int D, int num_heads);
int pair_dz_wide(const DzFusedParams& p, hipStream_t st);

}  // namespace peneo
