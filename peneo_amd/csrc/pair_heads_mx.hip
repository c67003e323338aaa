// MXFP8 eval path of the five pair-classifier heads (K11 + K12 + K13 forward, no dropout, no backward).
//
// Same skeleton as pair_heads_fwd_kernel (pair_heads.hip): one workgroup owns 256 consecutive pairs of one document, each
// 64-lane wave 32 of them (lane & 31 = pair); x = SiLU(a_i + b_j) stays in B-operand registers for the whole launch; the
// first-layer weights of all heads stream L2 -> LDS by LDS-DMA, one 32-row slab of hidden units at a time, through a ring of
// NSTAGE buffers; the C-layout accumulator of a slab is, after bias + SiLU, the B operand of the bf16 second layer.  The first
// layer runs on v_mfma_scale_f32_32x32x64_f8f6f4 with OCP e4m3 operands and E8M0 block scales (OCP MX v1.0, blocks of 32
// consecutive elements along D): twice the bf16 MFMA rate, half the weight bytes per slab, half the x registers.
//
// Operand maps of the scaled MFMA with e4m3 operands (checked on the MI355X with exact integer data and random scales):
//   A: lane l holds row l & 31; byte j (0..31) of its 8 dwords is k = 32 (j >> 4) + 16 (l >> 5) + (j & 15) of the 64-wide step
//   B: lane l holds column l & 31, bytes as for A
//   scales: the op_sel byte of lane r + 32 kb's scale VGPR scales row (column) r, K-block kb = k / 32 of the step
// so one 32-element block of a pair is spread over two lanes (16 elements in lane c, 16 in lane c + 32): its amax takes one
// cross-half exchange.  The C/D map is that of every 32x32 MFMA (common.h acc_row).
//
// Quantization (both operands of the first layer, the pack and peneo_mxfp8_quantize_rows alike): for a block with amax > 0 the
// scale is 2^e, e = floor(log2(amax)) - 8 clamped to [-127, 127] (E8M0 byte e + 127; an all-zero block gets byte 0); an element
// becomes e4m3fn(RNE(clamp(v / 2^e, -448, 448))).  v / 2^e is an exact power-of-two multiply; v_cvt_pk_fp8_f32 rounds to nearest
// even with e4m3 subnormals but returns NaN above 464 instead of saturating (measured), hence the explicit clamp.
#include <stdlib.h>

#include "common.h"
#include "mx_common.h"
#include "pair_heads_mx.h"

namespace peneo {
namespace {

constexpr int MX_WAVES = 8;
constexpr int MX_PAIRS = MX_WAVES * 32;   // as PH_PAIRS: the loss partial rows are peneo_pair_loss_partials(B, N)
constexpr int MX_MAX_KS = 8;              // D <= 512 (x: D / 8 VGPRs per lane)

// Packed slab: pair_heads_mx.h, padded for this kernel's eight waves.
__host__ __device__ constexpr int mx_upw(int ks8) { return mx_upw_t<MX_WAVES>(ks8); }
__host__ __device__ constexpr int mx_slab_bytes(int ks8) { return mx_slab_bytes_t<MX_WAVES>(ks8); }
// ring depth: 3 while two workgroups still fit a CU's 160 KiB of LDS, else 2
__host__ __device__ constexpr int mx_nstage(int ks8) { return ks8 <= 6 ? 3 : 2; }

// one thread per block of 32 elements of a row-major [rows, ld] source (fp32 or bf16: a bf16 value and its fp32 image quantize alike)
template <typename T>
__global__ __launch_bounds__(256) void mx_quantize_rows_kernel(const T* src, int64_t nblocks, int bpr, int64_t ld, uint8_t* q, uint8_t* sc) {
  for (int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; blk < nblocks; blk += (int64_t)gridDim.x * blockDim.x) {
    float v[32];
    const int64_t row = blk / bpr;
    const uint4* s4 = reinterpret_cast<const uint4*>(src + row * ld + (blk - row * bpr) * 32);
    constexpr int VEC = Elem<T>::kVec;
#pragma unroll
    for (int i = 0; i < 32 / VEC; ++i) unpack16<T>(s4[i], v + VEC * i);
    uint32_t w[8];
    sc[blk] = (uint8_t)mx_quantize32(v, w);
    uint4* d4 = reinterpret_cast<uint4*>(q + blk * 32);
    d4[0] = make_uint4(w[0], w[1], w[2], w[3]);
    d4[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
}

template <int KS8, int NSTAGE>
__global__ __launch_bounds__(MX_WAVES * 64, 2) void pair_heads_mx_fwd_kernel(MxFwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NSW = mx_scale_words(KS8), UPW = mx_upw(KS8), SLAB = mx_slab_bytes(KS8);
  constexpr int D = KS8 * 64;
  static_assert(UPW <= 12, "slab too large");
  char* sW = smem;                                                    // [NSTAGE][SLAB]
  float* sB1 = reinterpret_cast<float*>(smem + NSTAGE * SLAB);        // [nh * D]
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, b = blockIdx.y;
  const int64_t mypair = (int64_t)blockIdx.x * MX_PAIRS + wave * 32 + (lane & 31);
  const bool pair_ok = mypair < p.P;
  int pi, pj;
  pair_decode(pair_ok ? mypair : p.P - 1, N, pi, pj);
  const int nslab = p.num_heads * D / 32;

  for (int i = tid; i < p.num_heads * D; i += MX_WAVES * 64) sB1[i] = p.b1[i];

  // ---- x = SiLU(a_i + b_j), quantized to MXFP8 straight into B-operand registers: lane (c, half) of k-step ks holds
  //      k = 64 ks + 32 kb + 16 half + t (kb = 0, 1; t = 0..15); block kb's amax meets its other 16 elements in lane ^ 32,
  //      and this lane provides the scale of block kb = half ----
  const bf16_t* abd = p.ab + (int64_t)b * N * 2 * D;
  const bf16_t* arow = abd + (int64_t)pi * 2 * D;
  const bf16_t* brow = abd + (int64_t)pj * 2 * D + D;
  i32x8_t xf[KS8];
  uint32_t xs[NSW];
#pragma unroll
  for (int g = 0; g < NSW; ++g) xs[g] = 0u;
#pragma unroll
  for (int ks = 0; ks < KS8; ++ks) {
    float v[2][16];
    float am[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int c = 64 * ks + 32 * kb + 16 * half;
      float a[16], bb[16];
      unpack16<bf16_t>(*reinterpret_cast<const uint4*>(arow + c), a);
      unpack16<bf16_t>(*reinterpret_cast<const uint4*>(arow + c + 8), a + 8);
      unpack16<bf16_t>(*reinterpret_cast<const uint4*>(brow + c), bb);
      unpack16<bf16_t>(*reinterpret_cast<const uint4*>(brow + c + 8), bb + 8);
      float m = 0.f;
#pragma unroll
      for (int t = 0; t < 16; ++t) { v[kb][t] = silu_f(a[t] + bb[t]); m = fmaxf(m, fabsf(v[kb][t])); }
      am[kb] = fmaxf(m, __shfl_xor(m, 32, 64));
    }
    uint32_t q[8];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const uint32_t sb = mx_scale_byte(am[kb]);
      const float inv = mx_inv_scale(sb);
#pragma unroll
      for (int w = 0; w < 4; ++w)
        q[4 * kb + w] = mx_e4m3x4(v[kb][4 * w] * inv, v[kb][4 * w + 1] * inv, v[kb][4 * w + 2] * inv, v[kb][4 * w + 3] * inv);
      if (kb == half) xs[ks >> 2] |= sb << (8 * (ks & 3));
    }
#pragma unroll
    for (int w = 0; w < 8; ++w) xf[ks][w] = (int)q[w];
    __builtin_amdgcn_sched_barrier(0);   // few gathers in flight at a time (else their raw data spills)
  }
  // every ordinary global load above has been consumed: from here on the vm counter only sees our DMA pieces
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();   // sB1 visible

  const char* wsrc = p.wp + wave * (UPW * 1024) + lane * 16;
  const uint32_t wdst = lds_addr(sW) + wave * (UPW * 1024);
#pragma unroll
  for (int s0 = 0; s0 < NSTAGE - 1; ++s0)
    if (s0 < nslab) lds_dma_units<0, UPW>(wsrc + (int64_t)s0 * SLAB, wdst + s0 * SLAB);

  f32x16_t lg;   // logits^T[class, pair]
#pragma unroll
  for (int r = 0; r < 16; ++r) lg[r] = 0.f;

  for (int slab = 0; slab < nslab; ++slab) {
    // slabs slab .. slab + NSTAGE - 2 are in flight (fewer at the end): wait for the oldest, then publish it
    if (NSTAGE > 2 && slab + 1 < nslab) wait_vm<(NSTAGE - 2) * UPW>(); else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (slab + NSTAGE - 1 < nslab) lds_dma_units<0, UPW>(wsrc + (int64_t)(slab + NSTAGE - 1) * SLAB, wdst + ((slab + NSTAGE - 1) % NSTAGE) * SLAB);
    const char* wb = sW + (slab % NSTAGE) * SLAB;
    uint32_t ws[NSW];
#pragma unroll
    for (int g = 0; g < NSW; ++g) ws[g] = *reinterpret_cast<const uint32_t*>(wb + KS8 * 2048 + g * 256 + lane * 4);
    f32x16_t z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    mx_static_for<0, KS8>([&](auto kc) {
      constexpr int ks = decltype(kc)::value;
      const uint4 lo = *reinterpret_cast<const uint4*>(wb + ks * 2048 + lane * 16);
      const uint4 hi = *reinterpret_cast<const uint4*>(wb + ks * 2048 + 1024 + lane * 16);
      const i32x8_t wf = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
      z = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf, xf[ks], z, 0, 0, ks & 3, (int)ws[ks >> 2], ks & 3, (int)xs[ks >> 2]);
      // D = 512: x takes 64 VGPRs; with every fragment read of the slab hoisted to its top (16 VGPRs each) the kernel spills
      if constexpr (KS8 > 6 && (ks & 1) == 1) __builtin_amdgcn_sched_barrier(0);
    });
    // bias + SiLU in registers; accumulator rows 8g + 4 half + 0..3 are the second layer's B operand (pack order)
    float y[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 bv = *reinterpret_cast<const float4*>(sB1 + slab * 32 + 8 * g + 4 * half);
      y[4 * g + 0] = silu_f(z[4 * g + 0] + bv.x);
      y[4 * g + 1] = silu_f(z[4 * g + 1] + bv.y);
      y[4 * g + 2] = silu_f(z[4 * g + 2] + bv.z);
      y[4 * g + 3] = silu_f(z[4 * g + 3] + bv.w);
    }
    const char* w2 = wb + KS8 * 2048 + NSW * 256;
    Frag<bf16_t> w2a = load_frag_linear<bf16_t>(w2, 0, lane), w2b = load_frag_linear<bf16_t>(w2, 1, lane);
    mma_step(w2a, pack_frag8<bf16_t>(y), lg);
    mma_step(w2b, pack_frag8<bf16_t>(y + 8), lg);
  }
  mx_epilogue<MX_WAVES>(p, lg, smem, tid, lane, wave, half, b, mypair, pair_ok);
}

template <int KS8>
int launch_mx_fwd(const MxFwdParams& p, hipStream_t st) {
  constexpr int NSTAGE = mx_nstage(KS8);
  size_t sh = (size_t)NSTAGE * mx_slab_bytes(KS8) + (size_t)p.num_heads * p.D * sizeof(float);
  if (sh < (size_t)MX_WAVES * 32 * sizeof(float)) sh = (size_t)MX_WAVES * 32 * sizeof(float);
  if (sh > 160 * 1024) { set_error("peneo_pair_heads_fwd_mxfp8: D=%d, %d heads need %zu bytes of LDS", p.D, p.num_heads, sh); return PENEO_ERR_INVALID; }
  if (sh > 64 * 1024 && raise_dynamic_lds(pair_heads_mx_fwd_kernel<KS8, NSTAGE>, sh, "peneo_pair_heads_fwd_mxfp8") != PENEO_OK) return PENEO_ERR_LAUNCH;
  dim3 grid((unsigned)((p.P + MX_PAIRS - 1) / MX_PAIRS), p.B);
  hipLaunchKernelGGL((pair_heads_mx_fwd_kernel<KS8, NSTAGE>), grid, dim3(MX_WAVES * 64), sh, st, p);
  return check_launch("peneo_pair_heads_fwd_mxfp8");
}

// ================================================================================================
// Train forward (peneo_pair_heads_fwd_mxfp8_save): the eval kernel's first layer - same quantizer, same scaled MFMAs in the same
// order, so z is the eval kernel's z bit for bit - on the walk of the bf16 saving forward (pair_heads.hip, SAVE): a workgroup = two
// blocks of 8 x 16 pairs, a wave = one group of 32, lane & 31 = pair.  It leaves what peneo_pair_bwd_saved reads: x rows (bf16) and
// the f16 records of z + b1 with the K12 dropout applied (common.h: PB_REC_BYTES), and computes dropout scale, dlogits and the loss
// rows as peneo_pair_heads_fwd does.  The backward never repeats the first-layer product, so its gradients are those of the bf16
// weights taken at this forward's z (straight-through on the quantizer).
// ================================================================================================
struct MxSaveParams {
  MxFwdParams f;     // partials: [B * ceil(ntiles / 2)][32]
  float* dlogits[PENEO_MAX_HEADS];
  uint32_t drop_thr16, drop_seed; float drop_scale;   // K12 dropout (common.h: pair_drop_*): threshold 0 = off
  char* act; bf16_t* x_save; int ntiles;
};

constexpr int MXS_XPITCH = 272;   // x staging rows: 256 bytes (two k-steps) + 16 (bank spread)
__host__ __device__ constexpr int mxs_ring_bytes(int ks8, int nstage) {
  return nstage * mx_slab_bytes(ks8) > MX_WAVES * 32 * MXS_XPITCH ? nstage * mx_slab_bytes(ks8) : MX_WAVES * 32 * MXS_XPITCH;
}

// mx_epilogue plus what a train step needs: the dropout scale on the second layer's sums and the dlogits stores (pair_epilogue of
// pair_heads.hip; with scale 1 and no dlogits the values are mx_epilogue's)
__device__ __forceinline__ void mx_save_epilogue(const MxSaveParams& q, const f32x16_t& lg, char* smem, int tid, int lane, int wave,
                                                 int half, int b, int64_t mypair, bool pair_ok) {
  const MxFwdParams& p = q.f;
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
      for (int c = 0; c < 4; ++c) l[c] = (c < C) ? mx_cls_at(cls, off + c) * q.drop_scale + p.b2[off + c] : NEG_INF_MX;
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
          if (c < C && q.dlogits[h]) q.dlogits[h][((int64_t)b * p.P + mypair) * C + c] = g;
#pragma unroll
          for (int k = 0; k < MX_NCP; ++k) dls[k] += (k == off + c) ? g : 0.f;
        }
      }
      off += C;
    }
  }
  if (p.partials) {
    float* sRed = reinterpret_cast<float*>(smem);  // [8 waves][32] (the weight ring is dead)
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
      for (int w = 0; w < MX_WAVES; ++w) t += sRed[w * 32 + tid];
      p.partials[((int64_t)b * gridDim.x + blockIdx.x) * 32 + tid] = t;
    }
  }
}

template <int KS8, int NSTAGE, bool DROP>
__global__ __launch_bounds__(MX_WAVES * 64, 2) void pair_heads_mx_save_kernel(MxSaveParams q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NSW = mx_scale_words(KS8), UPW = mx_upw(KS8), SLAB = mx_slab_bytes(KS8);
  constexpr int D = KS8 * 64;
  static_assert(UPW <= 12 && KS8 % 2 == 0, "slab too large / x rows are staged two k-steps at a time");
  const MxFwdParams& p = q.f;
  char* sW = smem;                                                                 // [NSTAGE][SLAB]; before the loop: x staging
  float* sB1 = reinterpret_cast<float*>(smem + mxs_ring_bytes(KS8, NSTAGE));       // [nh * D]
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, b = blockIdx.y;
  // the backward's walk (pair_bwd.hip; pair_heads_fwd_hand_kernel<.., SAVE>): the absent second block of the last workgroup of an odd
  // block count repeats the last block and writes nothing
  const int T2 = 2 * (int)blockIdx.x + (wave >> 2), grp = wave & 3, r32 = lane & 31;
  const bool tile_ok = T2 < q.ntiles;
  const int tile = tile_ok ? T2 : q.ntiles - 1;
  int ti = 0;
  const int nti = pb_row_tiles(N);
  while (ti + 1 < nti && pb_tiles_before(ti + 1, N) <= tile) ++ti;
  const int tj = (ti >> 1) + (tile - pb_tiles_before(ti, N));
  const int qi = ti * PB_TI + 2 * grp + (r32 >> 4), qj = tj * PB_TJ + (r32 & 15);
  const bool pair_ok = tile_ok && qi < N && qj < N && qi <= qj;
  const int pi = min(qi, N - 1), pj = min(qj, N - 1);       // (pairs outside the triangle: finite x / z / y, their dlogits are never read)
  const int64_t mypair = pair_ok ? pair_row_start(pi, N) + (pj - pi) : p.P - 1;
  const int nslab = p.num_heads * D / 32;

  for (int i = tid; i < p.num_heads * D; i += MX_WAVES * 64) sB1[i] = p.b1[i];

  // ---- x = SiLU(a_i + b_j): quantized into B-operand registers exactly as in pair_heads_mx_fwd_kernel; its bf16 image goes through
  //      the wave's corner of the still empty weight ring and leaves as 256-byte runs of the block-order x rows (the bytes of
  //      peneo_pair_heads_fwd_save: bf16(silu_f(a + b))) ----
  const bf16_t* abd = p.ab + (int64_t)b * N * 2 * D;
  const bf16_t* arow = abd + (int64_t)pi * 2 * D;
  const bf16_t* brow = abd + (int64_t)pj * 2 * D + D;
  char* const sX = smem + wave * (32 * MXS_XPITCH);
  bf16_t* const xdst = q.x_save + (((int64_t)b * q.ntiles + tile) * PB_ROWS + grp * 32) * D;
  i32x8_t xf[KS8];
  uint32_t xs[NSW];
#pragma unroll
  for (int g = 0; g < NSW; ++g) xs[g] = 0u;
#pragma unroll
  for (int ks = 0; ks < KS8; ++ks) {
    float v[2][16];
    float am[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int c = 64 * ks + 32 * kb + 16 * half;
      float a[16], bb[16];
      unpack16<bf16_t>(*reinterpret_cast<const uint4*>(arow + c), a);
      unpack16<bf16_t>(*reinterpret_cast<const uint4*>(arow + c + 8), a + 8);
      unpack16<bf16_t>(*reinterpret_cast<const uint4*>(brow + c), bb);
      unpack16<bf16_t>(*reinterpret_cast<const uint4*>(brow + c + 8), bb + 8);
      float m = 0.f;
#pragma unroll
      for (int t = 0; t < 16; ++t) { v[kb][t] = silu_f(a[t] + bb[t]); m = fmaxf(m, fabsf(v[kb][t])); }
      am[kb] = fmaxf(m, __shfl_xor(m, 32, 64));
      // elements c .. c + 15 of the pair's row: bytes 2 c .. 2 c + 31, i.e. 128 (ks & 1) + 64 kb + 32 half of this pass
      char* const sx = sX + r32 * MXS_XPITCH + 128 * (ks & 1) + 64 * kb + 32 * half;
      *reinterpret_cast<uint4*>(sx) = pack16<bf16_t>(v[kb]);
      *reinterpret_cast<uint4*>(sx + 16) = pack16<bf16_t>(v[kb] + 8);
    }
    uint32_t qq[8];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const uint32_t sb = mx_scale_byte(am[kb]);
      const float inv = mx_inv_scale(sb);
#pragma unroll
      for (int w = 0; w < 4; ++w)
        qq[4 * kb + w] = mx_e4m3x4(v[kb][4 * w] * inv, v[kb][4 * w + 1] * inv, v[kb][4 * w + 2] * inv, v[kb][4 * w + 3] * inv);
      if (kb == half) xs[ks >> 2] |= sb << (8 * (ks & 3));
    }
#pragma unroll
    for (int w = 0; w < 8; ++w) xf[ks][w] = (int)qq[w];
    if (ks & 1) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r = 4 * j + (lane >> 4), c = lane & 15;
        const uint4 xv = *reinterpret_cast<const uint4*>(sX + r * MXS_XPITCH + 16 * c);
        if (tile_ok) *reinterpret_cast<uint4*>(xdst + (int64_t)r * D + 128 * (ks >> 1) + 8 * c) = xv;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
    }
    __builtin_amdgcn_sched_barrier(0);   // few gathers in flight at a time (else their raw data spills)
  }
  // every ordinary global access above has completed: from here on the vm counter sees our DMA pieces and the record stores
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();   // sB1 visible; every wave has left the x staging area

  const char* wsrc = p.wp + wave * (UPW * 1024) + lane * 16;
  const uint32_t wdst = lds_addr(sW) + wave * (UPW * 1024);
#pragma unroll
  for (int s0 = 0; s0 < NSTAGE - 1; ++s0)
    if (s0 < nslab) lds_dma_units<0, UPW>(wsrc + (int64_t)s0 * SLAB, wdst + s0 * SLAB);

  f32x16_t lg;   // logits^T[class, pair]
#pragma unroll
  for (int r = 0; r < 16; ++r) lg[r] = 0.f;
  const uint32_t drop_key = DROP ? pair_drop_key(q.drop_seed, b) : 0u;
  const uint32_t drop_base = (uint32_t)(mypair * nslab * 2) + (uint32_t)half;
  const uint32_t thr32 = q.drop_thr16 << 16;                // field = bits 16.. of the chain state
  // records of this wave's group: slab s at + s * 4 groups * PB_REC_BYTES; the lane's 16-byte piece of a half at row (lane & 31) (the
  // second half: ^ 4), byte 16 (lane >> 5) (common.h; the stores of pair_heads_fwd_hand_kernel's save_rows)
  char* const rec_l = q.act + ((((int64_t)b * q.ntiles + tile) * nslab * 4 + grp) * PB_REC_BYTES + 16 * half);
  const int rec_r0 = r32 * 32, rec_r1 = 1024 + (r32 ^ 4) * 32;

  for (int slab = 0; slab < nslab; ++slab) {
    // slabs slab .. slab + NSTAGE - 2 are in flight (fewer at the end): wait for the oldest, then publish it.  The record stores
    // of earlier slabs count too and are younger than that slab's pieces, so the count of the eval kernel only waits for more
    // (as pair_heads_fwd_hand_kernel's; a wave of an absent block issues no stores, so nothing may be added to the count)
    if (NSTAGE > 2 && slab + 1 < nslab) wait_vm<(NSTAGE - 2) * UPW>(); else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (slab + NSTAGE - 1 < nslab) lds_dma_units<0, UPW>(wsrc + (int64_t)(slab + NSTAGE - 1) * SLAB, wdst + ((slab + NSTAGE - 1) % NSTAGE) * SLAB);
    const char* wb = sW + (slab % NSTAGE) * SLAB;
    uint32_t ws[NSW];
#pragma unroll
    for (int g = 0; g < NSW; ++g) ws[g] = *reinterpret_cast<const uint32_t*>(wb + KS8 * 2048 + g * 256 + lane * 4);
    f32x16_t z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    mx_static_for<0, KS8>([&](auto kc) {
      constexpr int ks = decltype(kc)::value;
      const uint4 lo = *reinterpret_cast<const uint4*>(wb + ks * 2048 + lane * 16);
      const uint4 hi = *reinterpret_cast<const uint4*>(wb + ks * 2048 + 1024 + lane * 16);
      const i32x8_t wf = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
      z = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf, xf[ks], z, 0, 0, ks & 3, (int)ws[ks >> 2], ks & 3, (int)xs[ks >> 2]);
      // the fragment reads of a slab hoisted to its top take 16 VGPRs each: at most two k-steps' worth at a time
      if constexpr ((ks & 1) == 1) __builtin_amdgcn_sched_barrier(0);
    });
    // bias, then the K12 dropout: the lane's 16 units (accumulator rows 8g + 4 half + e) are the 16 fields of one chain, in register
    // order.  A dropped unit becomes -30000: SiLU of it is -0, the record's f16 is below -20000, the backward's SiLU' of it is 0
    uint32_t st = 0u, sinc = 0u;
    if constexpr (DROP) {
      st = pair_drop_seed(drop_key, drop_base + 2u * (uint32_t)slab);
      sinc = pair_drop_inc(drop_key, drop_base + 2u * (uint32_t)slab);
    }
    float zb[16], y[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 bv = *reinterpret_cast<const float4*>(sB1 + slab * 32 + 8 * g + 4 * half);
      const float be[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = z[4 * g + e] + be[e];
        if constexpr (DROP) { st = pair_drop_step(st, sinc); t = st >= thr32 ? t : -30000.f; }
        zb[4 * g + e] = t;
        y[4 * g + e] = silu_f(t);
      }
    }
    // records: the two halves of a pair's lanes hold 4 + 4 consecutive units of each group of 8; a v_permlane32_swap pair makes 16
    // contiguous bytes per lane (lanes 0-31: units 0..7 of the half, lanes 32-63: units 8..15); every store is 1 KiB contiguous
    char* const rec = rec_l + (int64_t)slab * (4 * PB_REC_BYTES);
#pragma unroll
    for (int G = 0; G < 4; G += 2) {
      const uint32_t z0 = pack_f16x2(zb[4 * G], zb[4 * G + 1]), z1 = pack_f16x2(zb[4 * G + 2], zb[4 * G + 3]);
      const uint32_t z2 = pack_f16x2(zb[4 * G + 4], zb[4 * G + 5]), z3 = pack_f16x2(zb[4 * G + 6], zb[4 * G + 7]);
      const auto zx = __builtin_amdgcn_permlane32_swap(z0, z2, false, false);
      const auto zy = __builtin_amdgcn_permlane32_swap(z1, z3, false, false);
      if (tile_ok) {
        typedef unsigned int mx_u4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(mx_u4{zx[0], zy[0], zx[1], zy[1]}, reinterpret_cast<mx_u4*>(rec + (G == 0 ? rec_r0 : rec_r1)));
      }
    }
    const char* w2 = wb + KS8 * 2048 + NSW * 256;
    Frag<bf16_t> w2a = load_frag_linear<bf16_t>(w2, 0, lane), w2b = load_frag_linear<bf16_t>(w2, 1, lane);
    mma_step(w2a, pack_frag8<bf16_t>(y), lg);
    mma_step(w2b, pack_frag8<bf16_t>(y + 8), lg);
  }
  wait_vm<0>();
  mx_save_epilogue(q, lg, smem, tid, lane, wave, half, b, mypair, pair_ok);
}

template <int KS8>
int launch_mx_save(const MxSaveParams& q, hipStream_t st) {
  constexpr int NSTAGE = mx_nstage(KS8);
  const size_t sh = (size_t)mxs_ring_bytes(KS8, NSTAGE) + (size_t)q.f.num_heads * q.f.D * sizeof(float);
  if (sh > 160 * 1024) { set_error("peneo_pair_heads_fwd_mxfp8_save: D=%d, %d heads need %zu bytes of LDS", q.f.D, q.f.num_heads, sh); return PENEO_ERR_INVALID; }
  const void* fn = q.drop_thr16 ? reinterpret_cast<const void*>(pair_heads_mx_save_kernel<KS8, NSTAGE, true>)
                                : reinterpret_cast<const void*>(pair_heads_mx_save_kernel<KS8, NSTAGE, false>);
  if (raise_dynamic_lds(fn, sh, "peneo_pair_heads_fwd_mxfp8_save") != PENEO_OK) return PENEO_ERR_LAUNCH;
  dim3 grid((unsigned)((q.ntiles + 1) / 2), q.f.B);
  if (q.drop_thr16) hipLaunchKernelGGL((pair_heads_mx_save_kernel<KS8, NSTAGE, true>), grid, dim3(MX_WAVES * 64), sh, st, q);
  else hipLaunchKernelGGL((pair_heads_mx_save_kernel<KS8, NSTAGE, false>), grid, dim3(MX_WAVES * 64), sh, st, q);
  return check_launch("peneo_pair_heads_fwd_mxfp8_save");
}

}  // namespace
}  // namespace peneo

using namespace peneo;

extern "C" int peneo_mxfp8_quantize_rows(const float* src, int64_t rows, int64_t cols, void* q_e4m3, void* scales_e8m0,
                                         peneo_stream_t stream) {
  PENEO_REQUIRE(src && q_e4m3 && scales_e8m0 && rows > 0 && cols > 0, "peneo_mxfp8_quantize_rows: bad arguments");
  PENEO_REQUIRE(cols % 32 == 0, "peneo_mxfp8_quantize_rows: cols must be a multiple of 32 (the MX block), got %lld", (long long)cols);
  PENEO_REQUIRE((reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(q_e4m3) & 15) == 0,
                "peneo_mxfp8_quantize_rows: src / q must be 16-byte aligned");
  const int64_t nblocks = rows * (cols / 32);
  hipLaunchKernelGGL(mx_quantize_rows_kernel<float>, dim3(mx_blocks(nblocks)), dim3(256), 0, (hipStream_t)stream, src, nblocks,
                     (int)(cols / 32), cols, static_cast<uint8_t*>(q_e4m3), static_cast<uint8_t*>(scales_e8m0));
  return check_launch("peneo_mxfp8_quantize_rows");
}

extern "C" int peneo_mxfp8_quantize_rows_bf16(const void* src, int64_t rows, int64_t cols, int64_t ld, void* q_e4m3, void* scales_e8m0,
                                              peneo_stream_t stream) {
  PENEO_REQUIRE(src && q_e4m3 && scales_e8m0 && rows > 0 && cols > 0, "peneo_mxfp8_quantize_rows_bf16: bad arguments");
  PENEO_REQUIRE(cols % 32 == 0 && cols <= (int64_t)32 * 0x7fffffff, "peneo_mxfp8_quantize_rows_bf16: cols must be a multiple of 32 (the MX block), got %lld", (long long)cols);
  PENEO_REQUIRE(ld >= cols && ld % 8 == 0, "peneo_mxfp8_quantize_rows_bf16: ld must be >= cols and a multiple of 8, got %lld", (long long)ld);
  PENEO_REQUIRE((reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(q_e4m3) & 15) == 0,
                "peneo_mxfp8_quantize_rows_bf16: src / q must be 16-byte aligned");
  const int64_t nblocks = rows * (cols / 32);
  hipLaunchKernelGGL(mx_quantize_rows_kernel<bf16_t>, dim3(mx_blocks(nblocks)), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const bf16_t*>(src), nblocks, (int)(cols / 32), ld, static_cast<uint8_t*>(q_e4m3),
                     static_cast<uint8_t*>(scales_e8m0));
  return check_launch("peneo_mxfp8_quantize_rows_bf16");
}

extern "C" int peneo_pair_mxfp8_supported(int D, int num_heads) {
  if (num_heads < 1 || num_heads > PENEO_MAX_HEADS || D < 64 || D > 64 * MX_MAX_KS || D % 64 != 0) return 0;
  const int ks8 = D / 64;
  const size_t sh = (size_t)mx_nstage(ks8) * mx_slab_bytes(ks8) + (size_t)num_heads * D * sizeof(float);
  return sh <= 160 * 1024 ? 1 : 0;
}

extern "C" size_t peneo_pair_heads_mxfp8_packed_bytes(int num_heads, int D) {
  if (!peneo_pair_mxfp8_supported(D, num_heads)) return 0;
  return (size_t)(num_heads * D / 32) * (size_t)mx_slab_bytes(D / 64);
}

extern "C" int peneo_pair_heads_pack_mxfp8(const float* const* w1, const float* const* w2, const int* classes, int num_heads,
                                           int D, void* packed, peneo_stream_t stream) {
  PENEO_REQUIRE(w1 && w2 && classes && packed, "peneo_pair_heads_pack_mxfp8: bad arguments");
  PENEO_REQUIRE(peneo_pair_mxfp8_supported(D, num_heads), "peneo_pair_heads_pack_mxfp8: D=%d with %d heads not supported (peneo_pair_mxfp8_supported)", D, num_heads);
  PENEO_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, "peneo_pair_heads_pack_mxfp8: packed must be 16-byte aligned");
  MxPackSrc s = {};
  s.num_heads = num_heads; s.D = D;
  int tc = 0;
  for (int h = 0; h < num_heads; ++h) {
    PENEO_REQUIRE(w1[h] && w2[h], "peneo_pair_heads_pack_mxfp8: null weight pointer for head %d", h);
    PENEO_REQUIRE(classes[h] >= 1 && classes[h] <= 4, "peneo_pair_heads_pack_mxfp8: classes[%d] must be 1..4", h);
    s.w1[h] = w1[h]; s.w2[h] = w2[h]; s.classes[h] = classes[h]; tc += classes[h];
  }
  PENEO_REQUIRE(tc <= MX_NCP, "peneo_pair_heads_pack_mxfp8: more than %d classes in total", MX_NCP);
  const hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(packed, 0, peneo_pair_heads_mxfp8_packed_bytes(num_heads, D), st) != hipSuccess) {
    set_error("peneo_pair_heads_pack_mxfp8: hipMemsetAsync failed");
    return PENEO_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(mx_pack_w1_kernel<MX_WAVES>, dim3(mx_blocks((int64_t)num_heads * D * (D / 32))), dim3(256), 0, st, s, static_cast<char*>(packed));
  hipLaunchKernelGGL(mx_pack_w2_kernel<MX_WAVES>, dim3(mx_blocks((int64_t)(num_heads * D / 32) * 1024)), dim3(256), 0, st, s, static_cast<char*>(packed));
  return check_launch("peneo_pair_heads_pack_mxfp8");
}

extern "C" int peneo_pair_heads_fwd_mxfp8(const void* ab, int B, int N, const peneo_pair_heads_desc* desc, float* const* logits,
                                          const peneo_pair_loss* loss, peneo_stream_t stream) {
  PENEO_REQUIRE(ab && desc && B > 0 && N > 0, "peneo_pair_heads_fwd_mxfp8: bad arguments");
  PENEO_REQUIRE(peneo_pair_mxfp8_supported(desc->D, desc->num_heads), "peneo_pair_heads_fwd_mxfp8: D=%d with %d heads not supported (peneo_pair_mxfp8_supported)", desc->D, desc->num_heads);
  PENEO_REQUIRE(desc->w_packed && desc->b1 && desc->b2, "peneo_pair_heads_fwd_mxfp8: null weights");
  PENEO_REQUIRE((reinterpret_cast<uintptr_t>(desc->w_packed) & 15) == 0 && (reinterpret_cast<uintptr_t>(ab) & 15) == 0,
                "peneo_pair_heads_fwd_mxfp8: ab / packed weights must be 16-byte aligned");
  PENEO_REQUIRE(desc->drop_p == 0.f, "peneo_pair_heads_fwd_mxfp8: eval only, drop_p must be 0");
  MxFwdParams p = {};
  p.ab = static_cast<const bf16_t*>(ab); p.B = B; p.N = N; p.D = desc->D; p.P = (int64_t)N * (N + 1) / 2;
  p.num_heads = desc->num_heads;
  p.wp = static_cast<const char*>(desc->w_packed); p.b1 = desc->b1; p.b2 = desc->b2;
  int tc = 0;
  for (int h = 0; h < desc->num_heads; ++h) {
    PENEO_REQUIRE(desc->classes[h] >= 1 && desc->classes[h] <= 4, "peneo_pair_heads_fwd_mxfp8: classes[%d] must be 1..4", h);
    p.classes[h] = desc->classes[h]; tc += desc->classes[h];
    p.logits[h] = logits ? logits[h] : nullptr;
    if (loss) {
      PENEO_REQUIRE(!loss->dlogits[h], "peneo_pair_heads_fwd_mxfp8: eval only, dlogits must be NULL");
      p.tags[h] = loss->tags[h]; p.cw[h] = loss->class_weight[h];
    }
  }
  PENEO_REQUIRE(tc <= MX_NCP, "peneo_pair_heads_fwd_mxfp8: more than %d classes in total", MX_NCP);
  if (loss) {
    p.partials = loss->partials;
    bool any = false;
    for (int h = 0; h < desc->num_heads; ++h) any = any || loss->tags[h];
    if (any) PENEO_REQUIRE(p.partials, "peneo_pair_heads_fwd_mxfp8: loss->partials workspace missing");
  }
  const hipStream_t st = (hipStream_t)stream;
  switch (desc->D / 64) {
    case 1: return launch_mx_fwd<1>(p, st);
    case 2: return launch_mx_fwd<2>(p, st);
    case 3: return launch_mx_fwd<3>(p, st);
    case 4: return launch_mx_fwd<4>(p, st);
    case 5: return launch_mx_fwd<5>(p, st);
    case 6: return launch_mx_fwd<6>(p, st);
    case 7: return launch_mx_fwd<7>(p, st);
    default: return launch_mx_fwd<8>(p, st);
  }
}

extern "C" int peneo_pair_mxfp8_save_supported(int D, int num_heads) {
  return peneo_pair_save_supported(PENEO_BF16, D, num_heads) && peneo_pair_mxfp8_supported(D, num_heads) ? 1 : 0;
}

extern "C" int peneo_pair_heads_fwd_mxfp8_save(const void* ab, int B, int N, const peneo_pair_heads_desc* desc, float* const* logits,
                                               const peneo_pair_loss* loss, void* act, void* x_rows, peneo_stream_t stream) {
  PENEO_REQUIRE(ab && desc && B > 0 && N > 0, "peneo_pair_heads_fwd_mxfp8_save: bad arguments");
  PENEO_REQUIRE(peneo_pair_mxfp8_save_supported(desc->D, desc->num_heads),
                "peneo_pair_heads_fwd_mxfp8_save: D=%d with %d heads not supported (peneo_pair_mxfp8_save_supported)", desc->D, desc->num_heads);
  PENEO_REQUIRE(act && x_rows, "peneo_pair_heads_fwd_mxfp8_save: null act / x_rows");
  PENEO_REQUIRE(desc->w_packed && desc->b1 && desc->b2, "peneo_pair_heads_fwd_mxfp8_save: null weights");
  PENEO_REQUIRE((reinterpret_cast<uintptr_t>(desc->w_packed) & 15) == 0 && (reinterpret_cast<uintptr_t>(ab) & 15) == 0 &&
                (reinterpret_cast<uintptr_t>(act) & 15) == 0 && (reinterpret_cast<uintptr_t>(x_rows) & 15) == 0,
                "peneo_pair_heads_fwd_mxfp8_save: ab / packed weights / act / x_rows must be 16-byte aligned");
  PENEO_REQUIRE(desc->drop_p >= 0.f && desc->drop_p < 1.f, "peneo_pair_heads_fwd_mxfp8_save: drop_p must be in [0, 1)");
  MxSaveParams q = {};
  MxFwdParams& p = q.f;
  p.ab = static_cast<const bf16_t*>(ab); p.B = B; p.N = N; p.D = desc->D; p.P = (int64_t)N * (N + 1) / 2;
  p.num_heads = desc->num_heads;
  PENEO_REQUIRE(p.P * (desc->num_heads * desc->D / 16) < ((int64_t)1 << 32), "peneo_pair_heads_fwd_mxfp8_save: pair space too large for the dropout counter");
  p.wp = static_cast<const char*>(desc->w_packed); p.b1 = desc->b1; p.b2 = desc->b2;
  q.drop_thr16 = pair_drop_thr16_host(desc->drop_p); q.drop_seed = desc->drop_seed; q.drop_scale = pair_drop_scale_host(desc->drop_p);
  q.act = static_cast<char*>(act); q.x_save = static_cast<bf16_t*>(x_rows); q.ntiles = pb_num_tiles(N);
  int tc = 0;
  for (int h = 0; h < desc->num_heads; ++h) {
    PENEO_REQUIRE(desc->classes[h] >= 1 && desc->classes[h] <= 4, "peneo_pair_heads_fwd_mxfp8_save: classes[%d] must be 1..4", h);
    p.classes[h] = desc->classes[h]; tc += desc->classes[h];
    p.logits[h] = logits ? logits[h] : nullptr;
    if (loss) { p.tags[h] = loss->tags[h]; p.cw[h] = loss->class_weight[h]; q.dlogits[h] = loss->dlogits[h]; }
  }
  PENEO_REQUIRE(tc <= MX_NCP, "peneo_pair_heads_fwd_mxfp8_save: more than %d classes in total", MX_NCP);
  if (loss) {
    p.partials = loss->partials;
    bool any = false;
    for (int h = 0; h < desc->num_heads; ++h) any = any || loss->tags[h];
    if (any) PENEO_REQUIRE(p.partials, "peneo_pair_heads_fwd_mxfp8_save: loss->partials workspace missing");
  }
  // only the width the saved backward exists for is instantiated (peneo_pair_mxfp8_save_supported)
  return launch_mx_save<6>(q, (hipStream_t)stream);
}
