// MXFP8 eval path of the five pair-classifier heads for decoder widths 512 < D <= 1024 (peneo_decoder_shrink = False: D = 768 /
// 960 / 1024): K11 + K12 + K13 forward, no dropout, no backward.
//
// The contract is peneo_pair_heads_fwd_mxfp8's (pair_heads_mx.hip, whose comment block has the operand maps of the scaled MFMA and
// the quantizer): x = SiLU(a_i + b_j) and W1cat as OCP MX e4m3 in blocks of 32 along D, fp32 accumulation on
// v_mfma_scale_f32_32x32x64_f8f6f4 in k-step order, + b1, SiLU, the bf16 second layer, + b2, the class-weighted CE row of 256 pairs.
//
// What differs is the budget.  x takes D / 8 registers per lane and 32 pairs: 96 / 120 / 128 at D = 768 / 960 / 1024.  The narrow
// kernel's eight waves of 32 pairs have 256 registers each, and the compiler does not fit x + accumulators + fragments in flight into
// them at these widths (it spills 219 .. 376 registers).  So the workgroup has FOUR waves, one per SIMD (__launch_bounds__(256, 1): up
// to 512 unified registers a lane), and each wave holds TWO groups of 32 pairs (lane & 31 = pair, group g of wave w = pairs
// 128 g + 32 w + 0..31 of the workgroup's 256): x takes 2 x D / 8 <= 256 registers, every weight fragment read from LDS feeds two
// MFMAs, and the workgroup's 256 pairs - one row of loss partials, peneo_pair_loss_partials - share ONE pass over every weight slab
// (pair_heads_wide.hip, bf16, walks them in two rounds and streams every slab twice).
//
// Packed weights (peneo_pair_heads_pack_mxfp8_wide): the slab of pair_heads_mx.h, one per 32 hidden units of the nh * D -
//   KS8 = D / 64 first-layer fragments of 2 KiB: byte (c * 1024 + lane * 16 + t) of fragment ks =
//        e4m3(W1cat[slab * 32 + (lane & 31)][64 ks + 32 c + 16 (lane >> 5) + t])        (c = K-block of the step, t = 0..15)
//   NSW = ceil(KS8 / 4) scale words of 256 B: byte (ks & 3) of word [ks >> 2][lane] = E8M0 of row slab * 32 + (lane & 31),
//        block 2 ks + (lane >> 5)
//   2 bf16 second-layer fragments of 1 KiB (the bf16 pack's fragments KS, KS + 1)
// - padded to a whole number of 4 KiB, so every one of the four waves moves the same number of 1 KiB DMA pieces: 24 .. 36 KiB a slab
// (28 at D = 768, 36 at 960 and 1024).  The narrow pack pads to 8 KiB; the two images differ in nothing else.
// LDS: a ring of three slabs + the b1 table (nh * D floats): 99 / 126.75 / 128 KiB for five heads at D = 768 / 960 / 1024.
// Slabs s + 1 and s + 2 stream L2 -> LDS (LDS-DMA) while the MFMAs of slab s run; one barrier per slab.
// Bias + SiLU of slab s run between the MFMAs of slab s + 1 (the one wave of a SIMD has no partner wave to hide them behind).
//
// No exit and no break: a workgroup past P does not exist (grid = ceil(P / 256)), and a pair past P is the clamped pair P - 1,
// computed and never written.
#include <stdlib.h>

#include "common.h"
#include "pair_heads_mx.h"

namespace peneo {
namespace {

constexpr int MXW_WAVES = 4;
constexpr int MXW_GROUPS = 2;                          // groups of 32 pairs per wave
constexpr int MXW_PAIRS = MXW_WAVES * MXW_GROUPS * 32; // 256: the loss partial rows are peneo_pair_loss_partials(B, N)
constexpr int MXW_NSTAGE = 3;
constexpr int MXW_MIN_KS = 9, MXW_MAX_KS = 16;         // 512 < D <= 1024

__host__ __device__ constexpr int mxw_upw(int ks8) { return mx_upw_t<MXW_WAVES>(ks8); }
__host__ __device__ constexpr int mxw_slab_bytes(int ks8) { return mx_slab_bytes_t<MXW_WAVES>(ks8); }
constexpr size_t mxw_lds_bytes(int D, int num_heads) {
  return (size_t)MXW_NSTAGE * mxw_slab_bytes(D / 64) + (size_t)num_heads * D * sizeof(float);
}

template <int KS8>
__global__ __launch_bounds__(MXW_WAVES * 64, 1) void pair_heads_mx_wide_kernel(MxFwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NSW = mx_scale_words(KS8), UPW = mxw_upw(KS8), SLAB = mxw_slab_bytes(KS8), NSTAGE = MXW_NSTAGE;
  constexpr int D = KS8 * 64;
  static_assert(KS8 >= MXW_MIN_KS && KS8 <= MXW_MAX_KS, "512 < D <= 1024, D a multiple of 64");
  static_assert(UPW <= 12 && (NSTAGE - 2) * UPW < 64, "slab too large for the vm counter");
  char* sW = smem;                                                    // [NSTAGE][SLAB]
  float* sB1 = reinterpret_cast<float*>(smem + NSTAGE * SLAB);        // [nh * D]
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, b = blockIdx.y;
  const int nslab = p.num_heads * D / 32;

  for (int i = tid; i < p.num_heads * D; i += MXW_WAVES * 64) sB1[i] = p.b1[i];

  // ---- x = SiLU(a_i + b_j) of the wave's two groups, quantized to MXFP8 straight into B-operand registers exactly as in
  //      pair_heads_mx_fwd_kernel: lane (c, half) of k-step ks holds k = 64 ks + 32 kb + 16 half + t (kb = 0, 1; t = 0..15); block
  //      kb's amax meets its other 16 elements in lane ^ 32, and this lane provides the scale of block kb = half ----
  const bf16_t* abd = p.ab + (int64_t)b * N * 2 * D;
  int64_t mypair[MXW_GROUPS];
  bool pair_ok[MXW_GROUPS];
  i32x8_t xf[MXW_GROUPS][KS8];
  uint32_t xs[MXW_GROUPS][NSW];
  mx_static_for<0, MXW_GROUPS>([&](auto gc) {
    constexpr int g = decltype(gc)::value;
    mypair[g] = (int64_t)blockIdx.x * MXW_PAIRS + g * (MXW_WAVES * 32) + wave * 32 + (lane & 31);
    pair_ok[g] = mypair[g] < p.P;
    int pi, pj;
    pair_decode(pair_ok[g] ? mypair[g] : p.P - 1, N, pi, pj);
    const bf16_t* arow = abd + (int64_t)pi * 2 * D;
    const bf16_t* brow = abd + (int64_t)pj * 2 * D + D;
#pragma unroll
    for (int w = 0; w < NSW; ++w) xs[g][w] = 0u;
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
        if (kb == half) xs[g][ks >> 2] |= sb << (8 * (ks & 3));
      }
      // the finished fragment is pinned where it is made: left alone, the compiler sinks the conversions into the slab loop's
      // preheader (the first use) and keeps the 32 fp32 values of every k-step alive until there - they spill
#pragma unroll
      for (int w = 0; w < 8; ++w) { asm volatile("" : "+v"(q[w]) :: "memory"); xf[g][ks][w] = (int)q[w]; }
      __builtin_amdgcn_sched_barrier(0);   // few gathers in flight at a time (else their raw data spills)
    }
#pragma unroll
    for (int w = 0; w < NSW; ++w) asm volatile("" : "+v"(xs[g][w]));
  });
  // every ordinary global load above has been consumed: from here on the vm counter only sees our DMA pieces
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();   // sB1 visible

  const char* wsrc = p.wp + wave * (UPW * 1024) + lane * 16;
  const uint32_t wdst = lds_addr(sW) + wave * (UPW * 1024);
#pragma unroll
  for (int s0 = 0; s0 < NSTAGE - 1; ++s0)
    if (s0 < nslab) lds_dma_units<0, UPW>(wsrc + (int64_t)s0 * SLAB, wdst + s0 * SLAB);

  f32x16_t lg[MXW_GROUPS];   // logits^T[class, pair]
#pragma unroll
  for (int g = 0; g < MXW_GROUPS; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) lg[g][r] = 0.f;

  // The SiLU of a slab runs one slab late: the one wave of a SIMD has nobody to overlap its VALU work with, so the accumulators of
  // slab s (zp), its bias row (bp) and its two second-layer fragments (w2p: read into registers, and the reads retired, before the
  // barrier behind which their ring slot is refilled) are
  // carried into slab s + 1, where bias + SiLU of the 32 values is spread between the MFMAs of the k-steps.  Slab 0 carries zeros:
  // SiLU(0) = 0 times a zero fragment adds +0 to the logits.  Same operations on the same values in the same order as without it.
  f32x16_t zp[MXW_GROUPS];
  float bp[16];
  Frag<bf16_t> w2p[2];
#pragma unroll
  for (int g = 0; g < MXW_GROUPS; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) zp[g][r] = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) bp[r] = 0.f;
  w2p[0].v = make_uint4(0u, 0u, 0u, 0u); w2p[1].v = make_uint4(0u, 0u, 0u, 0u);
  float yp[MXW_GROUPS][16];
  auto silu_slice = [&](auto lo_c, auto hi_c) {   // values lo .. hi - 1 of the 32 carried ones (16 g + r)
    constexpr int lo = decltype(lo_c)::value, hi = decltype(hi_c)::value;
#pragma unroll
    for (int v = lo; v < hi; ++v) yp[v >> 4][v & 15] = silu_f(zp[v >> 4][v & 15] + bp[v & 15]);
  };
  auto second_layer = [&]() {
#pragma unroll
    for (int g = 0; g < MXW_GROUPS; ++g) {
      mma_step(w2p[0], pack_frag8<bf16_t>(yp[g]), lg[g]);
      mma_step(w2p[1], pack_frag8<bf16_t>(yp[g] + 8), lg[g]);
    }
  };

  for (int slab = 0; slab < nslab; ++slab) {
    // slabs slab .. slab + NSTAGE - 2 are in flight (fewer at the end): wait for the oldest, then publish it
    if (slab + 1 < nslab) wait_vm<(NSTAGE - 2) * UPW>(); else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (slab + NSTAGE - 1 < nslab) lds_dma_units<0, UPW>(wsrc + (int64_t)(slab + NSTAGE - 1) * SLAB, wdst + ((slab + NSTAGE - 1) % NSTAGE) * SLAB);
    const char* wb = sW + (slab % NSTAGE) * SLAB;
    uint32_t ws[NSW];
#pragma unroll
    for (int w = 0; w < NSW; ++w) ws[w] = *reinterpret_cast<const uint32_t*>(wb + KS8 * 2048 + w * 256 + lane * 4);
    f32x16_t z[MXW_GROUPS];
#pragma unroll
    for (int g = 0; g < MXW_GROUPS; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) z[g][r] = 0.f;
    // the fragment of step ks + 1 is read in front of the two MFMAs of step ks, which cover its latency for the one wave of the
    // SIMD; the sched_barrier keeps the compiler from hoisting every read of the slab to its top (16 registers each)
    auto read_frag = [&](int ks) {
      const uint4 lo = *reinterpret_cast<const uint4*>(wb + ks * 2048 + lane * 16);
      const uint4 hi = *reinterpret_cast<const uint4*>(wb + ks * 2048 + 1024 + lane * 16);
      return i32x8_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    };
    i32x8_t wf[2];
    wf[0] = read_frag(0);
    mx_static_for<0, KS8>([&](auto kc) {
      constexpr int ks = decltype(kc)::value;
      if constexpr (ks + 1 < KS8) wf[(ks + 1) & 1] = read_frag(ks + 1);
#pragma unroll
      for (int g = 0; g < MXW_GROUPS; ++g)
        z[g] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[ks & 1], xf[g][ks], z[g], 0, 0, ks & 3, (int)ws[ks >> 2], ks & 3, (int)xs[g][ks >> 2]);
      // the carried slab's share of this step: its VALU work runs in the shadow of the two MFMAs
      silu_slice(std::integral_constant<int, ks * 32 / KS8>{}, std::integral_constant<int, (ks + 1) * 32 / KS8>{});
      __builtin_amdgcn_sched_barrier(0);
    });
    second_layer();   // of the carried slab; accumulator rows 8q + 4 half + 0..3 are the second layer's B operand (pack order)
    // carry this slab
    const char* w2 = wb + KS8 * 2048 + NSW * 256;
    w2p[0] = load_frag_linear<bf16_t>(w2, 0, lane); w2p[1] = load_frag_linear<bf16_t>(w2, 1, lane);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 bv = *reinterpret_cast<const float4*>(sB1 + slab * 32 + 8 * q + 4 * half);
      bp[4 * q + 0] = bv.x; bp[4 * q + 1] = bv.y; bp[4 * q + 2] = bv.z; bp[4 * q + 3] = bv.w;
    }
    // the ring slot these reads come from is refilled right behind the next barrier (slab + NSTAGE), one phase after them, and
    // s_barrier does not drain the LDS counter: the reads are retired here, before this wave can arrive there
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int g = 0; g < MXW_GROUPS; ++g) zp[g] = z[g];
  }
  silu_slice(std::integral_constant<int, 0>{}, std::integral_constant<int, 32>{});   // the last slab's
  second_layer();
  // (no DMA is in flight: the last slab issues none, and its pieces were waited for; the epilogue's sums reuse the ring behind a
  // barrier.)  The second group adds its sums to the workgroup's row of partials: same writers, same addresses
  mx_epilogue<MXW_WAVES>(p, lg[0], smem, tid, lane, wave, half, b, mypair[0], pair_ok[0]);
  mx_epilogue<MXW_WAVES, true>(p, lg[1], smem, tid, lane, wave, half, b, mypair[1], pair_ok[1]);
}

template <int KS8>
int launch_mx_wide(const MxFwdParams& p, hipStream_t st) {
  const size_t sh = mxw_lds_bytes(p.D, p.num_heads);
  if (raise_dynamic_lds(pair_heads_mx_wide_kernel<KS8>, sh, "peneo_pair_heads_fwd_mxfp8_wide") != PENEO_OK) return PENEO_ERR_LAUNCH;
  dim3 grid((unsigned)((p.P + MXW_PAIRS - 1) / MXW_PAIRS), p.B);
  hipLaunchKernelGGL((pair_heads_mx_wide_kernel<KS8>), grid, dim3(MXW_WAVES * 64), sh, st, p);
  return check_launch("peneo_pair_heads_fwd_mxfp8_wide");
}

}  // namespace
}  // namespace peneo

using namespace peneo;

extern "C" int peneo_pair_mxfp8_wide_supported(int D, int num_heads) {
  if (num_heads < 1 || num_heads > PENEO_MAX_HEADS || D < 64 * MXW_MIN_KS || D > 64 * MXW_MAX_KS || D % 64 != 0) return 0;
  return mxw_lds_bytes(D, num_heads) <= 160 * 1024 ? 1 : 0;
}

extern "C" size_t peneo_pair_heads_mxfp8_wide_packed_bytes(int num_heads, int D) {
  if (!peneo_pair_mxfp8_wide_supported(D, num_heads)) return 0;
  return (size_t)(num_heads * D / 32) * (size_t)mxw_slab_bytes(D / 64);
}

extern "C" int peneo_pair_heads_pack_mxfp8_wide(const float* const* w1, const float* const* w2, const int* classes, int num_heads,
                                                int D, void* packed, peneo_stream_t stream) {
  PENEO_REQUIRE(w1 && w2 && classes && packed, "peneo_pair_heads_pack_mxfp8_wide: bad arguments");
  PENEO_REQUIRE(peneo_pair_mxfp8_wide_supported(D, num_heads), "peneo_pair_heads_pack_mxfp8_wide: D=%d with %d heads not supported (peneo_pair_mxfp8_wide_supported)", D, num_heads);
  PENEO_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, "peneo_pair_heads_pack_mxfp8_wide: packed must be 16-byte aligned");
  MxPackSrc s = {};
  s.num_heads = num_heads; s.D = D;
  int tc = 0;
  for (int h = 0; h < num_heads; ++h) {
    PENEO_REQUIRE(w1[h] && w2[h], "peneo_pair_heads_pack_mxfp8_wide: null weight pointer for head %d", h);
    PENEO_REQUIRE(classes[h] >= 1 && classes[h] <= 4, "peneo_pair_heads_pack_mxfp8_wide: classes[%d] must be 1..4", h);
    s.w1[h] = w1[h]; s.w2[h] = w2[h]; s.classes[h] = classes[h]; tc += classes[h];
  }
  PENEO_REQUIRE(tc <= MX_NCP, "peneo_pair_heads_pack_mxfp8_wide: more than %d classes in total", MX_NCP);
  const hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(packed, 0, peneo_pair_heads_mxfp8_wide_packed_bytes(num_heads, D), st) != hipSuccess) {
    set_error("peneo_pair_heads_pack_mxfp8_wide: hipMemsetAsync failed");
    return PENEO_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(mx_pack_w1_kernel<MXW_WAVES>, dim3(mx_blocks((int64_t)num_heads * D * (D / 32))), dim3(256), 0, st, s, static_cast<char*>(packed));
  hipLaunchKernelGGL(mx_pack_w2_kernel<MXW_WAVES>, dim3(mx_blocks((int64_t)(num_heads * D / 32) * 1024)), dim3(256), 0, st, s, static_cast<char*>(packed));
  return check_launch("peneo_pair_heads_pack_mxfp8_wide");
}

extern "C" int peneo_pair_heads_fwd_mxfp8_wide(const void* ab, int B, int N, const peneo_pair_heads_desc* desc, float* const* logits,
                                               const peneo_pair_loss* loss, peneo_stream_t stream) {
  PENEO_REQUIRE(ab && desc && B > 0 && N > 0, "peneo_pair_heads_fwd_mxfp8_wide: bad arguments");
  PENEO_REQUIRE(peneo_pair_mxfp8_wide_supported(desc->D, desc->num_heads), "peneo_pair_heads_fwd_mxfp8_wide: D=%d with %d heads not supported (peneo_pair_mxfp8_wide_supported)", desc->D, desc->num_heads);
  PENEO_REQUIRE(desc->w_packed && desc->b1 && desc->b2, "peneo_pair_heads_fwd_mxfp8_wide: null weights");
  PENEO_REQUIRE((reinterpret_cast<uintptr_t>(desc->w_packed) & 15) == 0 && (reinterpret_cast<uintptr_t>(ab) & 15) == 0,
                "peneo_pair_heads_fwd_mxfp8_wide: ab / packed weights must be 16-byte aligned");
  PENEO_REQUIRE(desc->drop_p == 0.f, "peneo_pair_heads_fwd_mxfp8_wide: eval only, drop_p must be 0");
  MxFwdParams p = {};
  p.ab = static_cast<const bf16_t*>(ab); p.B = B; p.N = N; p.D = desc->D; p.P = (int64_t)N * (N + 1) / 2;
  p.num_heads = desc->num_heads;
  p.wp = static_cast<const char*>(desc->w_packed); p.b1 = desc->b1; p.b2 = desc->b2;
  int tc = 0;
  for (int h = 0; h < desc->num_heads; ++h) {
    PENEO_REQUIRE(desc->classes[h] >= 1 && desc->classes[h] <= 4, "peneo_pair_heads_fwd_mxfp8_wide: classes[%d] must be 1..4", h);
    p.classes[h] = desc->classes[h]; tc += desc->classes[h];
    p.logits[h] = logits ? logits[h] : nullptr;
    if (loss) {
      PENEO_REQUIRE(!loss->dlogits[h], "peneo_pair_heads_fwd_mxfp8_wide: eval only, dlogits must be NULL");
      p.tags[h] = loss->tags[h]; p.cw[h] = loss->class_weight[h];
    }
  }
  PENEO_REQUIRE(tc <= MX_NCP, "peneo_pair_heads_fwd_mxfp8_wide: more than %d classes in total", MX_NCP);
  if (loss) {
    p.partials = loss->partials;
    bool any = false;
    for (int h = 0; h < desc->num_heads; ++h) any = any || loss->tags[h];
    if (any) PENEO_REQUIRE(p.partials, "peneo_pair_heads_fwd_mxfp8_wide: loss->partials workspace missing");
  }
  const hipStream_t st = (hipStream_t)stream;
  switch (desc->D / 64) {
    case 9: return launch_mx_wide<9>(p, st);
    case 10: return launch_mx_wide<10>(p, st);
    case 11: return launch_mx_wide<11>(p, st);
    case 12: return launch_mx_wide<12>(p, st);
    case 13: return launch_mx_wide<13>(p, st);
    case 14: return launch_mx_wide<14>(p, st);
    case 15: return launch_mx_wide<15>(p, st);
    default: return launch_mx_wide<16>(p, st);
  }
}
