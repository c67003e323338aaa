// K11 + K12 + K13 fused for decoder widths 512 < D <= 1024 (peneo_decoder_shrink = False: D = 768 / 960 / 1024), bf16.
//
// The contract is peneo_pair_heads_fwd's (pair_heads.hip): per pair x = SiLU(a_i + b_j), z = W1cat x + b1, y = SiLU(z), the K12
// dropout, logits = s (W2 y) + b2, class-weighted CE, un-normalised dlogits, one row of 32 partial sums per workgroup.
//
// What differs is the budget.  x stays in registers as bf16 MFMA B fragments, 4 registers per 16 of D and lane: 192 at D = 768, 240
// at 960, 256 at 1024 - more than the 256 a wave of an eight-wave workgroup can have.  So the workgroup has FOUR waves, one per SIMD
// (__launch_bounds__(256, 1): up to 512 unified registers a lane), each with 32 pairs (lane & 31 = pair), and walks its 256 pairs
// - the pairs of one row of loss partials, peneo_pair_loss_partials - in two rounds of 4 x 32.
//
// Packed weights (peneo_pair_heads_pack for these D): the slabs of pack_weights_kernel, one per 32 hidden units of the nh * D,
//   fragment ks < D / 16 : W1cat[slab * 32 + (lane & 31)][16 ks + 8 (lane >> 5) + e]
//   fragment D / 16 + kk : W2full[class = lane & 31][hidden = slab * 32 + 16 kk + (e & 3) + 8 (e >> 2) + 4 (lane >> 5)]
// (64 lanes x 8 bf16 = 1 KiB a fragment), each slab zero-padded to pair_wide_slab_bytes(D): a whole number of 4 KiB, so every wave
// moves the same number of 1 KiB pieces (52 / 64 / 68 KiB a slab at D = 768 / 960 / 1024).
// LDS: a ring of two slabs + the b1 table (nh * D floats): 119 / 147 / 156 KiB for five heads; a ring of three does not fit.
// The slab of step s + 1 streams L2 -> LDS (LDS-DMA) while the MFMAs of step s run; one barrier per slab.
// The kernel is compiler-scheduled: nothing is interleaved by hand.
#include "common.h"
#include "pair_heads.h"

namespace peneo {

constexpr int PW_WAVES = 4;
constexpr int PW_ROUND = PW_WAVES * 32;    // pairs per round
constexpr int PW_PAIRS = 2 * PW_ROUND;     // pairs per workgroup == pairs per row of loss partials (pair_heads.hip: PH_PAIRS)

// LENS (peneo_pair_heads_fwd_lens, no dropout): the workgroup's 256 pairs are local pairs of the n_b-token document (pair_heads.h)
template <int KS, bool DROP, bool LENS = false>
__global__ __launch_bounds__(PW_WAVES * 64, 1) void pair_heads_wide_kernel(PairFwdParams p) {
  static_assert(!LENS || !DROP, "the length-aware walk is an inference form");
  using T = bf16_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int UPW = (KS + 2 + PW_WAVES - 1) / PW_WAVES;   // 1 KiB DMA pieces per wave per slab
  constexpr int SLAB_BYTES = UPW * PW_WAVES * 1024;         // == pair_wide_slab_bytes(16 KS)
  static_assert(KS % 4 == 0 && KS > 32 && KS <= 64, "512 < D <= 1024, D a multiple of 64");
  char* sW = smem;                                                 // [2][SLAB_BYTES]
  float* sB1 = reinterpret_cast<float*>(smem + 2 * SLAB_BYTES);    // [nh * D]
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = p.D, N = p.N;
  const int b = blockIdx.y;
  const int nslab = p.num_heads * D / 32;
  const T* abd = reinterpret_cast<const T*>(p.ab) + (int64_t)b * N * 2 * D;
  [[maybe_unused]] int nb = 0;
  [[maybe_unused]] int64_t Pb = 0;
  if constexpr (LENS) {
    nb = pair_lens_doc(p, b);
    Pb = (int64_t)nb * (nb + 1) / 2;
    // (uniform over the workgroup; before any barrier or DMA)
    if ((int64_t)blockIdx.x * PW_PAIRS >= Pb) { pair_lens_zero_row(p, b, tid); return; }
  }

  for (int i = tid; i < p.num_heads * D; i += PW_WAVES * 64) sB1[i] = p.b1[i];

  const char* wsrc = reinterpret_cast<const char*>(p.wp) + wave * (UPW * 1024) + lane * 16;
  const uint32_t wdst = lds_addr(sW) + wave * (UPW * 1024);
  auto dma = [&](int slab_, int buf_) { lds_dma_units<0, UPW>(wsrc + (int64_t)slab_ * SLAB_BYTES, wdst + buf_ * SLAB_BYTES); };
  const uint32_t drop_key = DROP ? pair_drop_key(p.drop_seed, b) : 0u;

  for (int round = 0; round < 2; ++round) {
    const int64_t p0 = (int64_t)blockIdx.x * PW_PAIRS + round * PW_ROUND;
    // (LENS is a constant: the plain instantiations keep their statements, each where it stood - this kernel is compiler-scheduled,
    // and a reordered form of the same walk came out 300 to 750 instructions longer per kernel)
    if (p0 >= (LENS ? Pb : p.P)) break;                     // (uniform over the workgroup)
    const int64_t qpair = p0 + wave * 32 + (lane & 31);     // the pair within the document as it is walked
    const bool pair_ok = qpair < (LENS ? Pb : p.P);
    int pi, pj;
    pair_decode(pair_ok ? qpair : (LENS ? Pb : p.P) - 1, LENS ? nb : N, pi, pj);
    int64_t packed = qpair;                                 // what the epilogue indexes by: N-packed
    if constexpr (LENS) { packed = pair_row_start(pi, N) + (pj - pi); asm volatile("" : "+v"(packed)); }   // (made here, not later)
    const int64_t mypair = packed;

    // ---- x = SiLU(a_i + b_j) as B-operand fragments (k = decoder dim), kept in registers ----
    const T* arow = abd + (int64_t)pi * 2 * D;
    const T* brow = abd + (int64_t)pj * 2 * D + D;
    Frag<T> xf[KS];
    {
      // groups of 4 k-steps, raw 16-byte gathers double-buffered by hand, each finished fragment pinned where it is made (as in
      // pair_heads_fwd_kernel: left alone, the compiler hoists every gather to the top and the raw data spills)
      uint4 ra[2][4], rb[2][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[0][i] = *reinterpret_cast<const uint4*>(arow + 16 * i + 8 * half);
        rb[0][i] = *reinterpret_cast<const uint4*>(brow + 16 * i + 8 * half);
      }
#pragma unroll
      for (int g = 0; g < KS / 4; ++g) {
        if (g + 1 < KS / 4) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            ra[(g + 1) & 1][i] = *reinterpret_cast<const uint4*>(arow + 16 * (4 * (g + 1) + i) + 8 * half);
            rb[(g + 1) & 1][i] = *reinterpret_cast<const uint4*>(brow + 16 * (4 * (g + 1) + i) + 8 * half);
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float a[8], bb[8];
          unpack16<T>(ra[g & 1][i], a);
          unpack16<T>(rb[g & 1][i], bb);
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = silu_f(a[e] + bb[e]);
          xf[4 * g + i] = pack_frag8<T>(a);
          asm volatile("" : "+v"(xf[4 * g + i].v.x), "+v"(xf[4 * g + i].v.y), "+v"(xf[4 * g + i].v.z), "+v"(xf[4 * g + i].v.w) :: "memory");
        }
      }
    }
    // every ordinary global load above has been consumed: from here on the vm counter only sees our DMA pieces
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                        // sB1 visible; every wave has left the ring of the round before
    dma(0, 0);

    f32x16_t lg;                                            // logits^T[class, pair]
#pragma unroll
    for (int r = 0; r < 16; ++r) lg[r] = 0.f;
    const uint32_t drop_base = (uint32_t)(mypair * nslab * 2) + (uint32_t)half;

    for (int slab = 0; slab < nslab; ++slab) {
      wait_vm<0>();                                         // this wave's pieces of `slab` have landed ...
      __builtin_amdgcn_s_barrier();                         // ... and everybody's; every wave is done with slab - 1
      __builtin_amdgcn_sched_barrier(0);
      if (slab + 1 < nslab) dma(slab + 1, (slab + 1) & 1);
      const char* wb = sW + (slab & 1) * SLAB_BYTES;
      f32x16_t z;
#pragma unroll
      for (int r = 0; r < 16; ++r) z[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) mma_step(load_frag_linear<T>(wb, ks, lane), xf[ks], z);
      // bias + SiLU (+ K12 dropout) in registers: the C-layout accumulator of the slab is the B operand of the second layer
      float y[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {   // accumulator rows 8g + 4*half + 0..3 -> one 16-byte bias read
        const float4 bv = *reinterpret_cast<const float4*>(sB1 + slab * 32 + 8 * g + 4 * half);
        y[4 * g + 0] = silu_f(z[4 * g + 0] + bv.x);
        y[4 * g + 1] = silu_f(z[4 * g + 1] + bv.y);
        y[4 * g + 2] = silu_f(z[4 * g + 2] + bv.z);
        y[4 * g + 3] = silu_f(z[4 * g + 3] + bv.w);
      }
      if constexpr (DROP) {
        // this lane's 16 hidden units of the slab (rows 8g + 4 half + e, y[4g + e]) are the 16 fields of ONE chain (common.h); the
        // 1 / (1 - p) factor is applied to the logits
        uint32_t st = pair_drop_seed(drop_key, drop_base + 2u * (uint32_t)slab);
        const uint32_t inc = pair_drop_inc(drop_key, drop_base + 2u * (uint32_t)slab);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          st = pair_drop_step(st, inc);
          y[i] = (st >> 16) >= p.drop_thr16 ? y[i] : 0.f;
        }
      }
      mma_step(load_frag_linear<T>(wb, KS, lane), pack_frag8<T>(y), lg);
      mma_step(load_frag_linear<T>(wb, KS + 1, lane), pack_frag8<T>(y + 8), lg);
    }

    // (no DMA is in flight: the last slab of a round issues none, and its pieces were waited for; the epilogue's sums reuse the
    // ring behind a barrier.)  The second round adds its sums to the workgroup's row of partials: same writers, same addresses
    pair_epilogue_t<PW_WAVES>(p, lg, smem, tid, lane, wave, half, b, mypair, pair_ok, round != 0);
  }
}

static size_t pair_wide_lds_bytes(int D, int num_heads) {
  return 2 * (size_t)pair_wide_slab_bytes(D) + (size_t)num_heads * D * sizeof(float);
}

bool pair_wide_supported(int dtype, int D, int num_heads) {
  return dtype == PENEO_BF16 && D > 512 && D <= 1024 && D % 64 == 0 && num_heads >= 1 && num_heads <= PENEO_MAX_HEADS &&
         pair_wide_lds_bytes(D, num_heads) <= 160 * 1024;
}

template <int KS, bool DROP, bool LENS = false>
static int launch_pair_wide(const PairFwdParams& p, hipStream_t st) {
  constexpr const char* who = LENS ? "peneo_pair_heads_fwd_lens" : "peneo_pair_heads_fwd";
  const size_t sh = pair_wide_lds_bytes(p.D, p.num_heads);
  if (raise_dynamic_lds(pair_heads_wide_kernel<KS, DROP, LENS>, sh, who) != PENEO_OK) return PENEO_ERR_LAUNCH;
  dim3 grid((unsigned)((p.P + PW_PAIRS - 1) / PW_PAIRS), p.B);
  hipLaunchKernelGGL((pair_heads_wide_kernel<KS, DROP, LENS>), grid, dim3(PW_WAVES * 64), sh, st, p);
  return check_launch(who);
}

int pair_wide_fwd(const PairFwdParams& p, hipStream_t st, bool lens_walk) {
  if (!pair_wide_supported(PENEO_BF16, p.D, p.num_heads) || p.act) {
    set_error("peneo_pair_heads_fwd: D=%d with %d heads not supported by the wide kernel", p.D, p.num_heads);
    return PENEO_ERR_INVALID;
  }
  // (lens_walk: peneo_pair_heads_fwd_lens, which has refused dropout)
#define PENEO_PW_CASE(KS_) \
  case KS_: return lens_walk ? launch_pair_wide<KS_, false, true>(p, st) : p.drop_thr16 ? launch_pair_wide<KS_, true>(p, st) : launch_pair_wide<KS_, false>(p, st);
  switch (p.D / 16) {
    PENEO_PW_CASE(36) PENEO_PW_CASE(40) PENEO_PW_CASE(44) PENEO_PW_CASE(48)
    PENEO_PW_CASE(52) PENEO_PW_CASE(56) PENEO_PW_CASE(60) PENEO_PW_CASE(64)
    default: set_error("peneo_pair_heads_fwd: D=%d not supported", p.D); return PENEO_ERR_INVALID;
  }
#undef PENEO_PW_CASE
}

}  // namespace peneo
