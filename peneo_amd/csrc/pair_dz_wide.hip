// peneo_pair_dz_fused for decoder widths 512 < D <= 1024 (peneo_decoder_shrink = False: D = 768 / 960 / 1024), bf16.
//
// The contract is pair_dz_fused_kernel's (pair_heads.hip): for the pairs of rows [i0, i1) of one document x = SiLU(a_i + b_j) is kept
// as bf16 MFMA fragments, z = x W1cat^T comes off the matrix cores with the operands swapped (lane = hidden column, the 16 accumulator
// registers = 16 pairs), and per element z + b1, y = SiLU(z), dy = sum_c g_c W2[c], dz = dy SiLU'(z), the K12 mask and scale of common.h
// on dz and y.  dz leaves as bf16 rows of nh * D, the column sums (three dW2 rows, db1) are added to the caller's [rows][4 nh D]
// workspace, x / a_i + b_j are stored on request bit for bit as peneo_pair_x_fwd writes them.  Pairs past the chunk store nothing and
// add zero to every sum (their g is 0).
//
// The budget is the wide forward's (pair_heads_wide.hip): the x fragments are 4 registers per 16 of D and lane, 192 / 240 / 256 at
// D = 768 / 960 / 1024, so the workgroup has FOUR waves, one per SIMD (__launch_bounds__(256, 1)), 32 pairs each, and walks its
// 256 pairs (PH_PAIRS: peneo_pair_dz_fused_workspace_rows and the blockIdx % 256 row are what they are at D <= 512) in two rounds of
// 4 x 32.  The weights are the image peneo_pair_heads_pack writes for these widths, slab stride pair_wide_slab_bytes(D); the two
// second-layer fragments of a slab travel with it and are not read.
// LDS: a ring of two slabs (LDS-DMA, one s_waitcnt vmcnt(0) + one barrier per slab)
//      + the column table {W2 row 0, 1, 2, b1} of the CURRENT head only (16 D bytes; all heads do not fit beside two wide slabs),
//        rewritten at a head boundary behind the slab barrier, one more barrier per head
//      + sG (scale * dlogits of each wave's 32 pairs, current head) 2 KiB + sPart (two slabs of column sums) 4 KiB:
//      122 / 149 / 158 KiB at D = 768 / 960 / 1024 whatever the number of heads.
// The loop is rotated by one slab: iteration s runs the dz arithmetic of slab s - 1 (its stores leave first) and then the MFMAs of
// slab s, so the stores have the whole MFMA phase to retire before the next vmcnt(0).  Nothing else is interleaved by hand.
//
// Column sums: wave s % 4 adds the four waves' sums of slab s to the workgroup's workspace row, lanes 0..31, one fp32 atomic per
// address; the second round adds to the same addresses FROM THE SAME LANE, later in program order.  With a row per workgroup
// (deterministic mode, ws_own) every address therefore has a single writer whose adds are ordered: the launch is order-independent.
#include "common.h"
#include "pair_heads.h"

namespace peneo {

constexpr int DW_WAVES = 4;
constexpr int DW_ROUND = DW_WAVES * 32;    // pairs per round
constexpr int DW_PAIRS = 2 * DW_ROUND;     // pairs per workgroup == PH_PAIRS (pair_heads.hip)

template <int KS>
__global__ __launch_bounds__(DW_WAVES * 64, 1) void pair_dz_wide_kernel(DzFusedParams p) {
  using T = bf16_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int UPW = (KS + 2 + DW_WAVES - 1) / DW_WAVES;   // 1 KiB DMA pieces per wave per slab
  constexpr int SLAB_BYTES = UPW * DW_WAVES * 1024;         // == pair_wide_slab_bytes(16 KS)
  static_assert(KS % 4 == 0 && KS > 32 && KS <= 64, "512 < D <= 1024, D a multiple of 64");
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = p.D, N = p.N, nh = p.a.num_heads, ncol = nh * D;
  char* sW = smem;                                                   // [2][SLAB_BYTES]
  float4* sCol = reinterpret_cast<float4*>(smem + 2 * SLAB_BYTES);   // [D]: W2 rows 0..2 of the column, b1 (current head)
  float4* sG = sCol + D;                                             // [DW_WAVES][32]: scale * dlogits of the wave's pairs
  float4* sPart = sG + DW_WAVES * 32;                                // [2][DW_WAVES][32]: column sums of one slab
  const int nslab = ncol / 32, spb = D / 32;
  const uint32_t drop_thr = pair_drop_thr16_dev(p.a.drop_p);
  const uint32_t drop_key = pair_drop_key(p.a.drop_seed, p.a.drop_doc);
  const float drop_scale = drop_thr ? 65536.f / (65536.f - (float)drop_thr) : 1.f;
  const uint32_t drop_half = ((lane & 31) >> 2) & 1;                                  // unit w = lane & 31 of every slab:
  const PairDropJump drop_jump = pair_drop_jump(4 * ((lane & 31) >> 3) + (lane & 3));  // half (w >> 2) & 1, position 4 (w >> 3) + (w & 3)

  const char* wsrc = reinterpret_cast<const char*>(p.wp) + wave * (UPW * 1024) + lane * 16;
  const uint32_t wdst = lds_addr(sW) + wave * (UPW * 1024);
  auto dma = [&](int slab_, int buf_) {
    lds_dma_units<0, UPW>(wsrc + (int64_t)slab_ * SLAB_BYTES, __builtin_amdgcn_readfirstlane(wdst + buf_ * SLAB_BYTES));
  };
  float* slot = p.ws + (int64_t)(p.ws_own ? blockIdx.x : blockIdx.x % DZF_SLOTS) * 4 * ncol;
  // the wave that owns slab s adds the four waves' column sums of that slab to the workspace
  auto flush = [&](int s) {
    if (wave == (s & (DW_WAVES - 1)) && lane < 32) {
      const float4* src = sPart + (s & 1) * (DW_WAVES * 32) + lane;
      float4 t = src[0];
#pragma unroll
      for (int w = 1; w < DW_WAVES; ++w) { const float4 u = src[w * 32]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
      float* dst = slot + s * 32 + lane;
      atomicAdd(dst, t.x); atomicAdd(dst + ncol, t.y); atomicAdd(dst + 2 * (int64_t)ncol, t.z); atomicAdd(dst + 3 * (int64_t)ncol, t.w);
    }
  };
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 one2 = f2{1.f, 1.f}, nl2e = f2{-kLog2e, -kLog2e};
  const float4* myG = sG + wave * 32;
  const bool odd = (lane & 1) != 0;

  for (int round = 0; round < 2; ++round) {
    const int64_t r0p = (int64_t)blockIdx.x * DW_PAIRS + round * DW_ROUND;
    if (r0p >= p.npairs) break;                               // (uniform over the workgroup)
    const int64_t lp0 = r0p + wave * 32;                      // first local pair of the wave
    const int64_t lp = lp0 + (lane & 31);
    const bool pair_ok = lp < p.npairs;
    int pi, pj;
    pair_decode(p.pbase + (pair_ok ? lp : p.npairs - 1), N, pi, pj);

    // ---- x = SiLU(a_i + b_j) as MFMA fragments (k = decoder dim), kept in registers; each lane owns 16 contiguous bytes per k-step
    // of what the dW1 / dx GEMMs need as x and a_i + b_j ----
    const T* arow = p.abd + (int64_t)pi * 2 * D;
    const T* brow = p.abd + (int64_t)pj * 2 * D + D;
    const bool want_x = p.x_out != nullptr && pair_ok;
    bf16_t* x_row = p.x_out + lp * D + 8 * half;
    bf16_t* pre_row = p.pre_out + lp * D + 8 * half;
    Frag<T> xf[KS];
    {
      // groups of 4 k-steps, raw 16-byte gathers double-buffered by hand, each finished fragment pinned where it is made (as in
      // pair_heads_wide_kernel: left alone, the compiler hoists every gather to the top and the raw data spills)
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
          for (int e = 0; e < 8; ++e) a[e] += bb[e];
          if (want_x) *reinterpret_cast<uint4*>(pre_row + 16 * (4 * g + i)) = pack_frag8<T>(a).v;
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = silu_f(a[e]);
          xf[4 * g + i] = pack_frag8<T>(a);
          asm volatile("" : "+v"(xf[4 * g + i].v.x), "+v"(xf[4 * g + i].v.y), "+v"(xf[4 * g + i].v.z), "+v"(xf[4 * g + i].v.w) :: "memory");
          if (want_x) *reinterpret_cast<uint4*>(x_row + 16 * (4 * g + i)) = xf[4 * g + i].v;
        }
      }
    }
    // every ordinary global access above has retired: from here on the vm counter sees our DMA pieces, the dz stores and the atomics,
    // and every wait on it is a vmcnt(0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                          // every wave has left the ring, sCol and sPart of the round before
    dma(0, 0);

    const int nrows = (int)min((int64_t)32, p.npairs - lp0);  // valid pairs of this wave's tile (may be <= 0)
    const bool full_tile = nrows >= 32;
    // dz leaves as 4-byte stores: even lanes hold columns (c, c+1) of pair row 2j', odd lanes columns (c-1, c) of row 2j'+1
    // (neighbour lanes trade one value)
    bf16_t* orow2 = p.out + lp0 * ncol + (int64_t)(4 * half + (lane & 1)) * ncol + ((lane & 31) & ~1);

    // head h begins: its column table and this wave's g.  Called behind a barrier that every reader of the previous table has passed;
    // ends with the barrier that makes the new one visible.
    auto head_begin = [&](int h) {
      const int Cn = p.a.classes[h];
      const float* w2h = p.a.w2[h];
      for (int k = tid; k < D; k += DW_WAVES * 64)
        sCol[k] = make_float4(w2h[k], Cn > 1 ? w2h[(int64_t)D + k] : 0.f, Cn > 2 ? w2h[(int64_t)2 * D + k] : 0.f, p.b1[h * D + k]);
      if (lane < 32) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (pair_ok) {
          const float sc = p.a.scale[h];
          const float* dl = p.a.dlogits[h] + lp * Cn;
          gx = dl[0] * sc;
          if (Cn > 1) gy = dl[1] * sc;
          if (Cn > 2) gz = dl[2] * sc;
        }
        // two adjacent pairs share 8 floats {g0, g0', g1, g1', g2, g2', -, -}: the packed-fp32 operands come out of LDS already paired
        float* gp = reinterpret_cast<float*>(sG + wave * 32) + (lane >> 1) * 8 + (lane & 1);
        gp[0] = gx; gp[2] = gy; gp[4] = gz;
      }
      __syncthreads();
    };

    // dz arithmetic of slab es on the accumulator z (rows = pairs, columns = hidden units)
    auto epilogue = [&](const f32x16_t& z, int es) {
      const float4 cw = sCol[(es % spb) * 32 + (lane & 31)];
      const f2 w0 = f2{cw.x, cw.x}, w1 = f2{cw.y, cw.y}, w2 = f2{cw.z, cw.z}, b1 = f2{cw.w, cw.w};
      f2 s0 = f2{0.f, 0.f}, s1 = s0, s2 = s0, sb = s0;
      bf16_t* ocol = orow2 + es * 32;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r0 = 2 * j, rowc = (r0 & 3) + 8 * (r0 >> 2);   // accumulator registers 2j, 2j+1: pair rows rowc + 4*half + {0, 1}
        const int row0 = rowc + 4 * half;
        const float4 g01 = myG[row0];   // (row0 is even: float4 slots row0, row0 + 1 = that pair's 8 floats)
        const float2 g2v = *reinterpret_cast<const float2*>(myG + row0 + 1);
        const f2 g0 = f2{g01.x, g01.y}, g1 = f2{g01.z, g01.w}, g2 = f2{g2v.x, g2v.y};
        const f2 zz = f2{z[r0], z[r0 + 1]} + b1;
        const f2 t = zz * nl2e;
        const f2 den = f2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)} + one2;
        const f2 sg = f2{__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
        const f2 y = zz * sg;
        const f2 dy = __builtin_elementwise_fma(g2, w2, __builtin_elementwise_fma(g1, w1, g0 * w0));
        f2 dz = dy * (sg * __builtin_elementwise_fma(zz, one2 - sg, one2));
        if (drop_thr) {
          // the forward's classifier dropout: this lane's unit sits at a fixed chain position, its pairs vary
          const uint32_t cnt0 = (uint32_t)(((p.a.drop_pair0 + lp0 + row0) * nslab + es) * 2) + drop_half;
          const uint32_t cnt1 = cnt0 + 2u * (uint32_t)nslab;
          const f2 kk = f2{pair_drop_keep_at(pair_drop_seed(drop_key, cnt0), pair_drop_inc(drop_key, cnt0), drop_jump, drop_thr) ? drop_scale : 0.f,
                           pair_drop_keep_at(pair_drop_seed(drop_key, cnt1), pair_drop_inc(drop_key, cnt1), drop_jump, drop_thr) ? drop_scale : 0.f};
          dz = dz * kk;
          const f2 ym = y * kk;
          s0 = __builtin_elementwise_fma(g0, ym, s0); s1 = __builtin_elementwise_fma(g1, ym, s1); s2 = __builtin_elementwise_fma(g2, ym, s2);
        } else {
          s0 = __builtin_elementwise_fma(g0, y, s0);
          s1 = __builtin_elementwise_fma(g1, y, s1);
          s2 = __builtin_elementwise_fma(g2, y, s2);
        }
        sb = sb + dz;
        const float give = odd ? dz.x : dz.y;
        const float got = __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(give), 0xB1, 0xf, 0xf, true));  // quad_perm [1,0,3,2]
        const uint32_t packed = odd ? pack_bf16x2(got, dz.y) : pack_bf16x2(dz.x, got);
        if (full_tile || row0 + (lane & 1) < nrows)
          *reinterpret_cast<uint32_t*>(ocol + (int64_t)rowc * ncol) = packed;
      }
      float4 part = make_float4(s0.x + s0.y, s1.x + s1.y, s2.x + s2.y, sb.x + sb.y);
      part.x += __shfl_xor(part.x, 32); part.y += __shfl_xor(part.y, 32);
      part.z += __shfl_xor(part.z, 32); part.w += __shfl_xor(part.w, 32);
      if (lane < 32) sPart[(es & 1) * (DW_WAVES * 32) + wave * 32 + lane] = part;
    };

    f32x16_t z;
    for (int slab = 0; slab < nslab; ++slab) {
      wait_vm<0>();                                           // this wave's pieces of `slab` have landed (and its stores have retired) ...
      __builtin_amdgcn_s_barrier();                           // ... and everybody's; every wave is done with slab - 1's buffer
      __builtin_amdgcn_sched_barrier(0);
      if (slab > 1) flush(slab - 2);                          // its four partial rows were written before this barrier
      if (slab > 0 && (slab - 1) % spb == 0) head_begin((slab - 1) / spb);
      if (slab + 1 < nslab) dma(slab + 1, (slab + 1) & 1);
      if (slab > 0) epilogue(z, slab - 1);
      const char* wb = sW + (slab & 1) * SLAB_BYTES;
#pragma unroll
      for (int r = 0; r < 16; ++r) z[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) mma_step(xf[ks], load_frag_linear<T>(wb, ks, lane), z);
    }
    __syncthreads();
    if (nslab > 1) flush(nslab - 2);
    if ((nslab - 1) % spb == 0) head_begin((nslab - 1) / spb);
    epilogue(z, nslab - 1);
    __syncthreads();
    flush(nslab - 1);
  }
}

static size_t pair_dz_wide_lds_bytes(int D) {
  return 2 * (size_t)pair_wide_slab_bytes(D) + (size_t)D * 16 + (size_t)DW_WAVES * 32 * 16 * 3;
}

// (the packed image is the wide forward's: a width it refuses has none)
bool pair_dz_wide_supported(int dtype, int D, int num_heads) {
  return pair_wide_supported(dtype, D, num_heads) && pair_dz_wide_lds_bytes(D) <= 160 * 1024;
}

template <int KS>
static int launch_pair_dz_wide(const DzFusedParams& p, hipStream_t st) {
  const size_t sh = pair_dz_wide_lds_bytes(p.D);
  if (raise_dynamic_lds(pair_dz_wide_kernel<KS>, sh, "peneo_pair_dz_fused") != PENEO_OK) return PENEO_ERR_LAUNCH;
  const int64_t blocks = (p.npairs + DW_PAIRS - 1) / DW_PAIRS;
  hipLaunchKernelGGL((pair_dz_wide_kernel<KS>), dim3((unsigned)blocks), dim3(DW_WAVES * 64), sh, st, p);
  return check_launch("peneo_pair_dz_fused");
}

int pair_dz_wide(const DzFusedParams& p, hipStream_t st) {
  if (!pair_dz_wide_supported(PENEO_BF16, p.D, p.a.num_heads)) {
    set_error("peneo_pair_dz_fused: D=%d with %d heads not supported by the wide kernel", p.D, p.a.num_heads);
    return PENEO_ERR_INVALID;
  }
  switch (p.D / 16) {
    case 36: return launch_pair_dz_wide<36>(p, st);
    case 40: return launch_pair_dz_wide<40>(p, st);
    case 44: return launch_pair_dz_wide<44>(p, st);
    case 48: return launch_pair_dz_wide<48>(p, st);
    case 52: return launch_pair_dz_wide<52>(p, st);
    case 56: return launch_pair_dz_wide<56>(p, st);
    case 60: return launch_pair_dz_wide<60>(p, st);
    case 64: return launch_pair_dz_wide<64>(p, st);
    default: set_error("peneo_pair_dz_fused: D=%d not supported", p.D); return PENEO_ERR_INVALID;
  }
}

}  // namespace peneo
