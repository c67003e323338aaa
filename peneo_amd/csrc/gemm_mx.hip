// OCP-MX FP8 GEMM for gfx950: C[m, n] = epilogue( sum_k A^(m, k) B^(n, k) ), both operands k-major e4m3 bytes with one E8M0 scale per 32
// consecutive k (the format of peneo_mxfp8_quantize_rows), fp32 accumulation on v_mfma_scale_f32_32x32x64_f8f6f4.
//
// Tile: one 4-wave workgroup owns 128 tokens (m) x 128 outputs (n); the waves sit 2 x 2, each on 64 n x 64 m = 2 x 2 accumulators of
// 32 x 32.  The product is computed TRANSPOSED: the weight rows B are the MFMA's A operand and the tokens its B operand, so accumulator
// element r of lane l is C[m = l & 31][n = 8 (r >> 2) + 4 (l >> 5) + (r & 3)] (common.h acc_row): a lane holds 4 x 4 consecutive n of ONE
// token and lane l ^ 32 the other 16 of the same 32, which makes the epilogue's stores 8- or 16-byte vectors along a row of C and the
// amax of an MX output block one in-lane maximum plus one cross-half exchange.
//
// Staging: a K stage is 128 bytes of every row of both operand tiles (2 x 16 KiB), brought in by LDS-DMA (global_load_lds_dwordx4, 8
// pieces of 1 KiB per wave and stage) into a ring of 2 stages; a piece is 8 rows x 128 B, and the 16-byte slot s of row r lands at slot
// s ^ ((r >> 1) & 7) (the swizzle of gemm.hip, applied on the source address since the LDS image of a piece is lane-linear).  One barrier per
// stage: wait for the stage's pieces (vmcnt(0): nothing younger is in flight with a ring of 2), barrier, issue the next stage into the
// buffer every wave has just finished reading, compute.  64 KiB of LDS and at most 128 VGPRs: two workgroups per CU, so that one's
// epilogue and prologue run under the other's k loop (K = 768 is only 6 stages).
//
// Operand maps (pair_heads_mx.hip, measured): lane l of an e4m3 operand holds row l & 31; its 32 bytes are k = 16 (l >> 5) + 0..15 and
// 32 + 16 (l >> 5) + 0..15 of the 64-deep step: slots 4 ks + (l >> 5) and 4 ks + 2 + (l >> 5) of the 128-byte stage row.  The op_sel byte
// of lane r + 32 kb's scale VGPR scales row r, K block kb of the step.  The four scale bytes of a row and stage are one dword; they ride
// in the ring (one global_load_lds_dword per wave and stage: lanes 0..31 the wave's 32 weight rows, lanes 32..63 its 32 token rows), a
// lane reads its rows' dwords back and shifts them right by 8 (l >> 5); op_sel = 2 ks then selects block 2 ks + (l >> 5).
//
// Rows past M (N) are not read: their DMA source is clamped to the last row, and the accumulator columns (rows) they feed are not stored.
#include "common.h"
#include "gemm_common.h"
#include "mx_common.h"

namespace peneo {
namespace {

constexpr int MXG_TILE = 128;                   // tokens and outputs per workgroup
constexpr int MXG_BK = 128;                     // k (= bytes) per stage and row
constexpr int MXG_OPER = MXG_TILE * MXG_BK;     // one operand tile of a stage
constexpr int MXG_SCALES = 1024;                // scale dwords of a stage: [4 waves][W rows 32 wave + 0..31 | X rows 32 wave + 0..31]
constexpr int MXG_STAGE = 2 * MXG_OPER + MXG_SCALES;
constexpr int MXG_NSTAGE = 2;
constexpr int MXG_LDS = MXG_NSTAGE * MXG_STAGE;

struct MxGemmParams {
  const uint8_t* Aq; const uint8_t* As; const uint8_t* Bq; const uint8_t* Bs;
  void* C; int64_t ldc; int M, N, K, c_dtype;
  const float* bias; int act; const void* residual; int64_t ld_res; float alpha;
  uint8_t* Cq; uint8_t* Cs;
};

// 64 lanes x 4 B -> 256 B of LDS at the uniform base (lane-linear), the dword form of common.h lds_dma_1k
__device__ __forceinline__ void mxg_dma_dword(const char* gsrc_lane, uint32_t lds_base_uniform) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc_lane), "s"(lds_base_uniform) : "memory");
}
__device__ __forceinline__ int mxg_off(int row, int slot) { return row * MXG_BK + ((slot ^ ((row >> 1) & 7)) << 4); }

__device__ __forceinline__ i32x8_t mxg_frag(const char* tile, int row, int ks, int half) {
  const uint4 lo = *reinterpret_cast<const uint4*>(tile + mxg_off(row, 4 * ks + half));
  const uint4 hi = *reinterpret_cast<const uint4*>(tile + mxg_off(row, 4 * ks + 2 + half));
  return i32x8_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

template <int KS>
__device__ __forceinline__ void mxg_step(const char* sW, const char* sX, int wrow, int xrow, int half, const uint32_t (&ws)[2],
                                         const uint32_t (&xs)[2], f32x16_t (&acc)[4]) {
  const i32x8_t w0 = mxg_frag(sW, wrow, KS, half), w1 = mxg_frag(sW, wrow + 32, KS, half);
  const i32x8_t x0 = mxg_frag(sX, xrow, KS, half), x1 = mxg_frag(sX, xrow + 32, KS, half);
  acc[0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w0, x0, acc[0], 0, 0, 2 * KS, (int)ws[0], 2 * KS, (int)xs[0]);
  acc[1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w0, x1, acc[1], 0, 0, 2 * KS, (int)ws[0], 2 * KS, (int)xs[1]);
  acc[2] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w1, x0, acc[2], 0, 0, 2 * KS, (int)ws[1], 2 * KS, (int)xs[0]);
  acc[3] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w1, x1, acc[3], 0, 0, 2 * KS, (int)ws[1], 2 * KS, (int)xs[1]);
}

// 32 n x 32 m of C from one accumulator: this lane's token m, its 16 outputs nb + 8 g + 4 half + 0..3 (g = 0..3)
__device__ __forceinline__ void mxg_epilogue(const MxGemmParams& p, const f32x16_t& c, int nb, int m, int half) {
  const bool ok = m < p.M;
  const bool bf = p.c_dtype == PENEO_BF16;
  float v[16];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int n = nb + 8 * g + 4 * half;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias) b = *reinterpret_cast<const float4*>(p.bias + n);
    v[4 * g + 0] = c[4 * g + 0] * p.alpha + b.x;
    v[4 * g + 1] = c[4 * g + 1] * p.alpha + b.y;
    v[4 * g + 2] = c[4 * g + 2] * p.alpha + b.z;
    v[4 * g + 3] = c[4 * g + 3] * p.alpha + b.w;
  }
  if (p.act == PENEO_ACT_GELU) {   // as the bf16 GEMM: polynomial erf for bf16 tiles, erff for fp32
    if (bf) {
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = gelu_fast_f(v[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = gelu_f(v[i]);
    }
  }
  if (p.residual && ok) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t idx = (int64_t)m * p.ld_res + nb + 8 * g + 4 * half;
      if (bf) {
        const uint2 r = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(p.residual) + idx);
        v[4 * g + 0] += __uint_as_float(r.x << 16); v[4 * g + 1] += __uint_as_float(r.x & 0xffff0000u);
        v[4 * g + 2] += __uint_as_float(r.y << 16); v[4 * g + 3] += __uint_as_float(r.y & 0xffff0000u);
      } else {
        const float4 r = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.residual) + idx);
        v[4 * g + 0] += r.x; v[4 * g + 1] += r.y; v[4 * g + 2] += r.z; v[4 * g + 3] += r.w;
      }
    }
  }
  if (p.C && ok) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t idx = (int64_t)m * p.ldc + nb + 8 * g + 4 * half;
      if (bf)
        *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(p.C) + idx) = make_uint2(pack_bf16x2(v[4 * g], v[4 * g + 1]), pack_bf16x2(v[4 * g + 2], v[4 * g + 3]));
      else
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.C) + idx) = make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
    }
  }
  if (p.Cq) {   // uniform: the MX copy of the value as rounded to bf16 (== peneo_mxfp8_quantize_rows_bf16 of a bf16 C)
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { v[i] = Elem<bf16_t>::round(v[i]); amax = fmaxf(amax, fabsf(v[i])); }
    amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
    const uint32_t sb = mx_scale_byte(amax);
    const float inv = mx_inv_scale(sb);
    if (ok) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<uint32_t*>(p.Cq + (int64_t)m * p.N + nb + 8 * g + 4 * half) =
            mx_e4m3x4(v[4 * g] * inv, v[4 * g + 1] * inv, v[4 * g + 2] * inv, v[4 * g + 3] * inv);
      if (half == 0) p.Cs[(int64_t)m * (p.N >> 5) + (nb >> 5)] = (uint8_t)sb;
    }
  }
}

__global__ __launch_bounds__(256, 2) void gemm_mx_kernel(MxGemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, r31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave & 1, wm = wave >> 1;
  // Tile order: workgroups go to the 8 XCDs round-robin, so workgroup id -> (XCD id % 8, position id / 8) -> a contiguous range of
  // tiles per XCD (bijective for any count), tiles in m-major order with n fastest: the workgroups resident on one XCD share a few
  // token tiles and the whole weight matrix, which its 4 MiB L2 then holds
  const int total = gridDim.x, tn = (p.N + MXG_TILE - 1) / MXG_TILE;
  const int xq = total >> 3, xr = total & 7, xcd = blockIdx.x & 7;
  const int tile = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (blockIdx.x >> 3);
  const int n0 = (tile % tn) * MXG_TILE, m0 = (tile / tn) * MXG_TILE;
  const int K = p.K, KT = K / MXG_BK;

  // DMA: this wave brings rows 32 wave .. 32 wave + 31 of both tiles, piece u = rows 32 wave + 8 u + (lane >> 3), LDS slot lane & 7
  const char* srcW[4];
  const char* srcX[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = 32 * wave + 8 * u + (lane >> 3);
    const int slot = (lane & 7) ^ ((row >> 1) & 7);
    srcW[u] = reinterpret_cast<const char*>(p.Bq) + (int64_t)min(n0 + row, p.N - 1) * K + slot * 16;
    srcX[u] = reinterpret_cast<const char*>(p.Aq) + (int64_t)min(m0 + row, p.M - 1) * K + slot * 16;
  }
  const uint32_t dst0 = lds_addr(smem) + wave * 4096;
  // scale dwords: this lane fetches the one of row 32 wave + r31 of the weight tile (lanes 0..31) or the token tile (32..63)
  const char* srcS = half == 0 ? reinterpret_cast<const char*>(p.Bs) + (int64_t)min(n0 + 32 * wave + r31, p.N - 1) * (K >> 5)
                               : reinterpret_cast<const char*>(p.As) + (int64_t)min(m0 + 32 * wave + r31, p.M - 1) * (K >> 5);
  const uint32_t dstS = lds_addr(smem) + 2 * MXG_OPER + wave * 256;
  const int wrow = wn * 64 + r31, xrow = wm * 64 + r31;
  const int wsoff = 2 * MXG_OPER + wn * 512 + r31 * 4, xsoff = 2 * MXG_OPER + wm * 512 + 128 + r31 * 4;   // + 256 for rows + 32

  f32x16_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

#pragma unroll
  for (int u = 0; u < 4; ++u) lds_dma_1k<0>(srcW[u], dst0 + u * 1024);
#pragma unroll
  for (int u = 0; u < 4; ++u) lds_dma_1k<0>(srcX[u], dst0 + MXG_OPER + u * 1024);
  mxg_dma_dword(srcS, dstS);

  for (int kt = 0; kt < KT; ++kt) {
    wait_vm<0>();                       // this stage's pieces
    __builtin_amdgcn_s_barrier();       // ... of every wave; and every wave is done reading the other buffer
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < KT) {
      const uint32_t so = ((kt + 1) & 1) * MXG_STAGE;
      const int64_t ko = (int64_t)(kt + 1) * MXG_BK;
#pragma unroll
      for (int u = 0; u < 4; ++u) lds_dma_1k<0>(srcW[u] + ko, dst0 + so + u * 1024);
#pragma unroll
      for (int u = 0; u < 4; ++u) lds_dma_1k<0>(srcX[u] + ko, dst0 + so + MXG_OPER + u * 1024);
      mxg_dma_dword(srcS + 4 * (kt + 1), dstS + so);
    }
    __builtin_amdgcn_sched_barrier(0);
    const char* sW = smem + (kt & 1) * MXG_STAGE;
    const char* sX = sW + MXG_OPER;
    const uint32_t ws[2] = {*reinterpret_cast<const uint32_t*>(sW + wsoff) >> (8 * half), *reinterpret_cast<const uint32_t*>(sW + wsoff + 256) >> (8 * half)};
    const uint32_t xs[2] = {*reinterpret_cast<const uint32_t*>(sW + xsoff) >> (8 * half), *reinterpret_cast<const uint32_t*>(sW + xsoff + 256) >> (8 * half)};
    mxg_step<0>(sW, sX, wrow, xrow, half, ws, xs, acc);
    mxg_step<1>(sW, sX, wrow, xrow, half, ws, xs, acc);
  }

  // rolled over the four accumulators (the tile in hand is always acc[0]; the others move up): one copy of the epilogue's code
#pragma unroll 1
  for (int t = 0; t < 4; ++t) {
    const int nb = n0 + wn * 64 + 32 * (t >> 1);
    if (nb < p.N) mxg_epilogue(p, acc[0], nb, m0 + wm * 64 + 32 * (t & 1) + r31, half);
    acc[0] = acc[1]; acc[1] = acc[2]; acc[2] = acc[3];
  }
}

bool mxg_bad_ep(const peneo_gemm_epilogue* e) {
  return e && (e->preact || e->grad_src || e->drop_p > 0.f || e->accumulate || e->pair_dz || e->pair_dz_ws || e->a_colsum ||
               (e->act != PENEO_ACT_NONE && e->act != PENEO_ACT_GELU));
}
bool aligned(const void* ptr, uintptr_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0; }

}  // namespace
}  // namespace peneo

using namespace peneo;

extern "C" int peneo_gemm_mxfp8_supported(int M, int N, int K) {
  if (M < 1 || N < 32 || K < MXG_BK || N % 32 != 0 || K % MXG_BK != 0) return 0;
  if ((int64_t)((M + MXG_TILE - 1) / MXG_TILE) * ((N + MXG_TILE - 1) / MXG_TILE) > 0x7fffffff) return 0;   // tiles = grid.x
  return 1;
}

extern "C" int peneo_gemm_mxfp8(int M, int N, int K, const void* A_q, const void* A_s, const void* B_q, const void* B_s, void* C,
                                int64_t ldc, int c_dtype, const peneo_gemm_epilogue* ep, void* C_q, void* C_s, peneo_stream_t stream) {
  PENEO_REQUIRE(peneo_gemm_mxfp8_supported(M, N, K), "peneo_gemm_mxfp8: shape M=%d N=%d K=%d not supported (peneo_gemm_mxfp8_supported)", M, N, K);
  PENEO_REQUIRE(A_q && A_s && B_q && B_s, "peneo_gemm_mxfp8: null operand");
  PENEO_REQUIRE(c_dtype == PENEO_BF16 || c_dtype == PENEO_F32, "peneo_gemm_mxfp8: c_dtype must be PENEO_BF16 or PENEO_F32");
  PENEO_REQUIRE(C || C_q, "peneo_gemm_mxfp8: no output (C and C_q both NULL)");
  PENEO_REQUIRE((C_q == nullptr) == (C_s == nullptr), "peneo_gemm_mxfp8: C_q and C_s go together");
  PENEO_REQUIRE(!mxg_bad_ep(ep), "peneo_gemm_mxfp8: the epilogue takes bias, act (none / GELU), residual and alpha only");
  PENEO_REQUIRE(aligned(A_q, 16) && aligned(B_q, 16) && aligned(A_s, 4) && aligned(B_s, 4),
                "peneo_gemm_mxfp8: A_q / B_q must be 16-byte aligned, A_s / B_s 4-byte aligned");
  PENEO_REQUIRE(!C || (aligned(C, 16) && ldc >= N && ldc % 4 == 0), "peneo_gemm_mxfp8: C must be 16-byte aligned with ldc >= N, ldc %% 4 == 0");
  PENEO_REQUIRE(!C_q || aligned(C_q, 4), "peneo_gemm_mxfp8: C_q must be 4-byte aligned");
  MxGemmParams p = {};
  p.Aq = static_cast<const uint8_t*>(A_q); p.As = static_cast<const uint8_t*>(A_s);
  p.Bq = static_cast<const uint8_t*>(B_q); p.Bs = static_cast<const uint8_t*>(B_s);
  p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K; p.c_dtype = c_dtype;
  p.alpha = 1.f;
  if (ep) {
    PENEO_REQUIRE(!ep->bias || aligned(ep->bias, 16), "peneo_gemm_mxfp8: bias must be 16-byte aligned");
    PENEO_REQUIRE(!ep->residual || (aligned(ep->residual, 16) && ep->ld_res >= N && ep->ld_res % 4 == 0),
                  "peneo_gemm_mxfp8: residual must be 16-byte aligned with ld_res >= N, ld_res %% 4 == 0");
    p.bias = ep->bias; p.act = ep->act; p.residual = ep->residual; p.ld_res = ep->ld_res;
    p.alpha = ep->alpha == 0.f ? 1.f : ep->alpha;
  }
  p.Cq = static_cast<uint8_t*>(C_q); p.Cs = static_cast<uint8_t*>(C_s);
  static std::atomic<uint64_t> devices{0};
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(gemm_mx_kernel), MXG_LDS, devices))
    return dynamic_lds_error("peneo_gemm_mxfp8", MXG_LDS);
  const dim3 grid((unsigned)(((N + MXG_TILE - 1) / MXG_TILE) * ((M + MXG_TILE - 1) / MXG_TILE)));
  hipLaunchKernelGGL(gemm_mx_kernel, grid, dim3(256), MXG_LDS, (hipStream_t)stream, p);
  return check_launch("peneo_gemm_mxfp8");
}
