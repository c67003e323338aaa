// bf16 GEMM with ONE 8-wave workgroup per CU and workgroup tiles of 256 x 256 / 384 x 192 / 256 x 128 (gfx950).
//
// Why: the 128 x 128 kernel of gemm.hip moves 32 KiB global -> LDS per 2 MFLOP; a CU turns LDS-DMA requests into LDS lines
// at ~20-26 B/clk, so that kernel is fill-bound at ~40 % of the matrix cores, and at M = 5672 its 270 / 810 /
// 1080 tiles quantise badly on 512 resident workgroups.  A 256 x 256 tile moves 64 KiB per 8.4 MFLOP (half the bytes per
// FLOP), wave tiles of 128 x 64 (4 x 2 MFMA 32 x 32 accumulators) read 0.75 KiB of LDS per MFMA instead of 1, and the tile
// shape is chosen per problem so that the tiles fill ONE round of the 256 CUs (M = 5672: 207 tiles of 256 x 256 for
// N = 2304, 240 tiles of 384 x 192 for N = 3072, 138 tiles of 256 x 128 for N = 768).
//
// Layouts: A k-major [M][K]; B k-major [N][K] (forward, x W^T) or mn-major [K][N] (dgrad, dy W).  K % 64 == 0.
// Both mn-major (A [K][M], B [K][N]: a weight gradient dy^T x) on the 384 x 192 tile, with split-k: launch_gemm_big_nn below;
// that form alone takes K % 8 == 0 (a ragged last k-tile, see "tail" in the body) and has a grouped launch (launch_gemm_big_group).
// LDS image of a k-major tile: rows of 128 B (64 k), 16-byte slot s of row r at slot s ^ ((r >> 1) & 7) (swizzle applied
// to the SOURCE address of each LDS-DMA lane, destination lane-linear: 1 KiB piece = 8 rows); fragments by ds_read_b128.
// mn-major tile: 1 KiB pieces of [8 k][64 columns], the two 64-byte halves of a line swapped when (k >> 1) & 1; fragments
// by ds_read_b64_tr_b16.  (Both are the images of gemm.hip's LDS-DMA kernels.)
// Pipeline: ring of NSTAGE k-tiles, LDS-DMA NSTAGE - 1 tiles ahead from inline asm (counted vmcnt, invisible to hipcc so
// that it does not drain the ring in front of every ds_read), one s_barrier per k-tile.
// Epilogue: each wave parks one 32-row block of its accumulators in its own LDS patch, reads it back row-major and runs
// the shared fused epilogue (gemm_common.h) on 8 consecutive columns per lane: 16-byte stores, whole 128-byte lines.
#include <cstdlib>
#include <type_traits>
#include "common.h"
#include "gemm_common.h"
#include "gemm_walk.h"

namespace peneo {

typedef short bg_s16x4 __attribute__((ext_vector_type(4)));

template <bool BK_, int WGM_, int WGN_, int FM_, int FN_, int NSTAGE_, bool AK_ = true>
struct BigCfg {
  static constexpr bool AK = AK_, BK = BK_;
  static constexpr int WGM = WGM_, WGN = WGN_, FM = FM_, FN = FN_, NSTAGE = NSTAGE_;
  static constexpr int BM = WGM * FM * 32, BN = WGN * FN * 32;
  static constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
  static constexpr int APW = BM / 64, BPW = BN / 64, PPW = APW + BPW;   // 1 KiB pieces per wave and k-tile
  static constexpr int LDS_BYTES = NSTAGE * STAGE;
  static constexpr int EP_LD = FN * 32 + 4;                               // floats per row of a wave's epilogue patch
  static_assert(WGM * WGN == 8, "eight waves");
  static_assert(BM % 64 == 0 && BN % 64 == 0, "pieces of 8 rows are dealt to 8 waves");
  static_assert(8 * 32 * EP_LD * 4 <= LDS_BYTES, "epilogue patches fit in the dead ring");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

// One problem of a grouped launch (launch_gemm_big_group): what the body reads of a problem, and nothing of the fused epilogue
struct BigGroupProblem {
  const void* A; const void* B; void* C;
  int64_t lda, ldb, ldc;
  int M, N, K, accumulate;
};
struct BigGroup {
  BigGroupProblem q[GEMM_GROUP_MAX];
  int first_tile[GEMM_GROUP_MAX + 1];
  int tiles_n[GEMM_GROUP_MAX];
  int n;
};

// How a workgroup leaves its tile:
//   EP_FUSED  the shared fused epilogue of peneo_gemm (gemm_common.h)
//   EP_PART   plain fp32 in slice zsplit of p.ws: the launch is tiles x split_k workgroups, workgroup (tile, z) multiplies k-tiles
//             [z kt_per_split, (z + 1) kt_per_split) and peneo_gemm's split-k reduce runs the caller's epilogue
//   EP_GROUP  fp32 C (+= with `accumulate`), the only epilogue a grouped problem on this tile may ask for
// Each is its own instantiation: the fused epilogue is part of the first one's code only.
enum { EP_FUSED = 0, EP_PART = 1, EP_GROUP = 2 };

// The workgroup's tile (m0, n0) over k-tiles [kt0, kt0 + ktiles) of 64, all of them full, and then, where tail_pieces > 0, the
// ragged last k-tile of 8 * tail_pieces rows (mn-major operands only; the caller passes 0 everywhere else).
template <typename C, int EPI, typename P>
__device__ __forceinline__ void gemm_big_body(const P& p, char* smem, const int m0, const int n0, const int zsplit, const int kt0,
                                              const int ktiles, const int tail_pieces) {
  constexpr int FM = C::FM, FN = C::FN, NSTAGE = C::NSTAGE;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / C::WGN, wn = wave % C::WGN;

  const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A);
  const bf16_t* B = reinterpret_cast<const bf16_t*>(p.B);

  // ---- LDS-DMA sources of this wave's pieces (piece g = wave + 8 u of the A tile / of the B tile): per-lane 32-bit byte
  //      offsets inside the tile (constant over k) + one uniform 64-bit base per operand that walks k with scalar adds ----
  uint32_t offA[C::APW], offB[C::BPW];
#pragma unroll
  for (int u = 0; u < C::APW; ++u) {
    const int g = wave + 8 * u;
    if constexpr (C::AK) {
      const int row = g * 8 + (lane >> 3);
      const int sg = (lane & 7) ^ ((row >> 1) & 7);
      offA[u] = (uint32_t)(((int64_t)(min(m0 + row, p.M - 1) - m0) * p.lda + sg * 8) * 2);
    } else {
      constexpr int MQ = C::BM / 64;
      const int kb = g / MQ, mq = g % MQ, kr = lane >> 3;
      const int cg = (lane & 7) ^ (((kr >> 1) & 1) << 2);
      offA[u] = (uint32_t)(((int64_t)(kb * 8 + kr) * p.lda + (min(m0 + mq * 64 + cg * 8, p.M - 8) - m0)) * 2);
    }
  }
#pragma unroll
  for (int u = 0; u < C::BPW; ++u) {
    const int g = wave + 8 * u;
    if constexpr (C::BK) {
      const int row = g * 8 + (lane >> 3);
      const int sg = (lane & 7) ^ ((row >> 1) & 7);
      offB[u] = (uint32_t)(((int64_t)(min(n0 + row, p.N - 1) - n0) * p.ldb + sg * 8) * 2);
    } else {
      constexpr int NQ = C::BN / 64;
      const int kb = g / NQ, nq = g % NQ, kr = lane >> 3;
      const int cg = (lane & 7) ^ (((kr >> 1) & 1) << 2);
      offB[u] = (uint32_t)(((int64_t)(kb * 8 + kr) * p.ldb + (min(n0 + nq * 64 + cg * 8, p.N - 8) - n0)) * 2);
    }
  }
  auto uniform_ptr = [](const void* q) -> const char* {
    const uint64_t v = reinterpret_cast<uint64_t>(q);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<const char*>(((uint64_t)hi << 32) | lo);
  };
  const int64_t stepA = C::AK ? 128 : (int64_t)64 * p.lda * 2;
  const int64_t stepB = C::BK ? 128 : (int64_t)64 * p.ldb * 2;
  const char* bA = uniform_ptr(reinterpret_cast<const char*>(C::AK ? A + (int64_t)m0 * p.lda : A + m0) + kt0 * stepA);
  const char* bB = uniform_ptr(reinterpret_cast<const char*>(C::BK ? B + (int64_t)n0 * p.ldb : B + n0) + kt0 * stepB);
  const uint32_t lds0 = lds_addr(smem);
  // The pieces of a k-tile are issued in four groups, one between the MFMA clusters of each k-step: a wave that issues
  // all of its pieces back to back stalls on the memory pipeline (measured: fill and compute then run one after the other,
  // 2.1 us per 256 x 256 k-tile instead of ~1)
  uint32_t dbase = 0;
  auto issue_group = [&](auto gc) {
    constexpr int G = decltype(gc)::value;
#pragma unroll
    for (int u = 0; u < C::PPW; ++u) {
      if (u * 4 / C::PPW != G) continue;
      if (u < C::APW) lds_dma_1k_s<0>(offA[u], bA, dbase + u * 8192);
      else lds_dma_1k_s<0>(offB[u - C::APW], bB, dbase + C::A_BYTES + (u - C::APW) * 8192);
    }
    if constexpr (G == 3) { bA += stepA; bB += stepB; }      // the k-tile is complete: the bases move on
  };
  auto issue = [&](int stage) {
    dbase = __builtin_amdgcn_readfirstlane(lds0 + stage * C::STAGE + wave * 1024);
    issue_group(std::integral_constant<int, 0>{}); issue_group(std::integral_constant<int, 1>{});
    issue_group(std::integral_constant<int, 2>{}); issue_group(std::integral_constant<int, 3>{});
  };

  // ---- fragment offsets inside a stage ----
  int aoff[C::AK ? 4 : FM], boff[C::BK ? 4 : FN];
  if constexpr (C::AK) {
    const int row = wm * FM * 32 + (lane & 31), swz = (row >> 1) & 7;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) aoff[ks] = row * 128 + (((2 * ks + half) ^ swz) << 4);
  } else {
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int m = wm * FM * 32 + i * 32 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
      aoff[i] = (half * (C::BM / 64) + (m >> 6)) * 1024 + ((lane & 15) >> 2) * 128 + (((m & 63) * 2) ^ (((lane >> 3) & 1) << 6));
    }
  }
  if constexpr (C::BK) {
    const int row = wn * FN * 32 + (lane & 31), swz = (row >> 1) & 7;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) boff[ks] = C::A_BYTES + row * 128 + (((2 * ks + half) ^ swz) << 4);
  } else {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = wn * FN * 32 + j * 32 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
      boff[j] = C::A_BYTES + (half * (C::BN / 64) + (n >> 6)) * 1024 + ((lane & 15) >> 2) * 128 +
                (((n & 63) * 2) ^ (((lane >> 3) & 1) << 6));
    }
  }

  f32x16_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto load_a = [&](const char* st, int ks, uint4 (&fa)[FM]) {
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      if constexpr (C::AK) {
        fa[i] = *reinterpret_cast<const uint4*>(st + aoff[ks] + i * 4096);
      } else {
        typedef __attribute__((address_space(3))) bg_s16x4* lds_s4p;
        const char* q = st + aoff[i] + ks * (2 * (C::BM / 64) * 1024);
        const bg_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4p)(q));
        const bg_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4p)(q + 512));
        const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
        fa[i] = make_uint4(l2.x, l2.y, h2.x, h2.y);
      }
    }
  };
  auto load_b = [&](const char* st, int ks, uint4 (&fb)[FN]) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      if constexpr (C::BK) {
        fb[j] = *reinterpret_cast<const uint4*>(st + boff[ks] + j * 4096);
      } else {
        typedef __attribute__((address_space(3))) bg_s16x4* lds_s4p;
        const char* q = st + boff[j] + ks * (2 * (C::BN / 64) * 1024);
        const bg_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4p)(q));
        const bg_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4p)(q + 512));
        const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
        fb[j] = make_uint4(l2.x, l2.y, h2.x, h2.y);
      }
    }
  };
  auto mma = [&](const uint4 (&fa)[FM], const uint4 (&fb)[FN]) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, fa[i]), __builtin_bit_cast(bf16x8_t, fb[j]),
                                                            acc[i][j], 0, 0, 0);
  };

  // ---- ring: tiles t .. t + NSTAGE - 2 in flight while tile t is multiplied ----
#pragma unroll
  for (int s = 0; s < NSTAGE - 1; ++s)
    if (s < ktiles) issue(s);
  for (int t = 0; t < ktiles; ++t) {
    // this wave's pieces of tile t have landed (younger tiles may still be in flight) ...
    if (NSTAGE > 2 && t + NSTAGE - 2 < ktiles) wait_vm<(NSTAGE - 2) * C::PPW>(); else wait_vm<0>();
    // ... and everybody's: the barrier also says that every wave is done reading tile t - 1, whose stage is refilled now
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    const bool more = t + NSTAGE - 1 < ktiles;
    dbase = __builtin_amdgcn_readfirstlane(lds0 + ((t + NSTAGE - 1) % NSTAGE) * C::STAGE + wave * 1024);
    const char* st = smem + (t % NSTAGE) * C::STAGE;
    uint4 fa0[FM], fb0[FN], fa1[FM], fb1[FN];
    load_a(st, 0, fa0); load_b(st, 0, fb0);
    if (more) issue_group(std::integral_constant<int, 0>{});
    load_a(st, 1, fa1); load_b(st, 1, fb1);
    __builtin_amdgcn_sched_barrier(0);
    mma(fa0, fb0);
    __builtin_amdgcn_sched_barrier(0);
    if (more) issue_group(std::integral_constant<int, 1>{});
    load_a(st, 2, fa0); load_b(st, 2, fb0);
    __builtin_amdgcn_sched_barrier(0);
    mma(fa1, fb1);
    __builtin_amdgcn_sched_barrier(0);
    if (more) issue_group(std::integral_constant<int, 2>{});
    load_a(st, 3, fa1); load_b(st, 3, fb1);
    __builtin_amdgcn_sched_barrier(0);
    mma(fa0, fb0);
    __builtin_amdgcn_sched_barrier(0);
    if (more) issue_group(std::integral_constant<int, 3>{});
    mma(fa1, fb1);
  }
  // ---- tail (A [K][M], B [K][N], K % 64 != 0): the last k-tile has tail_pieces < 8 row blocks of 8 k.  Decided once per
  //      workgroup, behind the loop over full tiles, whose code it does not touch.  A piece whose row block lies at or beyond K
  //      is NOT requested (no address of such a row is formed, clamped or not): its 1 KiB of LDS is zeroed with ds stores
  //      instead, and all four k-steps run, as the 128 x 128 kernel runs them over its zero lines (the same sums in the same order).
  //      Which wait proves what:
  //        barrier 1    every wave has read its last fragments of the full tiles: stage 0 may be overwritten;
  //        vmcnt(0)     this wave's requested pieces have landed.  The count needs no PPW bookkeeping: the loop's last iteration
  //                     waited for vmcnt(0) and issued nothing (`more` is false there; the two-stage ring waits for 0 in every
  //                     iteration), so the tail's own requests are the only ones outstanding, however many this wave has;
  //        barrier 2    __syncthreads waits for this wave's ds stores (lgkmcnt) and then for every wave: all pieces and all
  //                     zeros of the stage are visible before the first fragment read. ----
  if constexpr (!C::AK && !C::BK) {
    static_assert(C::AK || C::BK || NSTAGE == 2, "the tail's vmcnt(0) argument above is the two-stage ring's");
    if (tail_pieces > 0) {
      __syncthreads();
      dbase = __builtin_amdgcn_readfirstlane(lds0 + wave * 1024);
      const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int u = 0; u < C::APW; ++u) {
        if (walk_piece_in_tail(wave + 8 * u, C::BM / 64, tail_pieces)) lds_dma_1k_s<0>(offA[u], bA, dbase + u * 8192);
        else *reinterpret_cast<uint4*>(smem + (wave + 8 * u) * 1024 + lane * 16) = zero4;
      }
#pragma unroll
      for (int u = 0; u < C::BPW; ++u) {
        if (walk_piece_in_tail(wave + 8 * u, C::BN / 64, tail_pieces)) lds_dma_1k_s<0>(offB[u], bB, dbase + C::A_BYTES + u * 8192);
        else *reinterpret_cast<uint4*>(smem + C::A_BYTES + (wave + 8 * u) * 1024 + lane * 16) = zero4;
      }
      wait_vm<0>();
      __syncthreads();
#pragma unroll      // (unrolled on purpose: as a rolled loop the k-step's fragment addresses took 238 VGPRs, 7 more)
      for (int ks = 0; ks < 4; ++ks) {
        uint4 fa[FM], fb[FN];
        load_a(smem, ks, fa); load_b(smem, ks, fb);
        mma(fa, fb);
      }
    }
  }
  __syncthreads();     // the ring is dead: every wave has read its last fragments

  // ---- epilogue: 32-row blocks through a wave-private LDS patch ----
  float* patch = reinterpret_cast<float*>(smem) + wave * (32 * C::EP_LD);
  constexpr int CG = FN * 32 / 8;           // 8-column groups per row
  constexpr int RPP = 64 / CG;              // rows per pass (FN = 3: 5 rows, four lanes idle)
  constexpr int NPASS = (32 + RPP - 1) / RPP;
  const int cgi = lane % CG, rli = lane / CG;
  auto block = [&](auto ic) {
    constexpr int i = decltype(ic)::value;     // compile-time row block: a rolled loop would index acc[] dynamically (scratch)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) patch[acc_row(r, lane) * C::EP_LD + j * 32 + acc_col(lane)] = acc[i][j][r];
    __builtin_amdgcn_wave_barrier();
    const int mb = m0 + (wm * FM + i) * 32, nb = n0 + wn * FN * 32 + cgi * 8;
#pragma unroll 1
    for (int pass = 0; pass < NPASS; ++pass) {
      const int rl = pass * RPP + rli;
      if (rli < RPP && rl < 32 && mb + rl < p.M && nb + 8 <= p.N) {
        float v[8];
        const float4 x0 = *reinterpret_cast<const float4*>(patch + rl * C::EP_LD + cgi * 8);
        const float4 x1 = *reinterpret_cast<const float4*>(patch + rl * C::EP_LD + cgi * 8 + 4);
        v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w; v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
        if constexpr (EPI == EP_PART) {
          float4* q = reinterpret_cast<float4*>(p.ws + ((int64_t)zsplit * p.M + (mb + rl)) * p.N + nb);
          q[0] = x0; q[1] = x1;
        } else if constexpr (EPI == EP_GROUP) {
          float4* q = reinterpret_cast<float4*>(reinterpret_cast<float*>(p.C) + (int64_t)(mb + rl) * p.ldc + nb);
          if (p.accumulate) {
            const float4 c0 = q[0], c1 = q[1];
            v[0] += c0.x; v[1] += c0.y; v[2] += c0.z; v[3] += c0.w; v[4] += c1.x; v[5] += c1.y; v[6] += c1.z; v[7] += c1.w;
          }
          q[0] = make_float4(v[0], v[1], v[2], v[3]); q[1] = make_float4(v[4], v[5], v[6], v[7]);
        } else {
          epilogue_store8(p, mb + rl, nb, v);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  };
  block(std::integral_constant<int, 0>{});
  if constexpr (FM > 1) block(std::integral_constant<int, 1>{});
  if constexpr (FM > 2) block(std::integral_constant<int, 2>{});
  if constexpr (FM > 3) block(std::integral_constant<int, 3>{});
  static_assert(FM <= 4, "row blocks");
}

template <typename C, bool PART = false>
__global__ __launch_bounds__(512) void gemm_big_kernel(GemmParams p, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // XCD-aware tile order: workgroup ids go round-robin to the 8 XCDs; every XCD gets a contiguous band of tiles, n fastest
  const int total = gridDim.x, lin = blockIdx.x;
  const int q8 = total >> 3, r8 = total & 7, xcd = lin & 7, slot = lin >> 3;
  int tile = xcd * q8 + min(xcd, r8) + slot;
  // (PART: the order above runs over the whole launch, slice-major: the tiles of one k-range are neighbours on an XCD)
  // k-tiles: `ktiles` full ones, then the tail where the operands allow one (both mn-major) and this workgroup's range ends at K
  constexpr bool TAIL = !C::AK && !C::BK;
  const int kfull = p.K / 64;
  int zsplit = 0, kt0 = 0, ktiles = kfull, tail = TAIL ? walk_tail_pieces(p.K) : 0;
  if constexpr (PART) {
    const int tiles = total / p.split_k;
    zsplit = tile / tiles;
    tile -= zsplit * tiles;
    kt0 = zsplit * p.kt_per_split;
    const int kend = kt0 + p.kt_per_split;      // the host's ranges count the tail as a k-tile: (K + 63) / 64
    ktiles = min(kfull, kend) - kt0;
    if (TAIL && kend <= kfull) tail = 0;
  }
  const int m0 = (tile / tiles_n) * C::BM, n0 = (tile % tiles_n) * C::BN;
  gemm_big_body<C, PART ? EP_PART : EP_FUSED>(p, smem, m0, n0, zsplit, kt0, ktiles, tail);
}

// Grouped form on the (mn, mn) 384 x 192 tile: the tiles of up to GEMM_GROUP_MAX problems numbered consecutively (the tiles of one
// problem contiguous, n fastest: the tiles that share an A = dy panel are neighbours), the XCD-aware order over the whole launch,
// every workgroup the whole K of its tile: no split, no workspace, no atomics, the same bits on every run.
template <typename C>
__global__ __launch_bounds__(512) void gemm_big_group_kernel(BigGroup g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const WalkTile w = walk_group_tile(walk_xcd_tile(blockIdx.x, gridDim.x), g.first_tile, g.tiles_n, g.n, C::BM, C::BN);
  const BigGroupProblem& q = g.q[w.problem];
  gemm_big_body<C, EP_GROUP>(q, smem, w.m0, w.n0, 0, 0, q.K / 64, walk_tail_pieces(q.K));
}

template <typename C, bool PART = false>
static int launch_big(const GemmParams& p, hipStream_t st) {
  const int tm = (p.M + C::BM - 1) / C::BM, tn = (p.N + C::BN - 1) / C::BN;
  static std::atomic<uint64_t> lds_devices{0};
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(gemm_big_kernel<C, PART>), C::LDS_BYTES, lds_devices))
    return dynamic_lds_error("peneo_gemm", C::LDS_BYTES);
  const int wgs = tm * tn * (PART ? p.split_k : 1);
  hipLaunchKernelGGL((gemm_big_kernel<C, PART>), dim3((unsigned)wgs), dim3(512), C::LDS_BYTES, st, p, tn);
  const int rc = check_launch("peneo_gemm (big tiles)");
  return rc == PENEO_OK ? 1 : rc;
}

// Tile shapes: (workgroup tile, wave grid, wave tile, stages)
//   256 x 256: 2 x 4 waves of 128 x 64, 2 stages of 64 KiB
//   384 x 192: 4 x 2 waves of  96 x 96, 2 stages of 72 KiB
//   256 x 128: 4 x 2 waves of  64 x 64, 3 stages of 48 KiB
template <bool BK> using Big256 = BigCfg<BK, 2, 4, 4, 2, 2>;
template <bool BK> using Big384 = BigCfg<BK, 4, 2, 3, 3, 2>;
template <bool BK> using Big128 = BigCfg<BK, 4, 2, 2, 2, 3>;

// Cost model in cycles per k-tile of 64, calibrated on 4096^3 and the encoder shapes (tools/run_gemm_big.py): every kernel
// is bound by the CU's global -> LDS fill rate, so a round of tiles costs (bytes per k-tile) / (fill rate of that ring):
//   128 x 128, 2 workgroups per CU (gemm.hip)   3300 per round of 512 tiles (fractional rounds: the tails overlap)
//   256 x 256, 2 stages                         5080 per round of 256
//   384 x 192, 2 stages                         5550
//   256 x 128, 3 stages                         2760
static double big_cost(int M, int N, int bm, int bn, double per_round) {
  const int tiles = ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  return ((tiles + 255) / 256) * per_round;
}
static double small_cost(int M, int N) {
  const double r = ((M + 127) / 128) * (double)((N + 127) / 128) / 512.0;
  return (r > 1.0 ? r : 1.0) * 3300.0;
}

static int g_big_mode = -1;   // PENEO_GEMM_BIG: 0 = off, 1 = auto (default), 256 / 384 / 128 = force that tile where it applies
static int big_mode() {       // (read on first use, unless peneo_gemm_set_big_mode came first)
  if (g_big_mode < 0) { const char* e = getenv("PENEO_GEMM_BIG"); g_big_mode = e ? atoi(e) : 1; }
  return g_big_mode;
}

int launch_gemm_big(const GemmParams& p, bool b_kmajor, hipStream_t st) {
  const int mode = big_mode();
  if (mode == 0) return 0;
  // mn-major B = the dgrad GEMMs of the backward: in the step they run beside the weight-gradient stream, and a workgroup that
  // needs a CU's whole LDS cannot share it (measured: d_zi on 384 x 192 tiles 50 us alone, 166 us in the step; the step is
  // 0.2 ms FASTER with the 128 x 128 kernel there).  A forced tile (tools) still runs them.
  // (Those are SHORT launches that wait for empty CUs each time.  The one LONG launch of the step, the pair heads' dW1 on the side
  // stream, does run on whole-LDS workgroups: launch_gemm_big_nn.)
  if (!b_kmajor && mode == 1) return 0;
  if (p.split_k > 1 || p.dz_on || p.K % 64 != 0 || p.K < 128 || p.N % 8 != 0) return 0;
  if ((reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.B)) & 15) return 0;
  if ((p.lda * 2) % 16 != 0 || (p.ldb * 2) % 16 != 0) return 0;
  {
    const peneo_gemm_epilogue& e = p.ep;
    const int csz = p.c_dtype == PENEO_F32 ? 4 : 2;
    auto al = [](const void* ptr, int64_t ld, int esz) {
      return ptr == nullptr || (((reinterpret_cast<uintptr_t>(ptr) & 15) == 0) && ((ld * esz) % 16 == 0));
    };
    if (!(al(p.C, p.ldc, csz) && al(e.preact, e.ld_preact, csz) && al(e.grad_src, e.ld_grad, csz) && al(e.residual, e.ld_res, csz) &&
          al(e.bias, 0, 4)))
      return 0;
  }
  if ((int64_t)p.M * p.N < (int64_t)1 << 21 || p.M < 256 || p.N < 128) return 0;   // small problems: the 128 x 128 kernel fills the chip better
  int pick = mode;
  if (pick == 1) {
    const double c256 = big_cost(p.M, p.N, 256, 256, 5080.0), c384 = big_cost(p.M, p.N, 384, 192, 5550.0);
    const double c128 = b_kmajor ? big_cost(p.M, p.N, 256, 128, 2760.0) : 1e30;   // mn-major B: measured behind the 128 x 128 kernel
    pick = 256;
    double best = c256;
    if (c384 < best) { best = c384; pick = 384; }
    if (c128 < best) { best = c128; pick = 128; }
    if (best > 0.95 * small_cost(p.M, p.N)) return 0;      // how much better than the 128 x 128 kernel the model must predict
  }
  if (b_kmajor) {
    if (pick == 384) return launch_big<Big384<true>>(p, st);
    if (pick == 128) return launch_big<Big128<true>>(p, st);
    return launch_big<Big256<true>>(p, st);
  }
  if (pick == 384) return launch_big<Big384<false>>(p, st);
  if (pick == 128) return launch_big<Big128<false>>(p, st);
  return launch_big<Big256<false>>(p, st);
}

// ---- weight gradients with both operands mn-major: C[M][N] = A[K][M]^T B[K][N] on 384 x 192 tiles with split-k ----
// The pair heads' dW1 = dz^T x (M = 5 x 384, N = 384, K = all pairs of the batch) is the deepest contraction of the step and
// fill-bound on the 128 x 128 kernel (32 KiB staged per 2.1 MFLOP); 1920 x 384 is exactly 5 x 2 tiles of 384 x 192, which stage
// 72 KiB per 9.4 MFLOP: half the bytes.  tiles x split_k one-per-CU workgroups; partials leave as plain fp32 (PART) and
// peneo_gemm's split-k reduce applies `accumulate`.
// Taken only when ALL hold (everything else stays on its kernel): fp32 C, no epilogue option beyond accumulate, no a_colsum,
// M % 384 == 0, N % 192 == 0, K % 8 == 0, 16-byte aligned C / workspace rows, and K >= NN_MIN_K.
//   NN_MIN_K = 65536: the other (mn, mn) callers contract over the tokens of a batch (encoder / patch-embedding / decoder-input
//   weight gradients: K <= 8192 at every configuration), where the 128 x 128 kernel's M N / 16384 tiles x its own split fill the
//   chip and a workgroup's range is a few k-tiles; dW1 contracts over pairs (K = 8256 per document of 128 lines, 1 081 344 at the
//   benchmark shape), where a range is hundreds of k-tiles and the 144 KiB ring's prologue and the partial store are noise.
using BigNN384 = BigCfg<false, 4, 2, 3, 3, 2, false>;
constexpr int NN_MIN_K = 65536;

static int g_nn_mode = -1;    // PENEO_GEMM_NN384: 0 = off, 1 = by the rule above (default), 2 = without the K bound (tests, tools)

static std::atomic<uint64_t> g_nn_launches{0};   // calls that took the path (the tests' proof of routing: the 128 x 128 kernel sums
                                                 // the same k-steps in the same order, so the results alone cannot tell)

static int nn_mode() {
  if (g_nn_mode < 0) { const char* e = getenv("PENEO_GEMM_NN384"); g_nn_mode = e ? atoi(e) : 1; }
  return big_mode() == 0 ? 0 : g_nn_mode;      // PENEO_GEMM_BIG=0 switches every big-tile path off
}

// the shape part of the rule under the mode in force: the one copy, also what a caller sizes its split-k by (peneo_gemm_nn384_shape_ok)
static bool nn_shape_ok(int M, int N, int K) {
  const int mode = nn_mode();
  if (mode == 0 || M <= 0 || N <= 0 || K <= 0) return false;
  if (M % BigNN384::BM != 0 || N % BigNN384::BN != 0 || K % 8 != 0) return false;
  return mode != 1 || K >= NN_MIN_K;
}

int launch_gemm_big_nn(const GemmParams& p, hipStream_t st) {
  if (!nn_shape_ok(p.M, p.N, p.K)) return 0;
  const peneo_gemm_epilogue& e = p.ep;
  if (p.c_dtype != PENEO_F32 || p.dz_on || e.bias || e.preact || e.grad_src || e.residual || e.a_colsum || e.act != PENEO_ACT_NONE ||
      e.drop_p != 0.f || e.alpha != 1.f)
    return 0;
  if ((reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.B) | reinterpret_cast<uintptr_t>(p.C)) & 15) return 0;
  if (p.lda % 8 != 0 || p.ldb % 8 != 0 || p.ldc % 4 != 0) return 0;
  // per-lane source offsets are 32-bit: 64 rows of the operand
  if ((int64_t)64 * p.lda * 2 >= ((int64_t)1 << 31) || (int64_t)64 * p.ldb * 2 >= ((int64_t)1 << 31)) return 0;
  if (p.split_k > 1 && (p.ws == nullptr || (reinterpret_cast<uintptr_t>(p.ws) & 15))) return 0;
  g_nn_launches.fetch_add(1, std::memory_order_relaxed);
  return p.split_k > 1 ? launch_big<BigNN384, true>(p, st) : launch_big<BigNN384, false>(p, st);
}

// ---- the grouped form: up to GEMM_GROUP_MAX (mn, mn) weight gradients as ONE launch of whole-K 384 x 192 tiles ----
// An encoder layer's four weight gradients are 24 + 32 + 32 + 8 = 96 such tiles: 96 one-per-CU workgroups that stage 72 KiB per
// k-tile, half the bytes of the 432 tiles of 128 x 128.  peneo_gemm_group takes this path only when EVERY problem of the
// call passes the rule, which is launch_gemm_big_nn's without the K bound and without a split:
//   bf16 operands, A [K][M], B [K][N], fp32 C, no epilogue option beyond accumulate, M % 384 == 0, N % 192 == 0, K % 8 == 0,
//   16-byte aligned operands and C rows, 64 rows of A or B below 2 GiB, and the mode allows it.
static int g_group_nn_mode = -1;   // PENEO_WGRAD_NN384: 0 = off, 1 = on (default, by measurement: DESIGN 32), 2 = on except for the layer the encoder backward issues last
static std::atomic<uint64_t> g_group_nn_launches{0};

static int group_nn_mode() {
  if (g_group_nn_mode < 0) {      // read once; a negative value of the variable is 0, as in the setter
    const char* e = getenv("PENEO_WGRAD_NN384");
    const int v = e ? atoi(e) : 1;
    g_group_nn_mode = v < 0 ? 0 : v;
  }
  return big_mode() == 0 ? 0 : g_group_nn_mode;
}

int launch_gemm_big_group(const GemmParams* ps, int n, hipStream_t st) {
  if (group_nn_mode() == 0 || n < 1 || n > GEMM_GROUP_MAX) return 0;
  BigGroup g;
  g.n = n;
  int Ms[GEMM_GROUP_MAX], Ns[GEMM_GROUP_MAX];
  for (int i = 0; i < GEMM_GROUP_MAX; ++i) {
    const GemmParams& p = ps[i < n ? i : n - 1];
    if (i < n) {
      Ms[i] = p.M; Ns[i] = p.N;
      const peneo_gemm_epilogue& e = p.ep;
      if (p.c_dtype != PENEO_F32 || p.dz_on || p.split_k > 1 || e.bias || e.preact || e.grad_src || e.residual || e.a_colsum ||
          e.act != PENEO_ACT_NONE || e.drop_p != 0.f || e.alpha != 1.f)
        return 0;
      if (p.M <= 0 || p.N <= 0 || p.K < 8 || p.M % BigNN384::BM != 0 || p.N % BigNN384::BN != 0 || p.K % 8 != 0) return 0;
      if ((reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.B) | reinterpret_cast<uintptr_t>(p.C)) & 15) return 0;
      if (p.lda % 8 != 0 || p.ldb % 8 != 0 || p.ldc % 4 != 0) return 0;
      // per-lane source offsets are 32-bit: 64 rows of the operand
      if ((int64_t)64 * p.lda * 2 >= ((int64_t)1 << 31) || (int64_t)64 * p.ldb * 2 >= ((int64_t)1 << 31)) return 0;
    }
    BigGroupProblem& q = g.q[i];
    q.A = p.A; q.B = p.B; q.C = p.C; q.lda = p.lda; q.ldb = p.ldb; q.ldc = p.ldc; q.M = p.M; q.N = p.N; q.K = p.K;
    q.accumulate = p.ep.accumulate ? 1 : 0;
  }
  const int tiles = walk_group_fill(Ms, Ns, n, GEMM_GROUP_MAX, BigNN384::BM, BigNN384::BN, g.first_tile, g.tiles_n);
  static std::atomic<uint64_t> lds_devices{0};
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(gemm_big_group_kernel<BigNN384>), BigNN384::LDS_BYTES, lds_devices))
    return dynamic_lds_error("peneo_gemm_group", BigNN384::LDS_BYTES);
  hipLaunchKernelGGL((gemm_big_group_kernel<BigNN384>), dim3((unsigned)tiles), dim3(512), BigNN384::LDS_BYTES, st, g);
  const int rc = check_launch("peneo_gemm_group (384 x 192 tiles)");
  if (rc != PENEO_OK) return rc;
  g_group_nn_launches.fetch_add(1, std::memory_order_relaxed);
  return 1;
}

int gemm_group_nn384_mode() { return group_nn_mode(); }

}  // namespace peneo

/* tools/ only (not in the header): 0 = off, 1 = choose by the cost model, 256 / 384 / 128 = force that tile shape */
extern "C" void peneo_gemm_set_big_mode(int mode) { peneo::g_big_mode = mode; }
extern "C" int peneo_gemm_big_mode(void) { return peneo::big_mode(); }
/* 0 = off, 1 = the rule of launch_gemm_big_nn, 2 = that rule without its bound on K */
extern "C" void peneo_gemm_set_nn384_mode(int mode) { peneo::g_nn_mode = mode; }
extern "C" int peneo_gemm_nn384_mode(void) { return peneo::nn_mode(); }
extern "C" int peneo_gemm_nn384_shape_ok(int M, int N, int K) { return peneo::nn_shape_ok(M, N, K) ? 1 : 0; }
extern "C" uint64_t peneo_gemm_nn384_launches(void) { return peneo::g_nn_launches.load(std::memory_order_relaxed); }
/* grouped weight gradients on the 384 x 192 tile: 0 = off, 1 = on, 2 = on except for the layer peneo_encoder_layer_bwd is told is last */
extern "C" void peneo_gemm_group_set_nn384_mode(int mode) { peneo::g_group_nn_mode = mode < 0 ? 0 : mode; }
extern "C" int peneo_gemm_group_nn384_mode(void) { return peneo::group_nn_mode(); }
extern "C" uint64_t peneo_gemm_group_nn384_launches(void) { return peneo::g_group_nn_launches.load(std::memory_order_relaxed); }
