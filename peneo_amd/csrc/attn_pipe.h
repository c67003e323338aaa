// The device primitives the attention kernels share (attention.hip and the pipelined attn_*_pipe.hip / attn2_*_pipe.hip): the softmax
// constants, the XCD-aware unit order, the source-slot permutation of the LDS-DMA images, the transpose readers, the dword LDS-DMA,
// the dropout keep-mask helpers and the accumulator-row writer.  Everything here is inlined; tile geometry and device globals stay
// with their kernels.
#pragma once
#include "common.h"

namespace peneo {
namespace {

constexpr float kMasked = -1.0e30f;
// the running maximum of the online softmax only moves when a tile beats it by more than this (natural units): exponentials
// stay below e^4 and the rescaling of the accumulators - one multiply per element - is skipped for almost every tile
constexpr float kRescaleTau = 4.0f;

// Unit order of a one-dimensional grid whose units come in runs that stream the same rows (the query or key blocks of one
// (document, head)): consecutive workgroups go to the eight XCDs in turn, so workgroup L runs on XCD L & 7 and is handed unit
// (units before that XCD's share) + L >> 3 - every XCD works through ONE contiguous range of units and a run stays in one L2.
__device__ __forceinline__ int xcd_unit() {
  const int nwg = gridDim.x, L = blockIdx.x, q8 = nwg >> 3, r8 = nwg & 7, x = L & 7, i = L >> 3;
  return (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + i;
}

// DMA images are lane-linear, so bank conflicts are removed by permuting the SOURCE 16-byte slots of a row (the read applies the
// same involution).  Rows of 128 bytes (64 bf16 of a Q / K / V / dO row) use slot ^ bitrev3(row >> 1): conflict-free for the b128
// fragment reads AND for the transpose reads (rows r, r + 2 land in different 64-byte groups).
__device__ __forceinline__ int bitrev3(int x) { return ((x & 1) << 2) | (x & 2) | ((x >> 2) & 1); }
__device__ __forceinline__ int row128_slot_swz(int row) { return bitrev3((row >> 1) & 7); }

// ds_read_b64_tr_b16: one transpose read of a [4 k][16 rows] block per 16-lane group (EXEC all ones)
typedef short s16x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 tr64(const char* p) {
  typedef __attribute__((address_space(3))) s16x4_t* lds_s4p;
  return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4p)p));
}
// two of them = one MFMA fragment
__device__ __forceinline__ Frag<bf16_t> tr_frag(const char* lo, const char* hi) {
  const uint2 a = tr64(lo), b = tr64(hi);
  Frag<bf16_t> f;
  f.v = make_uint4(a.x, a.y, b.x, b.y);
  return f;
}

// 64 lanes x 4 bytes: global (uniform base + lane offset) -> LDS (uniform base + 4 * lane).  Inline asm for the reason given at
// lds_dma_1k (common.h); m0 is saved and restored around the instruction.
__device__ __forceinline__ void dma4_s(uint32_t voff_lane, const char* base_uniform, uint32_t lds_uniform) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff_lane), "s"(base_uniform), "s"(lds_uniform) : "memory");
}
// ... with a full per-lane pointer
__device__ __forceinline__ void dma4_v(const char* ptr_lane, uint32_t lds_uniform) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(ptr_lane), "s"(lds_uniform) : "memory");
}

// x where the lane's bit of the 64-bit mask is set, else 0 (mask in an SGPR pair).  s_nop 1: the pair comes from v_readlane,
// and gfx950 wants two wait states between a VALU write of an SGPR and a VALU read of it; the compiler pads that hazard for
// instructions it can see, not inside inline asm (the fp32 kernel's schedule put the two back to back: wrong masks)
__device__ __forceinline__ float mask_keep(float x, uint64_t m) {
  float r;
  asm("s_nop 1\n\tv_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(x), "s"(m));
  return r;
}
// register mask i of a forward tile from the wave's 64 keep words (lane L holds word L of the tile): two v_readlane into
// an SGPR pair.  (Scalar loads of the words straight into SGPRs were tried first: left to the compiler they sit right in
// front of the first use with a full s_waitcnt each - SMEM returns out of order - and the forward ran slower than with the
// hash; issued by hand at the top of the tile, the register allocator spilled the destination SGPRs between the load and
// the wait, i.e. before the data had arrived.)
__device__ __forceinline__ uint64_t lane_words_mask(uint32_t w, int word /* even, wave-uniform */) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)w, word), hi = (uint32_t)__builtin_amdgcn_readlane((int)w, word + 1);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
// the backward's form of the mask: m = 0 / -1 from one v_bfe_i32 of the key's keep word
__device__ __forceinline__ uint32_t and_u(float x, int m) { return __float_as_uint(x) & (uint32_t)m; }

// 8 bf16 of a row, times `scale`, rounded to bf16 again (peneo_head_concat's arithmetic; exact for a power of two)
__device__ __forceinline__ uint4 scaled8(const bf16_t* p, float scale, bool ok) {
  float f[8];
  unpack16<bf16_t>(*reinterpret_cast<const uint4*>(p), f);
  if (scale != 1.0f) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] *= scale;
  }
  const uint4 v = pack16<bf16_t>(f);
  return ok ? v : make_uint4(0u, 0u, 0u, 0u);
}

// rows d = 16 m + 8 half .. + 7 of an accumulator tile [d rows (registers)][key or query (lane)], times mul, as 8 bf16: a lane holds
// d = 8 g + 4 half + 0..3 of each register group g, so two groups and a v_permlane32_swap make 16 contiguous bytes per lane (run
// with every lane active)
__device__ __forceinline__ uint4 acc_piece(const f32x16_t& a, int m, float mul) {
  uint32_t ax = pack_bf16x2(a[8 * m + 0] * mul, a[8 * m + 1] * mul), ay = pack_bf16x2(a[8 * m + 2] * mul, a[8 * m + 3] * mul);
  uint32_t bx = pack_bf16x2(a[8 * m + 4] * mul, a[8 * m + 5] * mul), by = pack_bf16x2(a[8 * m + 6] * mul, a[8 * m + 7] * mul);
  const auto rx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
  const auto ry = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
  return make_uint4(rx[0], ry[0], rx[1], ry[1]);
}

}  // namespace
}  // namespace peneo
