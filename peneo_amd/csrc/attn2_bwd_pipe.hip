// Two-stream attention backward, pipelined (bf16, head dims 64 + 16: LiLT's text and layout streams).  The gradients of
//
//     scores[b, h, i, j] = (scale_a q_a) . k_a + (scale_b q_b) . k_b + key_bias[b, j]     P = softmax (dropout on P)
//     out_a = P v_a,  out_b = P v_b
//
// with respect to the UNSCALED q_a, k_a, v_a, q_b, k_b, v_b - what the concat path delivers (peneo_head_concat of the two output
// gradients -> attn_delta_kernel, attn_bwd_fused_kernel<96>, attn_dq_from_ds_kernel<96> at scale 1 -> peneo_head_split x 2 with the
// scales on dq), with the same arithmetic in the same order and the same bits, but without the three packed copies: the operands
// are read where the QKV GEMMs and the forward left them, and dq | dk | dv of both streams are written into the two gradient
// buffers the QKV weight-gradient and data-gradient GEMMs read.  Three launches, the skeletons of attn_bwd_pipe.hip:
//
//   1. delta[b, h, q] = sum dO_a . O_a + sum dO_b . O_b: eight lanes per (token, head) row with 16-byte loads.  The sums keep
//      attn_delta_kernel's association at head dim 80 (lane c of 64: O[c] dO[c], + O[64 + c] dO[64 + c] for c < 16; then the
//      lane ^ 32, 16, 8, 4, 2, 1 butterfly): element c sits in lane c / 8, slot c % 8, so the first three butterfly steps are
//      element-wise lane ^ 4, 2, 1 exchanges and the last three run inside the lane.
//   2. dK / dV / dS^T: a workgroup owns 128 keys of one (document, head) - lane = key; the K_a, K_b, V_a, V_b fragments and the
//      dK / dV accumulators of both streams in registers - and streams 32-query tiles by LDS-DMA into a ring of three (request for
//      tile t + 2 at the top of iteration t), ONE s_barrier per tile, S of tile t + 1 computed at the end of iteration t, dS^T
//      through the per-wave patch and stored one tile late, dK / dV rows out of the accumulator layout by v_permlane32_swap,
//      XCD-contiguous unit order.  A tile's buffer: Q_a and dO_a [32][128 B] (source slot ^ bitrev3(row >> 1)), Q_b and dO_b
//      [32][32 B] (one 1 KiB piece each; the two 16-byte halves of rows 16..31 swapped), lse, delta and the keep words: 11 KiB, no
//      bias block - the key bias of a lane's key is a lane constant.  The 32-byte rows are read two ways: the b128 fragment reads
//      of S / dP (row = lane & 31, half = lane >> 5: with the swap each 16-lane group covers the 256-byte bank row once) and the
//      transpose reads of dK_b / dV_b (four rows x 32 B per 16-lane group: 128 contiguous bytes per group whatever the order of
//      the halves; the groups of the 16 d-rows that do not exist read the OTHER eight query rows of the step, so the wave covers
//      512 contiguous bytes with EXEC all ones, and zero their fragment afterwards).  Neither read conflicts.
//      S and dP: four text k-steps then one layout k-step into one accumulator (step six of the DP = 96 kernel multiplies zeros).
//      The concat path pre-scales q; here the register-resident K fragments carry the scales (S) and the dK epilogue multiplies
//      by them: for powers of two that is the same arithmetic bit for bit.
//   3. dQ from the slab: 128 queries per workgroup, 32-key tiles of the slab, of K_a [32][128 B] and of K_b [32][32 B] read in
//      place; three accumulators; dq_a and dq_b leave with their scales (peneo_head_split's).
// The workspace (delta, then the slab) is the caller's; every byte that is read was written by this call.  Nothing here waits on
// another workgroup.
#include "common.h"
#include "attention.h"
#include "attn_pipe.h"

namespace peneo {
namespace {

struct Attn2BwdParams {
  const void* q_a; const void* k_a; const void* v_a; int64_t ld_a;
  const void* q_b; const void* k_b; const void* v_b; int64_t ld_b;
  const void* out_a; const void* d_out_a; int64_t ld_out_a;
  const void* out_b; const void* d_out_b; int64_t ld_out_b;
  const float* lse; int B, nh, T, Tp; float scale_a, scale_b;
  const float* key_bias;
  void* dq_a; void* dk_a; void* dv_a; int64_t ld_da;
  void* dq_b; void* dk_b; void* dv_b; int64_t ld_db;
  float* delta; void* slab;                                        // the workspace: fp32 [B, nh, T], bf16 [B, nh, T keys, Tp queries]
  float keep_scale; const uint32_t* words; int nqb, Tk;           // dropout keep bits (peneo_attn_drop_words) or NULL
};

constexpr int DA = 64, DB = 16;   // head dims of the two streams
constexpr int TQ = 32;            // queries per tile
constexpr int WK = 128;           // keys per workgroup (4 waves x 32)
// a tile's buffer: Q_a [32][128 B], dO_a [32][128 B], Q_b [32][32 B], dO_b [32][32 B], lse [64], delta [64], keep words [128]
constexpr int O_QA = 0, O_DOA = 4096, O_QB = 8192, O_DOB = 9216, O_LSE = 10240, O_DELTA = 10496, O_WORDS = 10752, BUF = 11264;
constexpr int STG_PITCH = 80, STG_WAVE = 32 * STG_PITCH;
constexpr int NBUF = 3;
constexpr int LDS_BYTES = NBUF * BUF + 4 * STG_WAVE;

__device__ float g_lse_pad2 = 1.0e30f;   // lse of query rows past T
__device__ uint4 g_zero_line2[8];        // 128 zero bytes (device globals are zero-initialised)

// ================================================================================================
// 1. delta
// ================================================================================================
__global__ __launch_bounds__(256) void attn2_delta_kernel(Attn2BwdParams p) {
  typedef bf16_t T;
  const int64_t item = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;      // (b * T + q) * nh + h
  const int sub = threadIdx.x & 7;
  const int64_t total = (int64_t)p.B * p.T * p.nh;
  const bool ok = item < total;
  const int64_t it = ok ? item : total - 1;
  const int h = (int)(it % p.nh);
  const int64_t tok = it / p.nh;                                             // b * T + q
  float a[8], g[8], x[8];
  unpack16<T>(*reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.out_a) + tok * p.ld_out_a + h * DA + sub * 8), a);
  unpack16<T>(*reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.d_out_a) + tok * p.ld_out_a + h * DA + sub * 8), g);
#pragma unroll
  for (int e = 0; e < 8; ++e) { x[e] = 0.f; x[e] += a[e] * g[e]; }
  if (sub < 2) {                                                             // elements 64 .. 79 of the packed row: the layout stream
    unpack16<T>(*reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.out_b) + tok * p.ld_out_b + h * DB + sub * 8), a);
    unpack16<T>(*reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.d_out_b) + tok * p.ld_out_b + h * DB + sub * 8), g);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] += a[e] * g[e];
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1)                                            // elements c ^ 32, c ^ 16, c ^ 8
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] += __shfl_xor(x[e], o, 64);
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] += x[e + 4];                              // c ^ 4, c ^ 2, c ^ 1
  x[0] += x[2]; x[1] += x[3];
  x[0] += x[1];
  if (ok && sub == 0) {
    const int64_t b = tok / p.T, q = tok % p.T;
    p.delta[(b * p.nh + h) * p.T + q] = x[0];
  }
}

// ================================================================================================
// 2. dK, dV and the dS^T slab
// ================================================================================================
template <bool DROP>
__global__ __launch_bounds__(256, 2) void attn2_bwd_pipe_kernel(Attn2BwdParams p) {
  typedef bf16_t T;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Tn = p.T, Tp = p.Tp;
  // unit order: the key blocks of one (document, head) run on ONE XCD (they stream the same Q / dO rows through its L2)
  const int nkb = (Tn + WK - 1) / WK;
  const int u = xcd_unit();
  const int kb = u % nkb, bh = u / nkb, h = bh % p.nh, b = bh / p.nh;
  const int key0 = kb * WK;
  const int keyl = wave * 32 + l31, mykey = key0 + keyl;
  const int64_t row0 = (int64_t)b * Tn;
  const T* Qa = reinterpret_cast<const T*>(p.q_a) + row0 * p.ld_a + h * DA;
  const T* Ka = reinterpret_cast<const T*>(p.k_a) + row0 * p.ld_a + h * DA;
  const T* Va = reinterpret_cast<const T*>(p.v_a) + row0 * p.ld_a + h * DA;
  const T* Qb = reinterpret_cast<const T*>(p.q_b) + row0 * p.ld_b + h * DB;
  const T* Kb = reinterpret_cast<const T*>(p.k_b) + row0 * p.ld_b + h * DB;
  const T* Vb = reinterpret_cast<const T*>(p.v_b) + row0 * p.ld_b + h * DB;
  const T* dOa = reinterpret_cast<const T*>(p.d_out_a) + row0 * p.ld_out_a + h * DA;
  const T* dOb = reinterpret_cast<const T*>(p.d_out_b) + row0 * p.ld_out_b + h * DB;
  const float* lse = p.lse + (int64_t)bh * Tn;
  const float* delta = p.delta + (int64_t)bh * Tn;
  const float keep_scale = DROP ? p.keep_scale : 1.0f;
  const int nt = (Tn + TQ - 1) / TQ;

  // ---- K / V fragments of this lane's key (B operands of S and dP): four text k-steps, one layout k-step; K carries the scales ----
  Frag<T> kf[5], vf[5];
  float my_kb;                                       // key bias of this lane's key (natural units)
  {
    const bool ok = mykey < Tn;
    const int64_t kr = ok ? mykey : 0;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      kf[ks].v = scaled8(Ka + kr * p.ld_a + 8 * half + 16 * ks, p.scale_a, ok);
      vf[ks].v = scaled8(Va + kr * p.ld_a + 8 * half + 16 * ks, 1.0f, ok);
    }
    kf[4].v = scaled8(Kb + kr * p.ld_b + 8 * half, p.scale_b, ok);
    vf[4].v = scaled8(Vb + kr * p.ld_b + 8 * half, 1.0f, ok);
    my_kb = ok ? (p.key_bias ? p.key_bias[(int64_t)b * Tp + mykey] : 0.f) : kMasked;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // from here on the vm counter holds the DMA pieces and the slab stores only
#pragma unroll
  for (int ks = 0; ks < 5; ++ks) {
    asm volatile("" : "+v"(kf[ks].v.x), "+v"(kf[ks].v.y), "+v"(kf[ks].v.z), "+v"(kf[ks].v.w));
    asm volatile("" : "+v"(vf[ks].v.x), "+v"(vf[ks].v.y), "+v"(vf[ks].v.z), "+v"(vf[ks].v.w));
  }
  asm volatile("" : "+v"(my_kb));

  const bool wave_on = key0 + wave * 32 < Tn;      // a wave whose 32 keys all lie past T only serves the DMA stream and the barriers

  // ---- DMA sources of this wave's pieces (lane constants; a tile adds a uniform base) ----
  //   wave w: Q_a piece w, dO_a piece w (rows 8 w .. 8 w + 7); wave 2 the whole Q_b tile, wave 3 the whole dO_b tile (lane: row
  //   lane / 2, half lane & 1); wave 0 lse, wave 1 delta, waves 2 and 3 the keep words 0..63 | 64..127
  const uint32_t lds0 = lds_addr(smem);
  const uint32_t ldq2 = (uint32_t)(p.ld_a * 2), ldo2 = (uint32_t)(p.ld_out_a * 2);
  const uint32_t ldb2 = (uint32_t)((wave == 2 ? p.ld_b : p.ld_out_b) * 2);       // (waves 2 and 3 only)
  const int qrow = 8 * wave + (lane >> 3);
  const uint32_t qcol = (uint32_t)(((lane & 7) ^ row128_slot_swz(qrow)) << 4);
  const int brow = lane >> 1;
  const uint32_t bcol = (uint32_t)(((lane & 1) ^ (brow >> 4)) << 4);
  // tiles are requested strictly in order: the uniform source pointers of the NEXT tile to request run along (scalar adds)
  const char* nq = reinterpret_cast<const char*>(Qa);
  const char* ndo = reinterpret_cast<const char*>(dOa);
  const char* nb = reinterpret_cast<const char*>(wave == 2 ? Qb : dOb);          // (waves 2 and 3 only)
  const char* ndl = reinterpret_cast<const char*>(delta);
  const char* nw = DROP ? reinterpret_cast<const char*>(p.words + (int64_t)bh * p.nqb * (int64_t)p.Tk + key0) : nullptr;
  const float* nl = lse;
  int nq0 = 0;                                                            // first query of that tile
  auto dma_tile = [&](auto buf_c) {
    const int buf = buf_c;                              // an integral_constant (static ring position) or a plain int
    const int lim = Tn - 1 - nq0;                       // (query rows past T: clamped to T - 1, finite; their P is 0)
    const uint32_t dst = lds0 + buf * BUF;
    const uint32_t qr = (uint32_t)min(qrow, lim);
    lds_dma_1k_s<0>(qr * ldq2 + qcol, nq, dst + O_QA + wave * 1024);
    lds_dma_1k_s<0>(qr * ldo2 + qcol, ndo, dst + O_DOA + wave * 1024);
    if (wave >= 2) lds_dma_1k_s<0>((uint32_t)min(brow, lim) * ldb2 + bcol, nb, dst + (wave == 2 ? O_QB : O_DOB));
    if (wave == 0) {
      const char* src = (nq0 + lane < Tn) ? reinterpret_cast<const char*>(nl + lane) : reinterpret_cast<const char*>(&g_lse_pad2);
      dma4_v(src, dst + O_LSE);
    } else if (wave == 1) {
      dma4_s((uint32_t)min(lane, lim) * 4u, ndl, dst + O_DELTA);
    } else if (DROP) {
      dma4_s((uint32_t)((wave - 2) * 64 + lane) * 4u, nw, dst + O_WORDS + (wave - 2) * 256);
    }
    nq += (int64_t)TQ * ldq2; ndo += (int64_t)TQ * ldo2; nb += (int64_t)TQ * ldb2; ndl += TQ * 4; nl += TQ; nq0 += TQ;
    if (DROP) nw += (int64_t)p.Tk * 4;
  };

  // ---- LDS read addresses (lane constants relative to a buffer) ----
  // S / dP fragment of text k-step ks: row l31, slot (2 ks + half) ^ swz = base ^ (ks << 5); of the layout k-step: aSb
  const int aS0 = l31 * 128 + ((half ^ row128_slot_swz(l31)) << 4);
  const int aSb = l31 * 32 + ((half ^ (l31 >> 4)) << 4);
  const int li = lane & 15, lj = (lane >> 4) & 1;
  int aT[2][2];                                      // transpose reads of the Q_a / dO_a tile: [d tile][rows +0 / +8]; + 2048 kk
  int aTb[2];                                        // of the Q_b / dO_b tile: [rows +0 / +8]; (^ (kk << 4)) + 512 kk
#pragma unroll
  for (int w8 = 0; w8 < 2; ++w8) {
    const int row = 4 * half + (li >> 2) + 8 * w8;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      const int slot = 4 * t2 + 2 * lj + ((li & 3) >> 1);
      aT[t2][w8] = row * 128 + ((slot ^ row128_slot_swz(row)) << 4) + ((li & 1) << 3);
    }
    aTb[w8] = (row ^ (8 * lj)) * 32 + ((li & 3) << 3);   // (lj = 1: the pad rows' groups read the other eight query rows)
  }
  const int aW = attn_kslot(keyl) * 4;
  char* stg = smem + NBUF * BUF + wave * STG_WAVE;
  char* stg_w = stg + l31 * STG_PITCH + 8 * half;                       // + 16 g
  const char* stg_r = stg + (lane >> 2) * STG_PITCH + (lane & 3) * 16;  // + 16 rows: STG_PITCH * 16
  T* slab = reinterpret_cast<T*>(p.slab) + ((int64_t)bh * Tn + key0 + wave * 32) * (int64_t)Tp;   // uniform
  const int slab_l = (lane >> 2) * Tp + (lane & 3) * 8;                                            // + 16 rows: 16 Tp

  f32x16_t dk[2], dv[2], dkb, dvb, s;
#pragma unroll
  for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f; dkb[r] = 0.f; dvb[r] = 0.f; s[r] = 0.f; }

  auto s_tile = [&](const char* buf) {               // S[q, key] of a tile: A = Q rows, B = K fragments
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      Frag<T> a;
      a.v = *reinterpret_cast<const uint4*>(buf + O_QA + (aS0 ^ (ks << 5)));
      mma_step(a, kf[ks], acc);
    }
    Frag<T> a;
    a.v = *reinterpret_cast<const uint4*>(buf + O_QB + aSb);
    mma_step(a, kf[4], acc);
    return acc;
  };
  auto flush = [&](int tt) {                         // dS^T of tile tt: the wave's patch -> 64-byte row pieces of the slab
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (lane >> 2) + 16 * i;
      const uint4 v = *reinterpret_cast<const uint4*>(stg_r + i * 16 * STG_PITCH);
      if (key0 + wave * 32 + row < Tn) *reinterpret_cast<uint4*>(slab + tt * TQ + 16 * i * Tp + slab_l) = v;
    }
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  dma_tile(I0{});
  if (nt > 1) dma_tile(I1{});
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  s = s_tile(smem);

  // one tile; the ring position is a compile-time constant (the loop below is unrolled over the ring), so every LDS address of
  // the body is a lane constant plus an immediate
  auto tile = [&](auto cur_c, int t) {
    const int cur = cur_c, nxt = cur + 1 == NBUF ? 0 : cur + 1, nn = nxt + 1 == NBUF ? 0 : nxt + 1;
    if (t > 0) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the next tile has landed (and the stores of tile t - 2 are out)
      __builtin_amdgcn_s_barrier();
    }
    if (t + 2 < nt) dma_tile(nn);
    if (t > 0) flush(t - 1);
    const char* buf = smem + cur * BUF;
    if (!wave_on) return;                              // (wave-uniform; the barrier and this wave's DMA pieces are above)

    // dP[q, key] = dO . V^T
    f32x16_t dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      Frag<T> a;
      a.v = *reinterpret_cast<const uint4*>(buf + O_DOA + (aS0 ^ (ks << 5)));
      mma_step(a, vf[ks], dp);
    }
    {
      Frag<T> a;
      a.v = *reinterpret_cast<const uint4*>(buf + O_DOB + aSb);
      mma_step(a, vf[4], dp);
    }
    uint32_t cw = 0u;
    if constexpr (DROP) cw = *reinterpret_cast<const uint32_t*>(buf + O_WORDS + aW) >> (4 * half);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      // P = exp2((S + key bias) log2e - lse); dS = P (dP keep / (1 - p) - delta); bf16 pairs in MFMA operand order
      uint32_t pp[4], dd[4];
#pragma unroll
      for (int gg = 0; gg < 2; ++gg) {
        const int g = 2 * kk + gg;
        const float4 l4 = *reinterpret_cast<const float4*>(buf + O_LSE + 16 * half + 32 * g);
        const float4 d4 = *reinterpret_cast<const float4*>(buf + O_DELTA + 16 * half + 32 * g);
        const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dl[4] = {d4.x, d4.y, d4.z, d4.w};
        float pd[4], ds[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const float pv = __builtin_amdgcn_exp2f(fmaf(fmaf(s[r], 1.0f, my_kb), kLog2e, -lv[e]));   // (bit for bit the fused kernel's order)
          if constexpr (DROP) {
            const int m = __builtin_amdgcn_sbfe((int)cw, 8 * g + e, 1);   // 0 / -1: bit (8 g + e) = this lane's query of register r
            pd[e] = __uint_as_float(and_u(pv, m));                        // (1 / (1 - p) goes onto dV once, at the end)
            ds[e] = pv * fmaf(dp[r], __uint_as_float(and_u(keep_scale, m)), -dl[e]);
          } else {
            pd[e] = pv;
            ds[e] = pv * (dp[r] - dl[e]);
          }
        }
        pp[2 * gg] = pack_bf16x2(pd[0], pd[1]); pp[2 * gg + 1] = pack_bf16x2(pd[2], pd[3]);
        dd[2 * gg] = pack_bf16x2(ds[0], ds[1]); dd[2 * gg + 1] = pack_bf16x2(ds[2], ds[3]);
        *reinterpret_cast<uint2*>(stg_w + 16 * g) = make_uint2(dd[2 * gg], dd[2 * gg + 1]);
      }
      // dV^T[d, key] += dO^T[d, q] . P[q, key] ;  dK^T[d, key] += Q^T[d, q] . dS[q, key]   (these 16 queries)
      Frag<T> pf, dsf;
      pf.v = make_uint4(pp[0], pp[1], pp[2], pp[3]);
      dsf.v = make_uint4(dd[0], dd[1], dd[2], dd[3]);
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const Frag<T> dot = tr_frag(buf + O_DOA + 2048 * kk + aT[t2][0], buf + O_DOA + 2048 * kk + aT[t2][1]);
        mma_step(dot, pf, dv[t2]);
        const Frag<T> qtf = tr_frag(buf + O_QA + 2048 * kk + aT[t2][0], buf + O_QA + 2048 * kk + aT[t2][1]);
        mma_step(qtf, dsf, dk[t2]);
      }
      // the layout d-tile: rows 16 .. 31 do not exist (zero fragments for their 16-lane groups)
      Frag<T> dob = tr_frag(buf + O_DOB + 512 * kk + (aTb[0] ^ (kk << 4)), buf + O_DOB + 512 * kk + (aTb[1] ^ (kk << 4)));
      if (lj) dob.v = make_uint4(0u, 0u, 0u, 0u);
      mma_step(dob, pf, dvb);
      Frag<T> qbf = tr_frag(buf + O_QB + 512 * kk + (aTb[0] ^ (kk << 4)), buf + O_QB + 512 * kk + (aTb[1] ^ (kk << 4)));
      if (lj) qbf.v = make_uint4(0u, 0u, 0u, 0u);
      mma_step(qbf, dsf, dkb);
    }
    if (t + 1 < nt) s = s_tile(smem + nxt * BUF);
  };
  {                            // the ring position is static: three copies of the body
    int t = 0;
    for (; t + 3 <= nt; t += 3) { tile(I0{}, t); tile(I1{}, t + 1); tile(I2{}, t + 2); }
    if (t < nt) tile(I0{}, t);
    if (t + 1 < nt) tile(I1{}, t + 1);
  }
  flush(nt - 1);
  // the slab's columns between the last tile and Tp are zero (its reader loads whole 16-byte groups up to Tp)
  for (int c = nt * TQ; c < Tp; c += TQ) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (lane >> 2) + 16 * i;
      if (key0 + wave * 32 + row < Tn) *reinterpret_cast<uint4*>(slab + c + 16 * i * Tp + slab_l) = make_uint4(0u, 0u, 0u, 0u);
    }
  }

  // ---- dK, dV rows: accumulator = [d rows (registers)][key (lane)]; the swaps run with every lane active, the stores are predicated ----
  uint4 pk[5], pv[5];
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      pk[2 * t2 + m] = acc_piece(dk[t2], m, p.scale_a);
      pv[2 * t2 + m] = acc_piece(dv[t2], m, keep_scale);
    }
  pk[4] = acc_piece(dkb, 0, p.scale_b);
  pv[4] = acc_piece(dvb, 0, keep_scale);
  if (mykey < Tn) {
    T* DKa = reinterpret_cast<T*>(p.dk_a) + (row0 + mykey) * p.ld_da + h * DA;
    T* DVa = reinterpret_cast<T*>(p.dv_a) + (row0 + mykey) * p.ld_da + h * DA;
    T* DKb = reinterpret_cast<T*>(p.dk_b) + (row0 + mykey) * p.ld_db + h * DB;
    T* DVb = reinterpret_cast<T*>(p.dv_b) + (row0 + mykey) * p.ld_db + h * DB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<uint4*>(DKa + 16 * i + 8 * half) = pk[i];
      *reinterpret_cast<uint4*>(DVa + 16 * i + 8 * half) = pv[i];
    }
    *reinterpret_cast<uint4*>(DKb + 8 * half) = pk[4];
    *reinterpret_cast<uint4*>(DVb + 8 * half) = pv[4];
  }
}

// ================================================================================================
// 3. dQ_a[q, :] = scale_a sum_key dS[q, key] K_a[key, :], dQ_b likewise with K_b, from the dS^T slab (key-major [B, nh, T, Tp]).
// Workgroup = 128 queries (lane = query: dQ^T[d, q] = K^T[d, key] . dS^T[key, q]), streaming 32-key tiles: the slab block
// [32 keys][128 q] (256-byte rows, source slots permuted by (row & 3) << 2), the K_a rows [32][128 B] (slot ^ bitrev3(row >> 1)) and
// the K_b rows [32][32 B] (halves of rows 16..31 swapped) arrive by LDS-DMA into a ring of three; every operand is read with the
// hardware transpose read.  K rows past T come from a zero line (the slab rows read beside them are clamped to T - 1: finite x 0).
// The same sums in the same order as attn_dq_from_ds_kernel<96> (k-chunks of 16 keys, ascending).
// ================================================================================================
constexpr int DQ_O_S = 0, DQ_O_KA = 8192, DQ_O_KB = 12288, DQ_BUF = 13312;

__global__ __launch_bounds__(256, 2) void attn2_dq_pipe_kernel(Attn2BwdParams p) {
  typedef bf16_t T;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Tn = p.T, Tp = p.Tp;
  const int nqb = (Tn + 127) / 128;
  const int u = xcd_unit();
  const int qb = u % nqb, bh = u / nqb, h = bh % p.nh, b = bh / p.nh;
  const int q0 = qb * 128, myq = q0 + wave * 32 + l31;
  const int64_t row0 = (int64_t)b * Tn;
  const T* DS = reinterpret_cast<const T*>(p.slab) + (int64_t)bh * Tn * (int64_t)Tp;
  const T* Ka = reinterpret_cast<const T*>(p.k_a) + row0 * p.ld_a + h * DA;
  const T* Kb = reinterpret_cast<const T*>(p.k_b) + row0 * p.ld_b + h * DB;
  const int nt = (Tn + 31) / 32;
  const uint32_t lds0 = lds_addr(smem);
  const uint32_t lds2 = (uint32_t)(Tp * 2), ldk2 = (uint32_t)(p.ld_a * 2), ldb2 = (uint32_t)(p.ld_b * 2);
  // DMA: wave w sends slab pieces 2 w, 2 w + 1 (four key rows each) and K_a piece w (eight key rows); wave 0 the whole K_b tile
  const int srow0 = 8 * wave + (lane >> 4), krow = 8 * wave + (lane >> 3), brow = lane >> 1;
  const int scl = Tp * 2 - 16;                                   // (a query block may pass the padded row end: clamp; those rows are not stored)
  const uint32_t sc0 = (uint32_t)min(q0 * 2 + (((lane & 15) ^ ((srow0 & 3) << 2)) << 4), scl);
  const uint32_t sc1 = (uint32_t)min(q0 * 2 + (((lane & 15) ^ (((srow0 + 4) & 3) << 2)) << 4), scl);
  const uint32_t kcol = (uint32_t)(((lane & 7) ^ row128_slot_swz(krow)) << 4);
  const uint32_t bcol = (uint32_t)(((lane & 1) ^ (brow >> 4)) << 4);
  const char* ns = reinterpret_cast<const char*>(DS);
  const char* nk = reinterpret_cast<const char*>(Ka);
  const char* nkb = reinterpret_cast<const char*>(Kb);
  int nk0 = 0;
  auto dma_tile = [&](auto buf_c) {
    const int buf = buf_c;
    const uint32_t dst = lds0 + buf * DQ_BUF;
    const int lim = Tn - 1 - nk0;
    lds_dma_1k_s<0>((uint32_t)min(srow0, lim) * lds2 + sc0, ns, dst + DQ_O_S + wave * 2048);
    lds_dma_1k_s<0>((uint32_t)min(srow0 + 4, lim) * lds2 + sc1, ns, dst + DQ_O_S + wave * 2048 + 1024);
    if (lim >= 31) {
      lds_dma_1k_s<0>((uint32_t)krow * ldk2 + kcol, nk, dst + DQ_O_KA + wave * 1024);
      if (wave == 0) lds_dma_1k_s<0>((uint32_t)brow * ldb2 + bcol, nkb, dst + DQ_O_KB);
    } else {                                                      // the last tile: K rows past T read the zero line
      const char* src = krow <= lim ? nk + (uint32_t)krow * ldk2 + kcol : reinterpret_cast<const char*>(g_zero_line2) + (lane & 7) * 16;
      lds_dma_1k<0>(src, dst + DQ_O_KA + wave * 1024);
      if (wave == 0) {
        const char* sb = brow <= lim ? nkb + (uint32_t)brow * ldb2 + bcol : reinterpret_cast<const char*>(g_zero_line2) + (lane & 1) * 16;
        lds_dma_1k<0>(sb, dst + DQ_O_KB);
      }
    }
    ns += (int64_t)32 * lds2; nk += (int64_t)32 * ldk2; nkb += (int64_t)32 * ldb2; nk0 += 32;
  };
  // transpose-read addresses: [4 key rows][16 columns] blocks; keys 16 kk + 8 half + {0..3} and + 4
  const int li = lane & 15, lj = (lane >> 4) & 1;
  int aA[2], aK[2][2], aKb[2];
#pragma unroll
  for (int w4 = 0; w4 < 2; ++w4) {
    const int row = 8 * half + 4 * w4 + (li >> 2);
    aA[w4] = DQ_O_S + row * 256 + (((4 * wave + 2 * lj + ((li & 3) >> 1)) ^ ((row & 3) << 2)) << 4) + ((li & 1) << 3);
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
      aK[t2][w4] = DQ_O_KA + row * 128 + (((4 * t2 + 2 * lj + ((li & 3) >> 1)) ^ row128_slot_swz(row)) << 4) + ((li & 1) << 3);
    aKb[w4] = (row ^ (4 * lj)) * 32 + ((li & 3) << 3);           // (lj = 1, the d rows that do not exist: the other four key rows); (^ (kk << 4)) + 512 kk
  }
  f32x16_t acc[2], accb;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; accb[r] = 0.f; }

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  dma_tile(I0{});
  if (nt > 1) dma_tile(I1{});
  auto tile = [&](auto cur_c, int t) {
    const int cur = cur_c, nxt = cur + 1 == 3 ? 0 : cur + 1, nn = nxt + 1 == 3 ? 0 : nxt + 1;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 2 < nt) dma_tile(nn);
    const char* buf = smem + cur * DQ_BUF;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const uint2 b0 = tr64(buf + aA[0] + 4096 * kk), b1 = tr64(buf + aA[1] + 4096 * kk);
      Frag<T> bf;                                                 // dS^T[key, q]: this lane's query, keys 16 kk + 8 half + 0..7
      bf.v = make_uint4(b0.x, b0.y, b1.x, b1.y);
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const uint2 a0 = tr64(buf + aK[t2][0] + 2048 * kk), a1 = tr64(buf + aK[t2][1] + 2048 * kk);
        Frag<T> af;                                               // K_a^T[d, key]
        af.v = make_uint4(a0.x, a0.y, a1.x, a1.y);
        mma_step(af, bf, acc[t2]);
      }
      const uint2 c0 = tr64(buf + DQ_O_KB + 512 * kk + (aKb[0] ^ (kk << 4))), c1 = tr64(buf + DQ_O_KB + 512 * kk + (aKb[1] ^ (kk << 4)));
      Frag<T> af;                                                 // K_b^T[d, key]; d rows 16 .. 31: zero
      af.v = lj ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(c0.x, c0.y, c1.x, c1.y);
      mma_step(af, bf, accb);
    }
  };
  {
    int t = 0;
    for (; t + 3 <= nt; t += 3) { tile(I0{}, t); tile(I1{}, t + 1); tile(I2{}, t + 2); }
    if (t < nt) tile(I0{}, t);
    if (t + 1 < nt) tile(I1{}, t + 1);
  }
  uint4 pa[4];
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int m = 0; m < 2; ++m) pa[2 * t2 + m] = acc_piece(acc[t2], m, p.scale_a);
  const uint4 pb = acc_piece(accb, 0, p.scale_b);
  if (myq < Tn) {
    T* da = reinterpret_cast<T*>(p.dq_a) + (row0 + myq) * p.ld_da + h * DA;
    T* db = reinterpret_cast<T*>(p.dq_b) + (row0 + myq) * p.ld_db + h * DB;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(da + 16 * i + 8 * half) = pa[i];
    *reinterpret_cast<uint4*>(db + 8 * half) = pb;
  }
}

// the workspace: delta, then (256-byte aligned) the slab
inline int64_t ws_slab_offset(int B, int nh, int T) { return ((int64_t)B * nh * T * 4 + 255) / 256 * 256; }

}  // namespace
}  // namespace peneo
using namespace peneo;

extern "C" size_t peneo_attn2_bwd_workspace_bytes(int B, int nh, int T) {
  if (B < 1 || nh < 1 || T < 1) return 0;
  return (size_t)(ws_slab_offset(B, nh, T) + (int64_t)B * nh * T * peneo_attn_padded_len(T) * 2);
}

extern "C" int peneo_attn2_bwd(int dtype, const void* q_a, const void* k_a, const void* v_a, int64_t ld_a, const void* q_b,
                               const void* k_b, const void* v_b, int64_t ld_b, const void* out_a, const void* d_out_a,
                               int64_t ld_out_a, const void* out_b, const void* d_out_b, int64_t ld_out_b, const float* lse, int B,
                               int nh, int T, int d_a, int d_b, float scale_a, float scale_b, const float* key_bias, void* dq_a,
                               void* dk_a, void* dv_a, int64_t ld_da, void* dq_b, void* dk_b, void* dv_b, int64_t ld_db,
                               void* workspace, float drop_p, const uint32_t* drop_words, peneo_stream_t stream) {
  PENEO_REQUIRE(peneo_attn2_supported(dtype, d_a, d_b), "peneo_attn2_bwd: dtype %d with head dims %d + %d is not supported (bf16, 64 + 16)",
                dtype, d_a, d_b);
  PENEO_REQUIRE(B > 0 && nh > 0 && T > 0, "peneo_attn2_bwd: bad sizes (B %d, nh %d, T %d)", B, nh, T);
  PENEO_REQUIRE(q_a && k_a && v_a && q_b && k_b && v_b && out_a && d_out_a && out_b && d_out_b && lse,
                "peneo_attn2_bwd: null operand");
  PENEO_REQUIRE(dq_a && dk_a && dv_a && dq_b && dk_b && dv_b, "peneo_attn2_bwd: null output");
  PENEO_REQUIRE(workspace, "peneo_attn2_bwd: null workspace (peneo_attn2_bwd_workspace_bytes)");
  auto al = [](const void* q, uintptr_t m) { return (reinterpret_cast<uintptr_t>(q) & m) == 0; };
  PENEO_REQUIRE(al(q_a, 15) && al(k_a, 15) && al(v_a, 15) && al(q_b, 15) && al(k_b, 15) && al(v_b, 15) && al(out_a, 15) &&
                al(d_out_a, 15) && al(out_b, 15) && al(d_out_b, 15) && al(dq_a, 15) && al(dk_a, 15) && al(dv_a, 15) && al(dq_b, 15) &&
                al(dk_b, 15) && al(dv_b, 15) && al(workspace, 15),
                "peneo_attn2_bwd: operands, outputs and the workspace must be 16-byte aligned");
  PENEO_REQUIRE(al(key_bias, 3) && al(lse, 3), "peneo_attn2_bwd: key_bias and lse must be 4-byte aligned");
  PENEO_REQUIRE(ld_a >= (int64_t)nh * DA && ld_out_a >= (int64_t)nh * DA && ld_da >= (int64_t)nh * DA && ld_b >= (int64_t)nh * DB &&
                ld_out_b >= (int64_t)nh * DB && ld_db >= (int64_t)nh * DB, "peneo_attn2_bwd: leading dims too small");
  PENEO_REQUIRE((ld_a * 2) % 16 == 0 && (ld_b * 2) % 16 == 0 && (ld_out_a * 2) % 16 == 0 && (ld_out_b * 2) % 16 == 0 &&
                (ld_da * 2) % 16 == 0 && (ld_db * 2) % 16 == 0, "peneo_attn2_bwd: row strides must be multiples of 16 bytes");
  // the kernels' per-lane DMA offsets (a row of a tile, a delta index, a slab row) are 32-bit byte offsets
  const int Tp = peneo_attn_padded_len(T);
  PENEO_REQUIRE(ld_a * 2 * TQ < (1ll << 31) && ld_b * 2 * TQ < (1ll << 31) && ld_out_a * 2 * TQ < (1ll << 31) &&
                ld_out_b * 2 * TQ < (1ll << 31) && (int64_t)Tp * 2 * TQ < (1ll << 31) && (int64_t)T * 4 < (1ll << 31),
                "peneo_attn2_bwd: row strides or T beyond the kernels' 32-bit lane offsets");
  PENEO_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "peneo_attn2_bwd: drop_p out of range");
  PENEO_REQUIRE(drop_p == 0.f || (drop_words && al(drop_words, 3)),
                "peneo_attn2_bwd: drop_p > 0 needs the keep words the forward used (peneo_attn_drop_words)");
  const int64_t units = (int64_t)((T + WK - 1) / WK) * nh * B;
  const int64_t rows = (int64_t)B * nh * T;
  PENEO_REQUIRE(units < (1ll << 31) && (rows * 8 + 255) / 256 < (1ll << 31), "peneo_attn2_bwd: too many workgroups");
  Attn2BwdParams p = {};
  p.q_a = q_a; p.k_a = k_a; p.v_a = v_a; p.ld_a = ld_a; p.q_b = q_b; p.k_b = k_b; p.v_b = v_b; p.ld_b = ld_b;
  p.out_a = out_a; p.d_out_a = d_out_a; p.ld_out_a = ld_out_a; p.out_b = out_b; p.d_out_b = d_out_b; p.ld_out_b = ld_out_b;
  p.lse = lse; p.B = B; p.nh = nh; p.T = T; p.Tp = Tp; p.scale_a = scale_a; p.scale_b = scale_b; p.key_bias = key_bias;
  p.dq_a = dq_a; p.dk_a = dk_a; p.dv_a = dv_a; p.ld_da = ld_da; p.dq_b = dq_b; p.dk_b = dk_b; p.dv_b = dv_b; p.ld_db = ld_db;
  p.delta = reinterpret_cast<float*>(workspace);
  p.slab = reinterpret_cast<char*>(workspace) + ws_slab_offset(B, nh, T);
  p.keep_scale = pair_drop_scale_host(drop_p); p.words = drop_words;
  peneo_attn_drop_words_dims(T, &p.nqb, &p.Tk);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(attn2_delta_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, st, p);
  int rc = check_launch("peneo_attn2_bwd(delta)");
  if (rc) return rc;
  if (drop_p > 0.f) hipLaunchKernelGGL(attn2_bwd_pipe_kernel<true>, dim3((unsigned)units), dim3(256), LDS_BYTES, st, p);
  else hipLaunchKernelGGL(attn2_bwd_pipe_kernel<false>, dim3((unsigned)units), dim3(256), LDS_BYTES, st, p);
  rc = check_launch("peneo_attn2_bwd(dk dv)");
  if (rc) return rc;
  hipLaunchKernelGGL(attn2_dq_pipe_kernel, dim3((unsigned)units), dim3(256), 3 * DQ_BUF, st, p);
  return check_launch("peneo_attn2_bwd(dq)");
}
