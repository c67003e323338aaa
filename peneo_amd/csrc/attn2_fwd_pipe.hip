// Two-stream attention forward, pipelined (bf16, head dims 64 + 16: LiLT's text and layout streams).  One shared softmax over
//
//     scores[b, h, i, j] = (scale_a q_a) . k_a + (scale_b q_b) . k_b + key_bias[b, j]        out_a = P v_a,  out_b = P v_b
//
// which is what the concat path computes at head dim 80 (peneo_head_concat x 2 -> attn_fwd_kernel<bf16, 96> -> peneo_head_split),
// with the same arithmetic in the same order and the same outputs bit for bit, but without the three copies: the operands are read
// where the QKV GEMMs left them and the two context streams are written where the output projections read them.  The skeleton is
// attn_fwd_pipe_kernel's (attn_fwd_pipe.hip):
//
//   * workgroup = 128 queries (lane = query; Q fragments, scaled and rounded to bf16 as peneo_head_concat writes them, and the
//     O^T accumulators in registers) streaming 32-key tiles by LDS-DMA into a ring of three buffers (request for tile t + 2 at the
//     top of iteration t), ONE s_barrier per tile, S^T of tile t + 1 computed at the end of iteration t;
//   * a tile's buffer: K_a [32][128 B] and V_a [32][128 B] (one 1 KiB piece per wave each, source slots permuted by
//     slot ^ bitrev3(row >> 1) as in attn_fwd_pipe), K_b [32][32 B] (wave 0) and V_b [32][32 B] (wave 1), each ONE 1 KiB piece
//     whose two 16-byte halves of a row are swapped for rows 16..31 (the four 16-lane groups of the b128 fragment read - key row
//     = lane & 31, half = lane >> 5 - then each cover the 256-byte bank row once; the transpose reads of V_b take 128 contiguous
//     bytes per 32-lane half either way), and the tile's key-bias floats (one dword DMA of wave 2; 64 lanes = 256 B, the first
//     32 are the tile's).  10.25 KiB per buffer, no bias block;
//   * S^T: five k-steps, four over the text dims then one over the 16 layout dims (k-step 5 of the DP = 96 kernel multiplies
//     zeros); P.V: two text d-tiles and one layout tile whose upper 16 rows are zero.  ds_read_b64_tr_b16 wants EXEC all ones: the
//     16-lane groups of those pad rows read the OTHER eight key rows of the step (a valid address; the wave's read then covers
//     512 contiguous bytes) and zero their fragment afterwards;
//   * keys past T: K / V rows are clamped to T - 1 and the ragged last tile masks its scores itself; nothing is read from the
//     padding columns [T, Tp) of key_bias beyond what the clamp allows (index <= T - 1);
//   * O rows leave as 16-byte pieces straight from the accumulator layout (v_permlane32_swap pairs), no LDS round trip;
//   * attention dropout (peneo_attn2_fwd_dropout, the DROP instantiation): the keep words of peneo_attn_drop_words arrive as in
//     attn_fwd_pipe_kernel<true> - every wave's 64 keep-word slots of the tile for ITS 32 queries by one dword DMA (1 KiB more per
//     buffer), register r's 64-lane mask by two v_readlane, one v_cndmask per element - applied to P after the row sum (lse is the
//     pre-dropout log-sum-exp), both value streams under the same mask, 1 / (1 - p) once on the accumulators.
// Nothing here waits on another workgroup.
#include "common.h"
#include "attn_pipe.h"

namespace peneo {
namespace {

struct Attn2Params {
  const void* q_a; const void* k_a; const void* v_a; int64_t ld_a;
  const void* q_b; const void* k_b; const void* v_b; int64_t ld_b;
  int B, nh, T, Tp; float scale_a, scale_b;
  const float* key_bias;
  void* out_a; int64_t ld_out_a; void* out_b; int64_t ld_out_b; float* lse;
  float keep_scale; const uint32_t* words; int nqb, Tk;           // dropout keep bits (peneo_attn_drop_words) or NULL
};

constexpr int DA = 64, DB = 16;   // head dims of the two streams
constexpr int TK = 32;            // keys per tile
constexpr int WQ = 128;           // queries per workgroup (4 waves x 32)
// a tile's buffer: K_a [32][128 B], V_a [32][128 B], K_b [32][32 B], V_b [32][32 B], key bias [64] fp32 (the first 32 are the tile's)
// with dropout: + the keep words [4 query blocks][64 slots] (attn_fwd_pipe.hip)
constexpr int O_KA = 0, O_VA = 4096, O_KB = 8192, O_VB = 9216, O_BIAS = 10240, O_WORDS = 10496;
constexpr int NBUF = 3;
constexpr int buf_bytes(bool drop) { return drop ? O_WORDS + 1024 : O_WORDS; }

template <bool DROP>
__global__ __launch_bounds__(256, 2) void attn2_fwd_pipe_kernel(Attn2Params p) {
  typedef bf16_t T;
  constexpr int BUF = buf_bytes(DROP);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Tn = p.T;
  // unit order: the query blocks of one (document, head) run on ONE XCD (they stream the same K / V rows through its L2)
  const int nqb = (Tn + WQ - 1) / WQ;
  const int u = xcd_unit();
  const int qb = u % nqb, bh = u / nqb, h = bh % p.nh, b = bh / p.nh;
  const int q0 = qb * WQ;
  const int myq = q0 + wave * 32 + l31;
  const int64_t row0 = (int64_t)b * Tn;
  const T* Qa = reinterpret_cast<const T*>(p.q_a) + row0 * p.ld_a + h * DA;
  const T* Ka = reinterpret_cast<const T*>(p.k_a) + row0 * p.ld_a + h * DA;
  const T* Va = reinterpret_cast<const T*>(p.v_a) + row0 * p.ld_a + h * DA;
  const T* Qb = reinterpret_cast<const T*>(p.q_b) + row0 * p.ld_b + h * DB;
  const T* Kb = reinterpret_cast<const T*>(p.k_b) + row0 * p.ld_b + h * DB;
  const T* Vb = reinterpret_cast<const T*>(p.v_b) + row0 * p.ld_b + h * DB;
  const bool has_kb = p.key_bias != nullptr;
  const int nt = (Tn + TK - 1) / TK;

  // ---- Q fragments of this lane's query (B operands of S^T): four text k-steps, one layout k-step ----
  Frag<T> qf[5];
  {
    const bool ok = myq < Tn;
    const T* qr = Qa + (int64_t)(ok ? myq : 0) * p.ld_a + 8 * half;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks].v = scaled8(qr + 16 * ks, p.scale_a, ok);
    qf[4].v = scaled8(Qb + (int64_t)(ok ? myq : 0) * p.ld_b + 8 * half, p.scale_b, ok);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // from here on the vm counter holds the DMA pieces only
#pragma unroll
  for (int ks = 0; ks < 5; ++ks) asm volatile("" : "+v"(qf[ks].v.x), "+v"(qf[ks].v.y), "+v"(qf[ks].v.z), "+v"(qf[ks].v.w));

  // ---- DMA: wave w sends K_a piece w and V_a piece w (rows 8 w .. 8 w + 7 of the tile); wave 0 the whole K_b tile, wave 1 the
  //      whole V_b tile (lane: row lane / 2, half lane & 1), wave 2 the key-bias floats ----
  const uint32_t lds0 = lds_addr(smem);
  const uint32_t lda2 = (uint32_t)(p.ld_a * 2), ldb2 = (uint32_t)(p.ld_b * 2);
  const int krow = 8 * wave + (lane >> 3);
  const uint32_t kcol = (uint32_t)(((lane & 7) ^ row128_slot_swz(krow)) << 4);
  const int brow = lane >> 1;
  const uint32_t bcol = (uint32_t)(((lane & 1) ^ (brow >> 4)) << 4);
  const char* nka = reinterpret_cast<const char*>(Ka);
  const char* nva = reinterpret_cast<const char*>(Va);
  const char* nb = reinterpret_cast<const char*>(wave == 0 ? Kb : Vb);     // (waves 0 and 1 only)
  const char* nkb = reinterpret_cast<const char*>(has_kb ? p.key_bias + (int64_t)b * p.Tp : nullptr);
  // with dropout every wave also sends the 64 keep-word slots that start at the tile's first key for ITS 32 queries
  const char* nw = DROP ? reinterpret_cast<const char*>(p.words + ((int64_t)bh * p.nqb + (qb * 4 + wave)) * (int64_t)p.Tk) : nullptr;
  int nk0 = 0;                                       // first key of the next tile to request
  auto dma_tile = [&](auto buf_c) {
    const int buf = buf_c;
    const uint32_t dst = lds0 + buf * BUF;
    const int last = Tn - 1 - nk0;                   // (key rows past T: clamped; the ragged tile masks their scores)
    const uint32_t ko = (uint32_t)min(krow, last) * lda2 + kcol;
    lds_dma_1k_s<0>(ko, nka, dst + O_KA + wave * 1024);
    lds_dma_1k_s<0>(ko, nva, dst + O_VA + wave * 1024);
    if (wave < 2) lds_dma_1k_s<0>((uint32_t)min(brow, last) * ldb2 + bcol, nb, dst + (wave == 0 ? O_KB : O_VB));
    else if (wave == 2 && has_kb) dma4_s((uint32_t)min(nk0 + lane, Tn - 1) * 4u, nkb, dst + O_BIAS);
    if (DROP) dma4_s((uint32_t)min(nk0 + lane, p.Tk - 1) * 4u, nw, dst + O_WORDS + wave * 256);
    nka += (int64_t)TK * lda2; nva += (int64_t)TK * lda2; nb += (int64_t)TK * ldb2; nk0 += TK;
  };

  // ---- LDS read addresses (lane constants relative to a buffer) ----
  const int aS0 = l31 * 128 + ((half ^ row128_slot_swz(l31)) << 4);           // K_a fragment of k-step ks: ^ (ks << 5)
  const int aSb = O_KB + l31 * 32 + ((half ^ (l31 >> 4)) << 4);          // K_b fragment
  const int li = lane & 15, lj = (lane >> 4) & 1;
  int aT[2][2];                                                          // transpose reads of the V_a tile: [d tile][rows +0 / +8]; + 2048 kh
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int w8 = 0; w8 < 2; ++w8) {
      const int row = 4 * half + (li >> 2) + 8 * w8;
      const int slot = 4 * t2 + 2 * lj + ((li & 3) >> 1);
      aT[t2][w8] = row * 128 + ((slot ^ row128_slot_swz(row)) << 4) + ((li & 1) << 3);
    }
  int aTb[2];                                                            // of the V_b tile: [rows +0 / +8]; (^ (kh << 4)) + 512 kh
#pragma unroll
  for (int w8 = 0; w8 < 2; ++w8) {
    const int row = (4 * half + (li >> 2) + 8 * w8) ^ (8 * lj);          // (lj = 1: the pad rows' groups read the other eight key rows)
    aTb[w8] = O_VB + row * 32 + ((li & 3) << 3);
  }
  const int aKb = O_BIAS + 16 * half;                                    // key bias of registers 4 g .. 4 g + 3: + 32 g
  const int aW = O_WORDS + wave * 256 + lane * 4;                        // lane L: keep word of key slot L of the tile

  f32x16_t o[3], s;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; o[2][r] = 0.f; s[r] = 0.f; }
  float m_run = kMasked, l_run = 0.f;

  auto s_tile = [&](const char* buf) {               // S^T[key, q] of a tile: A = K rows, B = Q fragments
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      Frag<T> a;
      a.v = *reinterpret_cast<const uint4*>(buf + O_KA + (aS0 ^ (ks << 5)));
      mma_step(a, qf[ks], acc);
    }
    Frag<T> a;
    a.v = *reinterpret_cast<const uint4*>(buf + aSb);
    mma_step(a, qf[4], acc);
    return acc;
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  if (!has_kb && tid < 3 * TK) *reinterpret_cast<float*>(smem + (tid >> 5) * BUF + O_BIAS + 4 * l31) = 0.f;   // no key bias: zeros, once
  dma_tile(I0{});
  if (nt > 1) dma_tile(I1{});
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  s = s_tile(smem);

  auto tile = [&](auto cur_c, int t) {
    const int cur = cur_c, nxt = cur + 1 == NBUF ? 0 : cur + 1, nn = nxt + 1 == NBUF ? 0 : nxt + 1;
    if (t > 0) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the next tile has landed
      __builtin_amdgcn_s_barrier();
    }
    if (t + 2 < nt) dma_tile(nn);
    const char* buf = smem + cur * BUF;
    uint32_t cw = 0u;
    if constexpr (DROP) cw = *reinterpret_cast<const uint32_t*>(buf + aW);
    // scores (natural units) and the block's row maximum  (attention.hip: the `block` lambda of attn_fwd_kernel at scale 1, same order)
    float mt = kMasked;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 kb = *reinterpret_cast<const float4*>(buf + aKb + 32 * g);
      const float bb[4] = {kb.x, kb.y, kb.z, kb.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = fmaf(s[4 * g + e], 1.0f, bb[e]);
        s[4 * g + e] = v;
        mt = fmaxf(mt, v);
      }
    }
    // keys past T (the ragged last tile only; a wave-uniform branch taken once per launch)
    if (t + 1 == nt && (Tn & (TK - 1)) != 0) {
      mt = kMasked;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (t * TK + 8 * g + 4 * half + e >= Tn) s[4 * g + e] = kMasked;
          mt = fmaxf(mt, s[4 * g + e]);
        }
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float m_new = (mt > m_run + kRescaleTau) ? mt : m_run;
    if (__builtin_amdgcn_ballot_w64(m_new != m_run)) {   // rare after the first tiles (wave-uniform branch)
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * kLog2e);
      l_run *= alpha;
      m_run = m_new;
#pragma unroll
      for (int t2 = 0; t2 < 3; ++t2)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t2][r] *= alpha;
    }
    const float nm = -m_run * kLog2e;
    float ls = 0.f;
    if constexpr (DROP) {                              // (the sum is taken before the mask: lse is the pre-dropout log-sum-exp)
      auto soft = [&](auto r_c) {
        constexpr int r = decltype(r_c)::value;
        const float e = __builtin_amdgcn_exp2f(fmaf(s[r], kLog2e, nm));
        ls += e;
        s[r] = mask_keep(e, lane_words_mask(cw, 2 * r));
      };
      soft(std::integral_constant<int, 0>{}); soft(std::integral_constant<int, 1>{});
      soft(std::integral_constant<int, 2>{}); soft(std::integral_constant<int, 3>{});
      soft(std::integral_constant<int, 4>{}); soft(std::integral_constant<int, 5>{});
      soft(std::integral_constant<int, 6>{}); soft(std::integral_constant<int, 7>{});
      soft(std::integral_constant<int, 8>{}); soft(std::integral_constant<int, 9>{});
      soft(std::integral_constant<int, 10>{}); soft(std::integral_constant<int, 11>{});
      soft(std::integral_constant<int, 12>{}); soft(std::integral_constant<int, 13>{});
      soft(std::integral_constant<int, 14>{}); soft(std::integral_constant<int, 15>{});
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(fmaf(s[r], kLog2e, nm));
        ls += e;
        s[r] = e;
      }
    }
    ls += __shfl_xor(ls, 32, 64);
    l_run += ls;
    // O^T[d, q] += V^T[d, key] . P^T[key, q]
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      float pv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) pv[e] = s[8 * kh + e];
      const Frag<T> pf = pack_frag8<T>(pv);
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const uint2 a0 = tr64(buf + O_VA + 2048 * kh + aT[t2][0]), a1 = tr64(buf + O_VA + 2048 * kh + aT[t2][1]);
        Frag<T> vf;
        vf.v = make_uint4(a0.x, a0.y, a1.x, a1.y);
        mma_step(vf, pf, o[t2]);
      }
      const uint2 b0 = tr64(buf + 512 * kh + (aTb[0] ^ (kh << 4))), b1 = tr64(buf + 512 * kh + (aTb[1] ^ (kh << 4)));
      Frag<T> vf;
      vf.v = lj ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(b0.x, b0.y, b1.x, b1.y);   // d rows 16 .. 31 of the layout tile: zero
      mma_step(vf, pf, o[2]);
    }
    if (t + 1 < nt) s = s_tile(smem + nxt * BUF);
  };
  {
    int t = 0;
    for (; t + 3 <= nt; t += 3) { tile(I0{}, t); tile(I1{}, t + 1); tile(I2{}, t + 2); }
    if (t < nt) tile(I0{}, t);
    if (t + 1 < nt) tile(I1{}, t + 1);
  }

  // ---- normalise; O rows: accumulator = [d rows (registers)][query (lane)], two groups + a v_permlane32_swap = 16 bytes per lane ----
  const bool any = m_run > 0.5f * kMasked;
  const float inv = (any && l_run > 0.f) ? (DROP ? p.keep_scale : 1.0f) / l_run : 0.f;   // (1 / (1 - p) once, on the accumulators)
  if (half == 0 && myq < Tn && p.lse) p.lse[(int64_t)bh * Tn + myq] = any ? fmaf(m_run, kLog2e, log2f(l_run)) : kMasked;   // log2 units
  // (a row whose keys are all masked: zeros - with the running maximum at -1e30 its P can be inf and its accumulators inf - inf,
  // attention.hip: `any`)
  auto nz = [&](float x) { return any ? x * inv : 0.f; };
  // acc_piece (attn_pipe.h) with nz in place of the multiply; written out here: through acc_piece the compiler schedules this
  // epilogue differently
  auto piece = [&](const f32x16_t& a, int m) {       // d rows 16 m + 8 half .. + 7 of an accumulator tile, as 8 bf16
    uint32_t ax = pack_bf16x2(nz(a[8 * m + 0]), nz(a[8 * m + 1])), ay = pack_bf16x2(nz(a[8 * m + 2]), nz(a[8 * m + 3]));
    uint32_t bx = pack_bf16x2(nz(a[8 * m + 4]), nz(a[8 * m + 5])), by = pack_bf16x2(nz(a[8 * m + 6]), nz(a[8 * m + 7]));
    const auto rx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
    const auto ry = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
    return make_uint4(rx[0], ry[0], rx[1], ry[1]);
  };
  // (the swaps run with every lane active; only the stores are predicated)
  uint4 pa[4];
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int m = 0; m < 2; ++m) pa[2 * t2 + m] = piece(o[t2], m);
  const uint4 pb = piece(o[2], 0);
  if (myq < Tn) {
    T* da = reinterpret_cast<T*>(p.out_a) + (row0 + myq) * p.ld_out_a + h * DA;
    T* db = reinterpret_cast<T*>(p.out_b) + (row0 + myq) * p.ld_out_b + h * DB;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(da + 16 * i + 8 * half) = pa[i];
    *reinterpret_cast<uint4*>(db + 8 * half) = pb;
  }
}

}  // namespace
}  // namespace peneo
using namespace peneo;

extern "C" int peneo_attn2_supported(int dtype, int d_a, int d_b) { return dtype == PENEO_BF16 && d_a == DA && d_b == DB ? 1 : 0; }

static int attn2_fwd_launch(const char* who, int dtype, const void* q_a, const void* k_a, const void* v_a, int64_t ld_a, const void* q_b,
                            const void* k_b, const void* v_b, int64_t ld_b, int B, int nh, int T, int d_a, int d_b, float scale_a,
                            float scale_b, const float* key_bias, void* out_a, int64_t ld_out_a, void* out_b, int64_t ld_out_b,
                            float* lse, float drop_p, const uint32_t* drop_words, peneo_stream_t stream) {
  PENEO_REQUIRE(peneo_attn2_supported(dtype, d_a, d_b), "%s: dtype %d with head dims %d + %d is not supported (bf16, 64 + 16)", who,
                dtype, d_a, d_b);
  PENEO_REQUIRE(B > 0 && nh > 0 && T > 0, "%s: bad sizes (B %d, nh %d, T %d)", who, B, nh, T);
  PENEO_REQUIRE(q_a && k_a && v_a && q_b && k_b && v_b && out_a && out_b, "%s: null operand or output", who);
  auto al = [](const void* q, uintptr_t m) { return (reinterpret_cast<uintptr_t>(q) & m) == 0; };
  PENEO_REQUIRE(al(q_a, 15) && al(k_a, 15) && al(v_a, 15) && al(q_b, 15) && al(k_b, 15) && al(v_b, 15) && al(out_a, 15) && al(out_b, 15),
                "%s: operands and outputs must be 16-byte aligned", who);
  PENEO_REQUIRE(al(key_bias, 3) && al(lse, 3), "%s: key_bias and lse must be 4-byte aligned", who);
  PENEO_REQUIRE(ld_a >= (int64_t)nh * DA && ld_out_a >= (int64_t)nh * DA && ld_b >= (int64_t)nh * DB && ld_out_b >= (int64_t)nh * DB,
                "%s: leading dims too small", who);
  PENEO_REQUIRE((ld_a * 2) % 16 == 0 && (ld_b * 2) % 16 == 0 && (ld_out_a * 2) % 16 == 0 && (ld_out_b * 2) % 16 == 0,
                "%s: row strides must be multiples of 16 bytes", who);
  // the kernel's per-lane DMA offsets (a key row of a tile, a key-bias index) are 32-bit byte offsets
  PENEO_REQUIRE(ld_a * 2 * TK < (1ll << 31) && ld_b * 2 * TK < (1ll << 31) && (int64_t)T * 4 < (1ll << 31),
                "%s: row strides or T beyond the kernel's 32-bit lane offsets", who);
  PENEO_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p out of range", who);
  PENEO_REQUIRE(drop_p == 0.f || (drop_words && al(drop_words, 3)), "%s: drop_p > 0 needs the keep words of peneo_attn_drop_words", who);
  const int64_t units = (int64_t)((T + WQ - 1) / WQ) * nh * B;
  PENEO_REQUIRE(units < (1ll << 31), "%s: too many workgroups", who);
  Attn2Params p = {};
  p.q_a = q_a; p.k_a = k_a; p.v_a = v_a; p.ld_a = ld_a; p.q_b = q_b; p.k_b = k_b; p.v_b = v_b; p.ld_b = ld_b;
  p.B = B; p.nh = nh; p.T = T; p.Tp = peneo_attn_padded_len(T); p.scale_a = scale_a; p.scale_b = scale_b; p.key_bias = key_bias;
  p.out_a = out_a; p.ld_out_a = ld_out_a; p.out_b = out_b; p.ld_out_b = ld_out_b; p.lse = lse;
  p.keep_scale = pair_drop_scale_host(drop_p); p.words = drop_words;
  peneo_attn_drop_words_dims(T, &p.nqb, &p.Tk);
  if (drop_p > 0.f) hipLaunchKernelGGL(attn2_fwd_pipe_kernel<true>, dim3((unsigned)units), dim3(256), NBUF * buf_bytes(true), (hipStream_t)stream, p);
  else hipLaunchKernelGGL(attn2_fwd_pipe_kernel<false>, dim3((unsigned)units), dim3(256), NBUF * buf_bytes(false), (hipStream_t)stream, p);
  return check_launch(who);
}

extern "C" int peneo_attn2_fwd(int dtype, const void* q_a, const void* k_a, const void* v_a, int64_t ld_a, const void* q_b,
                               const void* k_b, const void* v_b, int64_t ld_b, int B, int nh, int T, int d_a, int d_b, float scale_a,
                               float scale_b, const float* key_bias, void* out_a, int64_t ld_out_a, void* out_b, int64_t ld_out_b,
                               float* lse, peneo_stream_t stream) {
  return attn2_fwd_launch("peneo_attn2_fwd", dtype, q_a, k_a, v_a, ld_a, q_b, k_b, v_b, ld_b, B, nh, T, d_a, d_b, scale_a, scale_b, key_bias,
                          out_a, ld_out_a, out_b, ld_out_b, lse, 0.f, nullptr, stream);
}

extern "C" int peneo_attn2_fwd_dropout(int dtype, const void* q_a, const void* k_a, const void* v_a, int64_t ld_a, const void* q_b,
                                       const void* k_b, const void* v_b, int64_t ld_b, int B, int nh, int T, int d_a, int d_b,
                                       float scale_a, float scale_b, const float* key_bias, void* out_a, int64_t ld_out_a, void* out_b,
                                       int64_t ld_out_b, float* lse, float drop_p, const uint32_t* drop_words, peneo_stream_t stream) {
  return attn2_fwd_launch("peneo_attn2_fwd_dropout", dtype, q_a, k_a, v_a, ld_a, q_b, k_b, v_b, ld_b, B, nh, T, d_a, d_b, scale_a, scale_b,
                          key_bias, out_a, ld_out_a, out_b, ld_out_b, lse, drop_p, drop_words, stream);
}
