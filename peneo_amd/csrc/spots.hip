// K14, batched: every score map and label map of a batch -> ordered spot records, in two stream-ordered launches.
//
// peneo_spots_compact (pair_heads.hip) walks ONE [P, C] map with ONE workgroup: at N = 511 that is 128 dependent rounds of load,
// ballot and three barriers, and a batch of 8 documents x 5 heads is 40 such launches with a host read of the count behind each.
// Here a (map, document) is cut into segments of SP_SEG = 1024 consecutive pairs and every segment is one workgroup of 256 threads
// (grid = segments x B x maps: 5120 workgroups at B = 8, N = 511, 5 maps):
//
//   count pass   segment s of (m, b) writes its number of spots to workspace[(m * B + b) * nseg + s];
//   write pass   segment s sums the counts of segments 0 .. s-1 of its (m, b) (its first slot), recomputes its tags and scores, and
//                stores its spots behind that base in increasing p; the last segment also writes counts[m][b] = the full sum.
//
// The order between the passes is the stream's: no workgroup waits for another one, nothing spins.  Reading the maps twice costs
// 2 x 58 MB at B = 8, N = 511 - microseconds of HBM time - and buys a write pass whose slots are known before it starts.
// Every loop is bounded by its arguments (4 rounds per segment, nseg / 256 steps of the prefix sum); nothing is written past
// min(count, max_spots) records of a (map, document), and nothing outside records / counts / the workspace.
#include "common.h"

namespace peneo {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / kWave;
constexpr int SP_ROUNDS = 4;
constexpr int SP_SEG = SP_THREADS * SP_ROUNDS;   // pairs per workgroup

struct SpotsBatchArgs {
  const void* maps[PENEO_MAX_HEADS];
  int classes[PENEO_MAX_HEADS];   // >= 2: fp32 logits [B, P, C]; 0: int64 labels [B, P]
};

static inline int64_t sp_num_segments(int64_t P) { return (P + SP_SEG - 1) / SP_SEG; }

// tag of pair `row` (= b * P + p) of one map; want_score: also its score
template <bool kScore>
__device__ __forceinline__ int sp_tag(const void* map, int C, int64_t row, float& score) {
  if (C == 0) {   // a spot iff the int64 value != 0 (tested before narrowing); tag = its low 32 bits, or 1 where those are all zero
    score = 1.f;
    const int64_t v = static_cast<const int64_t*>(map)[row];
    const int t = (int)v;
    return (v != 0 && t == 0) ? 1 : t;
  }
  const float* l = static_cast<const float*>(map) + row * C;
  float mx;
  const int tag = spot_argmax(l, C, mx);
  if (kScore) score = spot_score(l, C, mx);
  return tag;
}

__device__ __forceinline__ int sp_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(SP_THREADS) void spots_batch_count_kernel(SpotsBatchArgs a, int64_t P, int nseg, int32_t* segc) {
  __shared__ int wsum[SP_WAVES];
  const int seg = blockIdx.x, b = blockIdx.y, m = blockIdx.z, B = gridDim.y;
  const void* map = a.maps[m];
  const int C = a.classes[m];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int n = 0;
#pragma unroll
  for (int r = 0; r < SP_ROUNDS; ++r) {
    const int64_t p = (int64_t)seg * SP_SEG + r * SP_THREADS + threadIdx.x;
    float unused;
    const bool spot = p < P && sp_tag<false>(map, C, (int64_t)b * P + p, unused) != 0;
    n += __popcll(__ballot(spot));
  }
  if (lane == 0) wsum[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < SP_WAVES; ++w) tot += wsum[w];
    segc[((int64_t)m * B + b) * nseg + seg] = tot;
  }
}

__global__ __launch_bounds__(SP_THREADS) void spots_batch_write_kernel(SpotsBatchArgs a, int64_t P, int N, int nseg,
                                                                      const int32_t* segc, int4* records, int32_t* counts,
                                                                      int max_spots) {
  __shared__ int red[SP_WAVES];
  __shared__ int wsum[SP_ROUNDS][SP_WAVES];
  const int seg = blockIdx.x, b = blockIdx.y, m = blockIdx.z, B = gridDim.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t doc = (int64_t)m * B + b;
  const int32_t* sc = segc + doc * nseg;
  // first slot of this segment: the spots of the segments before it
  int before_seg = 0;
  for (int s = threadIdx.x; s < seg; s += SP_THREADS) before_seg += sc[s];
  before_seg = sp_wave_sum(before_seg);
  if (lane == 0) red[wave] = before_seg;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < SP_WAVES; ++w) base += red[w];
  if (seg == nseg - 1 && threadIdx.x == 0) counts[doc] = base + sc[seg];
  if (base >= max_spots) return;   // (the whole workgroup: base is uniform) nothing of this segment is stored

  const void* map = a.maps[m];
  const int C = a.classes[m];
  int tag[SP_ROUNDS];
  float score[SP_ROUNDS];
  int before[SP_ROUNDS];
#pragma unroll
  for (int r = 0; r < SP_ROUNDS; ++r) {
    const int64_t p = (int64_t)seg * SP_SEG + r * SP_THREADS + threadIdx.x;
    tag[r] = 0; score[r] = 0.f;
    if (p < P) tag[r] = sp_tag<true>(map, C, (int64_t)b * P + p, score[r]);
    const unsigned long long bal = __ballot(tag[r] != 0);
    before[r] = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[r][wave] = __popcll(bal);
  }
  __syncthreads();
  int4* rec = records + doc * max_spots;
#pragma unroll
  for (int r = 0; r < SP_ROUNDS; ++r) {
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SP_WAVES; ++w) { if (w < wave) woff += wsum[r][w]; tot += wsum[r][w]; }
    if (tag[r] != 0) {
      const int slot = base + woff + before[r];
      if (slot < max_spots) {
        int i, j;
        pair_decode((int64_t)seg * SP_SEG + r * SP_THREADS + threadIdx.x, N, i, j);
        rec[slot] = make_int4(i, j, tag[r], __float_as_int(score[r]));
      }
    }
    base += tot;
  }
}

static bool sp_shape_ok(int num_maps, int B, int N) {
  return num_maps >= 1 && num_maps <= PENEO_MAX_HEADS && B >= 1 && B <= 65535 && N >= 1 && N <= 65535;   // P < 2^31
}

}  // namespace peneo
using namespace peneo;

extern "C" size_t peneo_spots_compact_batch_workspace_bytes(int num_maps, int B, int N) {
  if (!sp_shape_ok(num_maps, B, N)) return 0;
  const int64_t P = (int64_t)N * (N + 1) / 2;
  return (((size_t)num_maps * B * sp_num_segments(P) * sizeof(int32_t)) + 255) & ~(size_t)255;
}

extern "C" int peneo_spots_compact_batch(const peneo_spots_batch_desc* desc, int B, int N, void* records, int32_t* counts,
                                         int max_spots, void* workspace, size_t workspace_bytes, peneo_stream_t stream) {
  PENEO_REQUIRE(desc && counts && max_spots >= 0 && (records || max_spots == 0), "peneo_spots_compact_batch: bad arguments");
  PENEO_REQUIRE(sp_shape_ok(desc->num_maps, B, N), "peneo_spots_compact_batch: num_maps, B or N out of range");
  PENEO_REQUIRE((reinterpret_cast<uintptr_t>(records) & 15) == 0, "peneo_spots_compact_batch: records must be 16-byte aligned");
  SpotsBatchArgs a = {};
  for (int m = 0; m < desc->num_maps; ++m) {
    PENEO_REQUIRE(desc->maps[m], "peneo_spots_compact_batch: map %d is NULL", m);
    PENEO_REQUIRE(desc->classes[m] == 0 || desc->classes[m] >= 2,
                  "peneo_spots_compact_batch: map %d has %d classes (0 = label map, >= 2 = logits)", m, desc->classes[m]);
    a.maps[m] = desc->maps[m];
    a.classes[m] = desc->classes[m];
  }
  const size_t need = peneo_spots_compact_batch_workspace_bytes(desc->num_maps, B, N);
  PENEO_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
                "peneo_spots_compact_batch: workspace of %zu bytes needed (4-byte aligned), got %zu", need, workspace_bytes);
  const int64_t P = (int64_t)N * (N + 1) / 2;
  const int nseg = (int)sp_num_segments(P);
  const dim3 grid(nseg, B, desc->num_maps);
  int32_t* segc = static_cast<int32_t*>(workspace);
  hipLaunchKernelGGL(spots_batch_count_kernel, grid, dim3(SP_THREADS), 0, (hipStream_t)stream, a, P, nseg, segc);
  hipLaunchKernelGGL(spots_batch_write_kernel, grid, dim3(SP_THREADS), 0, (hipStream_t)stream, a, P, N, nseg, segc,
                     static_cast<int4*>(records), counts, max_spots);
  return check_launch("peneo_spots_compact_batch");
}
