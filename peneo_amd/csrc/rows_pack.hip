// Packed ("varlen") inference, the row movers (version 113; include/peneo_hip.h: peneo_pack_plan, peneo_rows_pack, peneo_rows_unpack).
//
//   * peneo_pack_plan: per-document order-preserving compaction of the int32 key mask [B, T] - lens, the exclusive row offsets cu_rows
//     and live_t (the original position of the i'-th live token, -1 from lens[b] on).  One launch of B workgroups, no atomics, no
//     workspace: workgroup b counts the live tokens of the documents before it itself (a contiguous range of the mask; B x T is a few
//     thousand words) and compacts its own row with a ballot / popcount scan, 256 positions per step.
//   * peneo_rows_pack: gathers rows src[b, live_t[b, i']] into the cu_rows layout (activations) or the per-document layout
//     [B, Tm, row] with the rows from lens[b] on zero-filled (the int32 pos / xs / ys inputs of peneo_relpos_buckets).
//   * peneo_rows_unpack: writes EVERY row of dst [B, T, row]: row (b, t) is looked up in the ascending live_t[b, 0 .. lens[b]) by
//     bisection - found at i': the packed row cu_rows[b] + i', else zeros.  No second pass, no ordering between workgroups.
//
// Rows move as 16-byte pieces where the row size and both base pointers allow it, else as dwords.  Every index read from the plan is
// range-checked against the caller's extents before it addresses memory (a row outside them is treated as absent).
#include "common.h"

namespace peneo {
namespace {

__global__ __launch_bounds__(256) void pack_plan_kernel(const int32_t* __restrict__ mask, int B, int T, int32_t* __restrict__ lens,
                                                        int32_t* __restrict__ cu_rows, int32_t* __restrict__ live_t) {
  __shared__ int wsum[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // live tokens of the documents before this one
  int before = 0;
  for (int64_t i = tid, n = (int64_t)b * T; i < n; i += 256) before += mask[i] != 0;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) before += __shfl_xor(before, s, 64);
  if (lane == 0) wsum[wave] = before;
  __syncthreads();
  before = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  // this document: positions of its live tokens, in order
  const int32_t* m = mask + (int64_t)b * T;
  int32_t* lt = live_t + (int64_t)b * T;
  int base = 0;
  for (int t0 = 0; t0 < T; t0 += 256) {
    const int t = t0 + tid;
    const bool live = t < T && m[t] != 0;
    const uint64_t bal = __builtin_amdgcn_ballot_w64(live);
    const int pre = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __builtin_popcountll(bal);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (live) lt[off + pre] = t;                  // off + pre <= t < T
    base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  for (int t = base + tid; t < T; t += 256) lt[t] = -1;
  if (tid == 0) {
    lens[b] = base;
    cu_rows[b] = before;
    if (b == B - 1) cu_rows[B] = before + base;
  }
}

template <typename V> __device__ __forceinline__ V zero_piece();
template <> __device__ __forceinline__ uint4 zero_piece<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }
template <> __device__ __forceinline__ uint32_t zero_piece<uint32_t>() { return 0u; }

// one thread per piece of a destination row (b, i), i < Tm.  cu_rows NULL: the per-document layout (every row written)
template <typename V>
__global__ __launch_bounds__(256) void rows_pack_kernel(const V* __restrict__ src, const int32_t* __restrict__ live_t,
                                                        const int32_t* __restrict__ lens, const int32_t* __restrict__ cu_rows, int B, int T,
                                                        int Tm, int per_row, int64_t dst_rows, V* __restrict__ dst) {
  const int64_t total = (int64_t)B * Tm * per_row;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / per_row;
    const int c = (int)(idx - row * per_row), b = (int)(row / Tm), i = (int)(row - (int64_t)b * Tm);
    const int n = min(lens[b], T);
    int t = -1;
    if (i < n) t = live_t[(int64_t)b * T + i];
    const bool live = t >= 0 && t < T;
    if (cu_rows) {
      const int64_t r = (int64_t)cu_rows[b] + i;
      if (live && r >= 0 && r < dst_rows) dst[r * per_row + c] = src[((int64_t)b * T + t) * per_row + c];
    } else {
      dst[row * per_row + c] = live ? src[((int64_t)b * T + t) * per_row + c] : zero_piece<V>();
    }
  }
}

// one thread per piece of a destination row (b, t), t < T: every row is written
template <typename V>
__global__ __launch_bounds__(256) void rows_unpack_kernel(const V* __restrict__ src, int64_t src_rows, const int32_t* __restrict__ live_t,
                                                          const int32_t* __restrict__ lens, const int32_t* __restrict__ cu_rows, int B, int T,
                                                          int per_row, V* __restrict__ dst) {
  const int64_t total = (int64_t)B * T * per_row;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / per_row;
    const int c = (int)(idx - row * per_row), b = (int)(row / T), t = (int)(row - (int64_t)b * T);
    const int32_t* lt = live_t + (int64_t)b * T;
    int lo = 0, hi = min(max(lens[b], 0), T);      // first i' in [0, lens[b]) with live_t[b, i'] >= t
    const int n = hi;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (lt[mid] < t) lo = mid + 1; else hi = mid;
    }
    V v = zero_piece<V>();
    if (lo < n && lt[lo] == t) {
      const int64_t r = (int64_t)cu_rows[b] + lo;
      if (r >= 0 && r < src_rows) v = src[r * per_row + c];
    }
    dst[row * per_row + c] = v;
  }
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
unsigned blocks_for(int64_t pieces) {
  int64_t n = (pieces + 255) / 256;
  return (unsigned)(n < 1 ? 1 : n > 65536 ? 65536 : n);
}

}  // namespace
}  // namespace peneo

using namespace peneo;

extern "C" int peneo_pack_plan(const int32_t* key_mask, int B, int T, int32_t* lens, int32_t* cu_rows, int32_t* live_t,
                               peneo_stream_t stream) {
  PENEO_REQUIRE(key_mask && lens && cu_rows && live_t, "peneo_pack_plan: null pointer");
  PENEO_REQUIRE(B > 0 && T > 0 && (int64_t)B * T <= 0x7fffffff, "peneo_pack_plan: bad sizes B=%d T=%d", B, T);
  hipLaunchKernelGGL(pack_plan_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, key_mask, B, T, lens, cu_rows, live_t);
  return check_launch("peneo_pack_plan");
}

extern "C" int peneo_rows_pack(const void* src, const int32_t* live_t, const int32_t* lens, const int32_t* cu_rows, int B, int T, int Tm,
                               int64_t row_bytes, void* dst, int64_t dst_rows, peneo_stream_t stream) {
  PENEO_REQUIRE(src && live_t && lens && dst, "peneo_rows_pack: null pointer");
  PENEO_REQUIRE(B > 0 && T > 0 && Tm > 0 && Tm <= T && (int64_t)B * T <= 0x7fffffff, "peneo_rows_pack: bad sizes B=%d T=%d Tm=%d", B, T, Tm);
  PENEO_REQUIRE(row_bytes > 0 && row_bytes % 4 == 0 && row_bytes <= (1 << 24), "peneo_rows_pack: row_bytes=%lld must be a multiple of 4",
                (long long)row_bytes);
  PENEO_REQUIRE(al4(src) && al4(dst), "peneo_rows_pack: src and dst must be 4-byte aligned");
  PENEO_REQUIRE(cu_rows ? dst_rows > 0 : dst_rows == (int64_t)B * Tm,
                "peneo_rows_pack: dst_rows=%lld (the cu_rows layout needs > 0, the per-document layout B * Tm)", (long long)dst_rows);
  hipStream_t st = (hipStream_t)stream;
  if (row_bytes % 16 == 0 && al16(src) && al16(dst)) {
    const int per_row = (int)(row_bytes / 16);
    hipLaunchKernelGGL(rows_pack_kernel<uint4>, dim3(blocks_for((int64_t)B * Tm * per_row)), dim3(256), 0, st, (const uint4*)src, live_t, lens,
                       cu_rows, B, T, Tm, per_row, dst_rows, (uint4*)dst);
  } else {
    const int per_row = (int)(row_bytes / 4);
    hipLaunchKernelGGL(rows_pack_kernel<uint32_t>, dim3(blocks_for((int64_t)B * Tm * per_row)), dim3(256), 0, st, (const uint32_t*)src, live_t,
                       lens, cu_rows, B, T, Tm, per_row, dst_rows, (uint32_t*)dst);
  }
  return check_launch("peneo_rows_pack");
}

extern "C" int peneo_rows_unpack(const void* src, int64_t src_rows, const int32_t* live_t, const int32_t* lens, const int32_t* cu_rows, int B,
                                 int T, int64_t row_bytes, void* dst, peneo_stream_t stream) {
  PENEO_REQUIRE(src && live_t && lens && cu_rows && dst, "peneo_rows_unpack: null pointer");
  PENEO_REQUIRE(B > 0 && T > 0 && src_rows > 0 && (int64_t)B * T <= 0x7fffffff, "peneo_rows_unpack: bad sizes B=%d T=%d src_rows=%lld", B, T,
                (long long)src_rows);
  PENEO_REQUIRE(row_bytes > 0 && row_bytes % 4 == 0 && row_bytes <= (1 << 24), "peneo_rows_unpack: row_bytes=%lld must be a multiple of 4",
                (long long)row_bytes);
  PENEO_REQUIRE(al4(src) && al4(dst), "peneo_rows_unpack: src and dst must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (row_bytes % 16 == 0 && al16(src) && al16(dst)) {
    const int per_row = (int)(row_bytes / 16);
    hipLaunchKernelGGL(rows_unpack_kernel<uint4>, dim3(blocks_for((int64_t)B * T * per_row)), dim3(256), 0, st, (const uint4*)src, src_rows,
                       live_t, lens, cu_rows, B, T, per_row, (uint4*)dst);
  } else {
    const int per_row = (int)(row_bytes / 4);
    hipLaunchKernelGGL(rows_unpack_kernel<uint32_t>, dim3(blocks_for((int64_t)B * T * per_row)), dim3(256), 0, st, (const uint32_t*)src,
                       src_rows, live_t, lens, cu_rows, B, T, per_row, (uint32_t*)dst);
  }
  return check_launch("peneo_rows_unpack");
}
