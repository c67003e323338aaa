// Plain integer arithmetic of the one-per-CU 384 x 192 launches (gemm_big.hip), kept free of HIP so that a host program can
// call the same functions the kernels call (tests/host/gemm_walk_check.cpp walks every tile of a launch with them).
#pragma once

#if defined(__HIPCC__)
#define PENEO_WALK_FN __host__ __device__ inline
#else
#define PENEO_WALK_FN inline
#endif

namespace peneo {

// XCD-aware order of a launch of `total` workgroups: workgroup ids go round-robin to the 8 XCDs, XCD x gets the contiguous band
// of tiles [x q + min(x, r), ...) with q = total / 8, r = total % 8.  A bijection of [0, total).
PENEO_WALK_FN int walk_xcd_tile(int lin, int total) {
  const int q8 = total >> 3, r8 = total & 7, xcd = lin & 7, slot = lin >> 3;
  return xcd * q8 + (xcd < r8 ? xcd : r8) + slot;
}

// Tile `tile` of a group whose problem i owns the tiles [first_tile[i], first_tile[i + 1]) with tiles_n[i] tiles per row of
// tiles, n fastest: which problem, and the tile's first row and column.
struct WalkTile { int problem, m0, n0; };
PENEO_WALK_FN WalkTile walk_group_tile(int tile, const int* first_tile, const int* tiles_n, int n, int bm, int bn) {
  int i = 0;
  for (int k = 1; k < n; ++k)
    if (tile >= first_tile[k]) i = k;
  const int t = tile - first_tile[i];
  return WalkTile{i, (t / tiles_n[i]) * bm, (t % tiles_n[i]) * bn};
}

// The tile table of a group of n <= max_n problems of whole bm x bn tiles (M[i] % bm == 0, N[i] % bn == 0), as the launch fills it:
// first_tile[0 .. max_n] and tiles_n[0 .. max_n); the unused slots i >= n own no tile (first_tile[i] = the total) and repeat the last
// problem's tiles_n.  Returns the number of tiles = workgroups of the launch.
PENEO_WALK_FN int walk_group_fill(const int* M, const int* N, int n, int max_n, int bm, int bn, int* first_tile, int* tiles_n) {
  int tiles = 0;
  for (int i = 0; i < max_n; ++i) {
    const int j = i < n ? i : n - 1;
    first_tile[i] = tiles;
    tiles_n[i] = N[j] / bn;
    if (i < n) tiles += (M[j] / bm) * (N[j] / bn);
  }
  first_tile[max_n] = tiles;
  return tiles;
}

// Ragged K with mn-major operands ([K][rows], K % 8 == 0): a 1 KiB piece is 8 k-rows x 64 columns, so the last k-tile of 64
// holds walk_tail_pieces(K) row blocks of 8 that exist (0 = no tail); the blocks behind them are never requested.
PENEO_WALK_FN int walk_tail_pieces(int K) { return ((K & 63) + 7) >> 3; }
// Is piece g of an operand tile with `quads` 64-column quads (piece g = k-row block g / quads, quad g % quads) requested in a
// tail of `tail_pieces` row blocks?
PENEO_WALK_FN bool walk_piece_in_tail(int g, int quads, int tail_pieces) { return g / quads < tail_pieces; }

}  // namespace peneo
