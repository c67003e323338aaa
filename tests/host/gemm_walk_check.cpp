// Host check of the integer arithmetic the 384 x 192 one-per-CU launches share with this program (peneo_amd/csrc/gemm_walk.h):
// the XCD-aware order, the grouped tile walk (workgroup -> problem, m0, n0) and the pieces of a ragged last k-tile.
// Built with -fsanitize=address,undefined and run on the CPU by tests/test_gemm_walk_host.py; exit status 0 = every check held.
#include <cstdio>
#include <vector>

#include "../../peneo_amd/csrc/gemm_walk.h"

using namespace peneo;

namespace {

constexpr int BM = 384, BN = 192, GROUP_MAX = 4;
int failures = 0;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::fprintf(stderr, "FAILED %s: ", #cond);         \
      std::fprintf(stderr, __VA_ARGS__);                  \
      std::fprintf(stderr, "\n");                         \
      ++failures;                                         \
    }                                                     \
  } while (0)

struct Shape { int M, N; };

// every workgroup of the launch lands on one output tile, and every output tile of every problem is hit exactly once
void check_group(const std::vector<Shape>& shapes, const char* what) {
  const int n = (int)shapes.size();
  int first_tile[GROUP_MAX + 1], tiles_n[GROUP_MAX], Ms[GROUP_MAX], Ns[GROUP_MAX];
  int expect = 0;
  for (int i = 0; i < n; ++i) { Ms[i] = shapes[i].M; Ns[i] = shapes[i].N; expect += (shapes[i].M / BM) * (shapes[i].N / BN); }
  // the table as launch_gemm_big_group fills it: the same function
  const int tiles = walk_group_fill(Ms, Ns, n, GROUP_MAX, BM, BN, first_tile, tiles_n);
  CHECK(tiles == expect && first_tile[GROUP_MAX] == tiles, "%s: %d tiles, want %d", what, tiles, expect);
  for (int i = n; i < GROUP_MAX; ++i) CHECK(first_tile[i] == tiles, "%s: unused slot %d owns tiles from %d", what, i, first_tile[i]);
  std::vector<std::vector<int>> hits(n);
  for (int i = 0; i < n; ++i) hits[i].assign((shapes[i].M / BM) * (shapes[i].N / BN), 0);
  std::vector<int> order_hits(tiles, 0);
  int prev_problem = -1, prev_tile = -1;
  for (int lin = 0; lin < tiles; ++lin) {
    const int tile = walk_xcd_tile(lin, tiles);
    CHECK(tile >= 0 && tile < tiles, "%s: workgroup %d -> tile %d of %d", what, lin, tile, tiles);
    if (tile < 0 || tile >= tiles) continue;
    ++order_hits[tile];
    const WalkTile w = walk_group_tile(tile, first_tile, tiles_n, n, BM, BN);
    CHECK(w.problem >= 0 && w.problem < n, "%s: tile %d -> problem %d", what, tile, w.problem);
    if (w.problem < 0 || w.problem >= n) continue;
    const Shape& s = shapes[w.problem];
    CHECK(w.m0 >= 0 && w.m0 % BM == 0 && w.m0 + BM <= s.M && w.n0 >= 0 && w.n0 % BN == 0 && w.n0 + BN <= s.N,
          "%s: tile %d -> problem %d at (%d, %d) outside %d x %d", what, tile, w.problem, w.m0, w.n0, s.M, s.N);
    if (w.m0 < 0 || w.m0 + BM > s.M || w.n0 < 0 || w.n0 + BN > s.N) continue;
    ++hits[w.problem][(w.m0 / BM) * (s.N / BN) + w.n0 / BN];
  }
  for (int t = 0; t < tiles; ++t) CHECK(order_hits[t] == 1, "%s: tile %d taken %d times by the XCD order", what, t, order_hits[t]);
  for (int i = 0; i < n; ++i)
    for (size_t t = 0; t < hits[i].size(); ++t) CHECK(hits[i][t] == 1, "%s: problem %d tile %zu computed %d times", what, i, t, hits[i][t]);
  // the tiles of one problem are contiguous in tile order, n fastest
  for (int tile = 0; tile < tiles; ++tile) {
    const WalkTile w = walk_group_tile(tile, first_tile, tiles_n, n, BM, BN);
    const int t = (w.m0 / BM) * tiles_n[w.problem] + w.n0 / BN;
    CHECK(w.problem >= prev_problem, "%s: tile %d goes back to problem %d", what, tile, w.problem);
    if (w.problem == prev_problem) CHECK(t == prev_tile + 1, "%s: tile %d is tile %d of its problem after %d", what, tile, t, prev_tile);
    else CHECK(t == 0, "%s: problem %d starts at its tile %d", what, w.problem, t);
    prev_problem = w.problem;
    prev_tile = t;
  }
}

// a tail of rem = K % 64 rows holds ceil(rem / 8) row blocks of 8; over the 8 waves x (quads pieces per wave) of an operand tile the
// requested pieces are exactly those whose 8 rows lie below K, each once
void check_tail(int K) {
  const int rem = K % 64, pieces = walk_tail_pieces(K);
  CHECK(pieces == (rem + 7) / 8, "K = %d: %d tail pieces", K, pieces);
  for (int quads : {BM / 64, BN / 64}) {
    std::vector<int> requested(8 * quads, 0);
    int count = 0;
    for (int wave = 0; wave < 8; ++wave)
      for (int u = 0; u < quads; ++u) {       // pieces per wave and operand = quads (APW = BM / 64, BPW = BN / 64)
        const int g = wave + 8 * u;
        if (walk_piece_in_tail(g, quads, pieces)) { ++requested[g]; ++count; }
      }
    CHECK(count == pieces * quads, "K = %d, %d quads: %d pieces requested", K, quads, count);
    for (int g = 0; g < 8 * quads; ++g) {
      const int first_row = (K - rem) + (g / quads) * 8;      // the piece's first k-row; its last is first_row + 7
      const bool below = first_row + 8 <= K;
      CHECK(requested[g] == (below ? 1 : 0), "K = %d, %d quads: piece %d (rows %d..%d) requested %d times", K, quads, g, first_row,
            first_row + 7, requested[g]);
    }
  }
}

}  // namespace

int main() {
  // the groups of tests/test_gpu_gemm_group_nn384.py, and the benchmark's four weight gradients (H = 768, I = 3072)
  check_group({{384, 192}, {768, 192}, {384, 576}, {768, 384}}, "test group");
  check_group({{2304, 768}, {3072, 768}, {768, 3072}, {768, 768}}, "encoder layer H = 768");
  check_group({{1152, 384}, {768, 384}, {384, 768}, {384, 384}}, "encoder layer H = 384");
  check_group({{384, 192}}, "one tile");
  check_group({{768, 192}, {384, 192}}, "three tiles");
  for (int total = 1; total <= 300; ++total) {       // the XCD order is a bijection at every launch size
    std::vector<int> seen(total, 0);
    for (int lin = 0; lin < total; ++lin) {
      const int t = walk_xcd_tile(lin, total);
      CHECK(t >= 0 && t < total, "launch of %d: workgroup %d -> %d", total, lin, t);
      if (t >= 0 && t < total) ++seen[t];
    }
    for (int t = 0; t < total; ++t) CHECK(seen[t] == 1, "launch of %d: tile %d taken %d times", total, t, seen[t]);
  }
  for (int K : {8, 40, 64, 104, 168, 232, 5672, 65536, 65544}) check_tail(K);
  for (int K = 8; K <= 1024; K += 8) check_tail(K);
  if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
  std::puts("gemm_walk_check: ok");
  return 0;
}
