// Stand-alone driver of the Jacobian structure plan in csrc/ba_evaluate_plan.cpp (tests/test_jacobian_plan_host.py builds it with
// -fsanitize=address,undefined and runs it as a child process): the compressed-row structure of rsba_solver_jacobian_structure and
// the tables k_eval_jacobian_* read, checked against the contracts the kernels and the callers rely on —
//   row_ptr is monotone, starts at 0 and ends at the number of nonzeros; all rows of an observation have the layout's width,
//   widths are in {0, 3, 6, 9} (point model) / {0, 6, 12, 18} (marker chain),
//   columns ascend inside a row and lie inside the blocks the observation names,
//   every free named block is present exactly once per row, with all of its columns; constant and base blocks are absent,
//   an observation's piece starts at off[i] and off is what the row pointers say,
//   the point rows name the observation's camera and the device position of its point.
// usage: jacobian_plan_driver <tests/golden/hongo/correspondence.txt>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <numeric>
#include <random>
#include <vector>

#include "ba_evaluate_plan.hpp"

using namespace rsba;

static int g_checks = 0;
#define CHECK(cond)                                                                   \
  do {                                                                                \
    ++g_checks;                                                                       \
    if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)

static bool Const(const std::vector<uint8_t>& flags, int b) { return b >= 0 && (size_t)b < flags.size() && flags[b] != 0; }

struct Block {
  int offset, size;
  bool free;
};

// The structure of `l` against the blocks every observation names (in ascending offset order), `d` rows per observation.
static void CheckStructure(const EvalJacobianLayout& l, int d, int64_t num_cols, const std::vector<std::vector<Block>>& named,
                           const std::vector<int64_t>& row_ptr, const std::vector<int32_t>& cols, std::initializer_list<int> widths) {
  const size_t N = named.size();
  CHECK(l.width.size() == N && l.off.size() == N + 1 && l.off[0] == 0);
  CHECK(row_ptr.size() == (size_t)d * N + 1 && row_ptr[0] == 0 && row_ptr.back() == l.off[N] && (int64_t)cols.size() == l.off[N]);
  for (size_t i = 0; i < N; ++i) {
    const int w = l.width[i];
    CHECK(std::find(widths.begin(), widths.end(), w) != widths.end());
    CHECK(l.off[i + 1] - l.off[i] == (int64_t)d * w && l.off[i] == row_ptr[(size_t)d * i]);
    int expect = 0;
    for (const Block& b : named[i]) if (b.free) expect += b.size;
    CHECK(w == expect);
    for (int r = 0; r < d; ++r) {
      const int64_t lo = row_ptr[(size_t)d * i + r], hi = row_ptr[(size_t)d * i + r + 1];
      CHECK(lo <= hi && hi - lo == w && lo == l.off[i] + (int64_t)r * w);
      int64_t q = lo;
      for (const Block& b : named[i]) {
        if (!b.free) continue;   // constant (or base: not in `named` at all): absent
        for (int a = 0; a < b.size; ++a, ++q) CHECK(q < hi && cols[q] == b.offset + a && cols[q] >= 0 && cols[q] < num_cols);
      }
      CHECK(q == hi);   // ... and nothing else: every free named block exactly once
      for (int64_t e = lo + 1; e < hi; ++e) CHECK(cols[e - 1] < cols[e]);
    }
  }
}

static void CheckPoints(int C, int P, const std::vector<int32_t>& cam, const std::vector<int32_t>& pt, const std::vector<int>& pt_perm,
                        const std::vector<uint8_t>& cconst, const std::vector<uint8_t>& pconst) {
  const int64_t N = (int64_t)cam.size();
  const EvalJacobianLayout l = EvalPointJacobianLayout(N, cam.data(), pt.data(), cconst, pconst);
  CHECK(l.off.size() == (size_t)N + 1);
  std::vector<int64_t> row_ptr(2 * (size_t)N + 1, -1);
  std::vector<int32_t> cols((size_t)l.off[N], -1);
  EvalJacobianRowPtr(l, 2, row_ptr.data());
  EvalPointJacobianCols(l, C, cam.data(), pt.data(), cconst, pconst, cols.data());
  EvalJacobianRowPtr(l, 2, nullptr);   // a NULL output: nothing is written
  EvalPointJacobianCols(l, C, cam.data(), pt.data(), cconst, pconst, nullptr);
  std::vector<std::vector<Block>> named((size_t)N);
  for (int64_t i = 0; i < N; ++i)
    named[i] = {Block{6 * cam[i], 6, !Const(cconst, cam[i])}, Block{6 * C + 3 * pt[i], 3, !Const(pconst, pt[i])}};
  CheckStructure(l, 2, 6 * (int64_t)C + 3 * (int64_t)P, named, row_ptr, cols, {0, 3, 6, 9});
  const std::vector<EvalJacobianPointRow> rows = EvalJacobianPointRows(P, N, cam.data(), pt.data(), pt_perm);
  CHECK(rows.size() == (size_t)N);
  for (int64_t i = 0; i < N; ++i) {
    CHECK(rows[i].camera == cam[i] && rows[i].point >= 0 && rows[i].point < P);
    CHECK((pt_perm.empty() ? rows[i].point : pt_perm[rows[i].point]) == pt[i]);
  }
}

static void CheckMarker(int nb, const std::vector<EvalMarkerRow>& rows, const std::vector<uint8_t>& constant) {
  const EvalJacobianLayout l = EvalMarkerJacobianLayout(rows, constant);
  CHECK(l.off.size() == rows.size() + 1);
  std::vector<int64_t> row_ptr(8 * rows.size() + 1, -1);
  std::vector<int32_t> cols((size_t)l.off[rows.size()], -1);
  EvalJacobianRowPtr(l, 8, row_ptr.data());
  EvalMarkerJacobianCols(l, rows, constant, cols.data());
  EvalMarkerJacobianCols(l, rows, constant, nullptr);
  std::vector<std::vector<Block>> named(rows.size());
  for (size_t i = 0; i < rows.size(); ++i)
    for (int b : {rows[i].cam_block, rows[i].time_block, rows[i].marker_block})
      if (b >= 0) { CHECK(b < nb); named[i].push_back(Block{6 * b, 6, !Const(constant, b)}); }
  CheckStructure(l, 8, 6 * (int64_t)nb, named, row_ptr, cols, {0, 6, 12, 18});
  // the base blocks (-1 in the row) hold no column of that observation
  for (size_t i = 0; i < rows.size(); ++i)
    for (int64_t q = row_ptr[8 * i]; q < row_ptr[8 * i + 8]; ++q) {
      const int b = cols[q] / 6;
      CHECK(b == rows[i].cam_block || b == rows[i].time_block || b == rows[i].marker_block);
    }
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s correspondence.txt\n", argv[0]); return 2; }
  {
    // the hongo indices, wired as RSBA_MODEL_MARKER_CHAIN (camera 0 / marker 0: no parameters) and as _TEST2 (camera 0 only)
    std::ifstream f(argv[1]);
    int T = 0, C = 0, M = 0, N = 0;
    f >> T >> C >> M >> N;
    CHECK(f.good() && T > 0 && C > 0 && M > 0 && N > 0);
    double skip;
    for (int i = 0; i < T * (1 + C); ++i) f >> skip;
    std::vector<int> t(N), c(N), m(N);
    for (int i = 0; i < N; ++i) { f >> t[i] >> c[i] >> m[i]; for (int e = 0; e < 8; ++e) f >> skip; }
    CHECK(f.good());
    for (int test2 = 0; test2 < 2; ++test2) {
      std::vector<EvalMarkerRow> rows(N);
      for (int i = 0; i < N; ++i) rows[i] = EvalMarkerRow{c[i] != 0 ? c[i] : -1, C + t[i], (test2 || m[i] != 0) ? C + T + m[i] : -1, c[i]};
      CheckMarker(C + T + M, rows, {});
      std::vector<uint8_t> constant(C + T + 2, 0);   // shorter than the block array: the rest is free
      constant[1] = 1; constant[C + 2] = 1; constant[C + T + 1] = 1;
      CheckMarker(C + T + M, rows, constant);
    }
    printf("hongo: %d observations checked\n", N);
  }
  {
    // a seeded random point shape with an unreferenced camera (3) and an unreferenced point (11), a constant camera (0) and a
    // constant point (5; 11 is constant AND unreferenced), a duplicate row, shuffled rows, in file order and in a shuffled point order
    std::mt19937 rng(20240611);
    const int C = 7, P = 150;
    std::vector<int32_t> cam, pt;
    for (int j = 0; j < P; ++j) {
      if (j == 11) continue;
      const int k = 1 + (int)(rng() % 6);
      for (int e = 0; e < k; ++e) { int c = (int)(rng() % C); if (c == 3) c = 4; cam.push_back(c); pt.push_back(j); }
    }
    cam.push_back(0); pt.push_back(5);            // constant camera x constant point: an observation without a free block
    cam.push_back(cam[0]); pt.push_back(pt[0]);   // a duplicate of the first row, at the end
    std::vector<int> sh(cam.size());
    std::iota(sh.begin(), sh.end(), 0);
    std::shuffle(sh.begin(), sh.end(), rng);
    std::vector<int32_t> cam2(cam.size()), pt2(pt.size());
    for (size_t i = 0; i < sh.size(); ++i) { cam2[i] = cam[sh[i]]; pt2[i] = pt[sh[i]]; }
    std::vector<int> perm(P);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<uint8_t> cconst(C, 0), pconst(20, 0);
    cconst[0] = 1; pconst[5] = 1; pconst[11] = 1;
    CheckPoints(C, P, cam2, pt2, {}, {}, {});
    CheckPoints(C, P, cam2, pt2, perm, cconst, pconst);
    printf("random point shape: %zu observations checked\n", cam2.size());
  }
  {
    // the empty problem, one observation, an observation all of whose blocks are constant
    CheckPoints(2, 3, {}, {}, {}, {}, {});
    CheckPoints(2, 3, {1}, {2}, {2, 0, 1}, {0, 1}, {});
    CheckPoints(2, 3, {1}, {2}, {}, {0, 1}, {0, 0, 1});
    CheckMarker(5, {}, {});
    CheckMarker(5, {EvalMarkerRow{-1, 2, -1, 0}}, {});
    CheckMarker(5, {EvalMarkerRow{1, 2, 4, 1}}, {0, 0, 1});
    CheckMarker(5, {EvalMarkerRow{1, 2, 4, 1}}, {0, 1, 1, 0, 1});
    CheckMarker(5, {EvalMarkerRow{-1, 2, -1, 0}}, {0, 0, 1});
    printf("empty, single-observation and all-constant problems checked\n");
  }
  printf("jacobian plan driver: ok (%d checks)\n", g_checks);
  return 0;
}
