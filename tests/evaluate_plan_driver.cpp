// Stand-alone driver of csrc/ba_evaluate_plan.cpp (tests/test_evaluate_plan_host.py builds it with -fsanitize=address,undefined and runs
// it as a child process): the index structures of rsba_solver_evaluate's gradient kernels, checked against the contracts the kernels
// rely on —
//   every observation appears exactly once in the list of every block it names (with the right slot / the right point),
//   every list is in ascending observation order,
//   the list pointers are right, and a block is live exactly when it is referenced and not constant.
// usage: evaluate_plan_driver <tests/golden/hongo/correspondence.txt>
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

static void CheckMarker(int nb, const std::vector<EvalMarkerRow>& rows, const std::vector<uint8_t>& constant) {
  const EvalMarkerLists l = BuildEvalMarkerLists(nb, rows);
  CHECK((int)l.ptr.size() == nb + 1 && l.ptr[0] == 0);
  size_t named = 0;
  std::vector<char> ref(nb, 0);
  for (const EvalMarkerRow& r : rows)
    for (int b : {r.cam_block, r.time_block, r.marker_block}) if (b >= 0) { ++named; ref[b] = 1; }
  CHECK((size_t)l.ptr[nb] == named && l.obs.size() == named && l.slot.size() == named);
  // seen[3 i + slot]: how often observation i sits in the list of the block it names in that slot
  std::vector<int> seen(3 * rows.size() + 1, 0);
  for (int b = 0; b < nb; ++b) {
    CHECK(l.ptr[b] <= l.ptr[b + 1]);
    for (int q = l.ptr[b]; q < l.ptr[b + 1]; ++q) {
      const int i = l.obs[q], k = l.slot[q];
      CHECK(i >= 0 && i < (int)rows.size() && k < 3);
      const int blk[3] = {rows[i].cam_block, rows[i].time_block, rows[i].marker_block};
      CHECK(blk[k] == b);
      if (q > l.ptr[b]) CHECK(l.obs[q - 1] < i);
      seen[3 * (size_t)i + k]++;
    }
  }
  for (size_t i = 0; i < rows.size(); ++i) {
    const int blk[3] = {rows[i].cam_block, rows[i].time_block, rows[i].marker_block};
    for (int k = 0; k < 3; ++k) CHECK(seen[3 * i + k] == (blk[k] >= 0 ? 1 : 0));
  }
  const std::vector<unsigned char> live = EvalMarkerLive(nb, rows, constant);
  CHECK((int)live.size() == nb);
  for (int b = 0; b < nb; ++b) {
    const bool is_const = b < (int)constant.size() && constant[b];
    CHECK((live[b] != 0) == (ref[b] && !is_const));
  }
}

static void CheckPoints(int C, int P, const std::vector<int32_t>& cam, const std::vector<int32_t>& pt, const std::vector<int>& pt_perm,
                        const std::vector<uint8_t>& cconst, const std::vector<uint8_t>& pconst) {
  const size_t N = cam.size();
  // the solver's slots: by device position of the point, observations of one point in the problem's order
  std::vector<int> pos(P);
  for (int jn = 0; jn < P; ++jn) pos[pt_perm.empty() ? jn : pt_perm[jn]] = jn;
  std::vector<int64_t> order(N);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return pos[pt[a]] < pos[pt[b]]; });
  const EvalCameraIndex x = BuildEvalCameraIndex(C, P, order, cam.data(), pt.data(), pt_perm);
  CHECK((int)x.ptr.size() == C + 1 && x.ptr[0] == 0 && (size_t)x.ptr[C] == N && x.slot.size() == N && x.point.size() == N);
  std::vector<int> seen(N + 1, 0);
  for (int c = 0; c < C; ++c) {
    CHECK(x.ptr[c] <= x.ptr[c + 1]);
    for (int q = x.ptr[c]; q < x.ptr[c + 1]; ++q) {
      const int s = x.slot[q];
      CHECK(s >= 0 && (size_t)s < N);
      CHECK(cam[order[s]] == c);
      CHECK(x.point[q] >= 0 && x.point[q] < P && x.point[q] == pos[pt[order[s]]]);
      if (q > x.ptr[c]) CHECK(x.slot[q - 1] < s);
      seen[s]++;
    }
  }
  for (size_t s = 0; s < N; ++s) CHECK(seen[s] == 1);
  const std::vector<unsigned char> live = EvalPointLive(C, P, (int64_t)N, cam.data(), pt.data(), cconst, pconst);
  CHECK((int)live.size() == C + P);
  std::vector<char> rc(C, 0), rp(P, 0);
  for (size_t i = 0; i < N; ++i) { rc[cam[i]] = 1; rp[pt[i]] = 1; }
  for (int c = 0; c < C; ++c)
    CHECK((live[c] != 0) == (rc[c] && !(c < (int)cconst.size() && cconst[c])));
  for (int j = 0; j < P; ++j)
    CHECK((live[C + j] != 0) == (rp[j] && !(j < (int)pconst.size() && pconst[j])));
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
    // a seeded random point shape with an unreferenced camera (3) and an unreferenced point (11), a camera observing one point
    // twice, in file order and in a shuffled point order
    std::mt19937 rng(20240611);
    const int C = 7, P = 150;
    std::vector<int32_t> cam, pt;
    for (int j = 0; j < P; ++j) {
      if (j == 11) continue;
      const int k = 1 + (int)(rng() % 6);
      for (int e = 0; e < k; ++e) { int c = (int)(rng() % C); if (c == 3) c = 4; cam.push_back(c); pt.push_back(j); }
    }
    cam.push_back(cam[0]); pt.push_back(pt[0]);   // a duplicate of the first row, at the end
    // rows shuffled: `order` is not the identity
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
    // the empty problem and one observation
    CheckPoints(2, 3, {}, {}, {}, {}, {});
    CheckPoints(2, 3, {1}, {2}, {2, 0, 1}, {0, 1}, {});
    CheckMarker(5, {}, {});
    CheckMarker(5, {EvalMarkerRow{-1, 2, -1, 0}}, {});
    CheckMarker(5, {EvalMarkerRow{1, 2, 4, 1}}, {0, 0, 1});
    printf("empty and single-observation problems checked\n");
  }
  printf("evaluate plan driver: ok (%d checks)\n", g_checks);
  return 0;
}
