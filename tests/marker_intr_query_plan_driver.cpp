// Stand-alone driver of the host plans behind the queries of a solver with free intrinsics under the extended layout
// (tests/test_marker_intr_query_plan_host.py builds it with -fsanitize=address,undefined and runs it as a child process):
//   evaluate    PlanEvalMarkerIntr (csrc/ba_evaluate_plan.cpp): the lists over [C | T | M | C intrinsics blocks].  The pose part is
//               BuildEvalMarkerLists' own; camera k's list names every detection of camera k exactly once, ascending, through the
//               (obs, slot) encoding k_eval_marker_block_sum decodes — 18 obs + 6 slot = 18 N + 6 i — and no entry reads past the
//               24 N doubles of the J'r buffer; live = mask != 0 and some detection; held = the clear mask bits of a live block, a pose
//               block's subset mask, 0 for a block that is not live
//   covariance  CovMarkerIntrColumns / CovPlanMarkerIntrRows (csrc/ba_covariance_plan.hpp): the intrinsics blocks' columns behind the
//               pose blocks', ascending camera index, only for a mask on a detected camera; bsub and the rows' bits 18-23; offset
//               resolution of num_parameters + 6 k (REDUCED, CONSTANT for mask 0, RSBA_ERR_ARG for a camera nobody detects, for an
//               offset inside a block and behind the last block); I back to 0 after CovMarkerColumns
// Shapes: a seeded random rig with an undetected camera, a detected camera with mask 0 and short flag vectors; one observation; the
// empty problem; both paths.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "ba_covariance_plan.hpp"
#include "ba_evaluate_plan.hpp"

using namespace rsba;

static long g_checks = 0;
static std::string g_case;
#define CHECK(cond)                                                                                                        \
  do {                                                                                                                     \
    ++g_checks;                                                                                                            \
    if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_case.c_str()); exit(1); }       \
  } while (0)

struct Obs { int c, t, m; };
static rsba_problem MarkerProblem(int C, int T, int M, const std::vector<Obs>& obs) {
  rsba_problem p;
  p.model = RSBA_MODEL_MARKER_CHAIN;
  p.num_cameras = C; p.num_times = T; p.num_markers = M; p.marker_side = 0.1;
  for (const Obs& o : obs) { p.camera_index.push_back(o.c); p.time_index.push_back(o.t); p.marker_index.push_back(o.m); }
  p.num_observations = (int64_t)obs.size();
  p.observations.resize(8 * obs.size());
  for (size_t i = 0; i < p.observations.size(); ++i) p.observations[i] = (double)i;
  p.parameters.assign(6 * (size_t)(C + T + M), 0.0);
  p.intrinsics.assign(4 * (size_t)C, 1.0);
  return p;
}
static int MaskOf(const std::vector<int>& m, int k) { return k < (int)m.size() ? m[k] & 63 : 0; }

static void CheckEvaluate(const rsba_problem& p, const std::vector<uint8_t>& constant, const std::vector<uint8_t>& subset, const std::vector<int>& mask) {
  const int C = p.num_cameras, nb = C + p.num_times + p.num_markers;
  const std::vector<EvalMarkerRow> rows = EvalMarkerRows(p);
  const size_t N = rows.size();
  const EvalMarkerIntrPlan x = PlanEvalMarkerIntr(nb, C, rows, constant, subset, mask);
  const EvalMarkerLists pose = BuildEvalMarkerLists(nb, rows);
  const std::vector<unsigned char> pose_live = EvalMarkerLive(nb, rows, constant);
  CHECK((int)x.lists.ptr.size() == nb + C + 1 && (int)x.live.size() == nb + C && (int)x.held.size() == nb + C);
  for (int b = 0; b <= nb; ++b) CHECK(x.lists.ptr[b] == pose.ptr[b]);
  CHECK(x.lists.obs.size() == pose.obs.size() + N && x.lists.slot.size() == x.lists.obs.size());
  for (size_t q = 0; q < pose.obs.size(); ++q) CHECK(x.lists.obs[q] == pose.obs[q] && x.lists.slot[q] == pose.slot[q]);
  CHECK((size_t)x.lists.ptr[nb + C] == x.lists.obs.size());
  std::vector<int> seen(N, 0), count(C, 0);
  for (int k = 0; k < C; ++k) {
    CHECK(x.lists.ptr[nb + k] <= x.lists.ptr[nb + k + 1]);
    long last = -1;
    for (int q = x.lists.ptr[nb + k]; q < x.lists.ptr[nb + k + 1]; ++q) {
      const long at = 18L * x.lists.obs[q] + 6L * x.lists.slot[q];     // what k_eval_marker_block_sum reads: six doubles from here
      CHECK(x.lists.slot[q] < 3 && at >= 18L * (long)N && at + 6 <= 24L * (long)N && (at - 18L * (long)N) % 6 == 0);
      const long i = (at - 18L * (long)N) / 6;
      CHECK(i > last && rows[i].camera == k);
      last = i;
      seen[i]++; count[k]++;
    }
  }
  for (size_t i = 0; i < N; ++i) CHECK(seen[i] == 1);
  for (int b = 0; b < nb; ++b) {
    CHECK(x.live[b] == pose_live[b]);
    CHECK(x.held[b] == (pose_live[b] && b < (int)subset.size() ? (subset[b] & 63) : 0));
  }
  for (int k = 0; k < C; ++k) {
    const bool live = MaskOf(mask, k) != 0 && count[k] > 0;
    CHECK((x.live[nb + k] != 0) == live);
    CHECK(x.held[nb + k] == (live ? (~MaskOf(mask, k) & 63) : 0));
  }
}

static void CheckCovariance(const rsba_problem& p, const std::vector<uint8_t>& constant, const std::vector<uint8_t>& subset, const std::vector<int>& mask,
                            bool elim_path) {
  const int C = p.num_cameras, nb = C + p.num_times + p.num_markers;
  CovLayout base, L;
  CovMarkerColumns(p, constant, elim_path, &base);
  CovMarkerColumns(p, constant, elim_path, &L);
  CovMarkerIntrColumns(p, mask, &L);
  CHECK(base.I == 0 && L.I == C && L.blocks() == nb && L.all_blocks() == nb + C && (int)L.pos.size() == nb + C && (int)L.ref.size() == nb + C);
  for (int b = 0; b < nb; ++b) CHECK(L.pos[b] == base.pos[b] && L.ref[b] == base.ref[b]);
  std::vector<char> detected(C, 0);
  for (int64_t i = 0; i < p.num_observations; ++i) detected[p.camera_index[i]] = 1;
  int next = base.n;
  for (int k = 0; k < C; ++k) {
    const bool column = detected[k] && MaskOf(mask, k) != 0;
    CHECK((L.ref[nb + k] != 0) == (detected[k] != 0));
    CHECK(L.pos[nb + k] == (column ? next : -1));
    if (column) next += 6;
    CHECK(!L.is_time(nb + k));
    // offsets
    CovBlockRef r;
    const int rc = L.Resolve(6LL * nb + 6LL * k, &r);
    CHECK(rc == (detected[k] ? RSBA_OK : RSBA_ERR_ARG));
    if (rc == RSBA_OK) {
      CHECK(r.size == 6 && r.kind == (column ? CovBlockRef::REDUCED : CovBlockRef::CONSTANT));
      if (column) CHECK(r.idx == L.pos[nb + k]);
      CovSingle q;
      CHECK(L.Single(6LL * nb + 6LL * k, 6LL * nb + 6LL * k, &q) == RSBA_OK && q.what == (column ? CovSingle::SINV : CovSingle::ZEROS));
    }
    CHECK(L.Resolve(6LL * nb + 6LL * k + 3, &r) == RSBA_ERR_ARG);
    CHECK(base.Resolve(6LL * nb + 6LL * k, &r) == RSBA_ERR_ARG);           // without the layout the offset names nothing
  }
  CHECK(L.n == next);
  CovBlockRef r;
  CHECK(L.Resolve(6LL * (nb + C), &r) == RSBA_ERR_ARG && L.Resolve(-6, &r) == RSBA_ERR_ARG);
  // rows
  std::vector<double> w((size_t)p.num_observations, 0.5);
  const CovMarkerRows R0 = CovPlanMarkerRows(p, L, w.data(), subset);
  const CovMarkerRows R = CovPlanMarkerIntrRows(p, L, w.data(), subset, mask);
  CHECK(R.with_sub && (int)R.bsub.size() == nb + C && R.sub18.size() == R.rows.size() && R.rows.size() == R0.rows.size());
  CHECK(R.tptr == R0.tptr && R.obs == R0.obs && R.wrow == R0.wrow);
  for (int b = 0; b < nb; ++b) CHECK(R.bsub[b] == (R0.with_sub ? R0.bsub[b] : 0));
  for (int k = 0; k < C; ++k) CHECK(R.bsub[nb + k] == (L.pos[nb + k] >= 0 ? (~MaskOf(mask, k) & 63) : 0));
  for (size_t q = 0; q < (size_t)p.num_observations; ++q) {
    const int k = R.rows[q].camera;
    CHECK((R.sub18[q] & 0x3FFFF) == (R0.with_sub ? R0.sub18[q] : 0));
    CHECK((R.sub18[q] >> 18) == (L.pos[nb + k] >= 0 ? (~MaskOf(mask, k) & 63) : 63));
  }
  // the next compute without the layout starts clean
  CovMarkerColumns(p, constant, elim_path, &L);
  CHECK(L.I == 0 && (int)L.pos.size() == nb && L.n == base.n);
}

int main() {
  {
    g_case = "random rig";
    const int C = 5, T = 9, M = 4;
    std::mt19937 rng(7);
    std::vector<Obs> obs;
    for (int i = 0; i < 131; ++i) {
      Obs o{(int)(rng() % 4), (int)(rng() % T), (int)(rng() % M)};      // camera 4 detects nothing
      if (o.t == 5) continue;                                            // a time nobody sees
      obs.push_back(o);
    }
    const rsba_problem p = MarkerProblem(C, T, M, obs);
    const std::vector<uint8_t> constant = {0, 1, 0, 0, 0, 0, 1};       // shorter than the block array
    std::vector<uint8_t> subset((size_t)(C + T + M), 0);
    subset[2] = 0b100100; subset[C + 1] = 0b000011; subset[1] = 0b111000;   // (block 1 is constant: its mask is ignored)
    for (const std::vector<int>& mask : {std::vector<int>{0x3F, 0x0F, 0, 0x33, 0}, std::vector<int>{0x01, 0x3F}, std::vector<int>{}}) {
      CheckEvaluate(p, constant, subset, mask);
      CheckEvaluate(p, {}, {}, mask);
      for (bool elim : {false, true}) { CheckCovariance(p, constant, subset, mask, elim); CheckCovariance(p, {}, {}, mask, elim); }
    }
    printf("random rig: %zu observations checked\n", obs.size());
  }
  {
    g_case = "one observation";
    const rsba_problem p = MarkerProblem(2, 1, 2, {Obs{1, 0, 1}});
    CheckEvaluate(p, {}, {}, {0, 0x3F});
    for (bool elim : {false, true}) CheckCovariance(p, {}, {}, {0, 0x3F}, elim);
    g_case = "one observation of the base camera";
    const rsba_problem b = MarkerProblem(2, 1, 2, {Obs{0, 0, 0}});
    CheckEvaluate(b, {}, {}, {0x3F, 0});
    for (bool elim : {false, true}) CheckCovariance(b, {}, {}, {0x3F, 0}, elim);
  }
  {
    g_case = "empty";
    const rsba_problem p = MarkerProblem(2, 1, 1, {});
    CheckEvaluate(p, {}, {}, {0x3F, 0x3F});
    for (bool elim : {false, true}) CheckCovariance(p, {}, {}, {0x3F, 0x3F}, elim);
  }
  printf("marker intrinsics query plan driver: ok (%ld checks)\n", g_checks);
  return 0;
}
