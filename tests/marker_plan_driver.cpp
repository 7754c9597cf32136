// Stand-alone driver of csrc/ba_marker_plan.hpp (tests/test_marker_plan_host.py builds it with -fsanitize=address,undefined and runs it
// as a child process): the index tables and the path rules of the marker chain's time elimination.
//   marker_plan_driver FILE   plans the problem whose wiring FILE holds, under the switches of the environment
//                             (MarkerSwitches::FromEnv) and 256 CUs, checks the plan's contracts and prints one JSON line: the return
//                             code, the path (elimination, accumulation, solve, back-substitution) and nr, dmax, pmax, widest — the
//                             Python test holds it against tests/marker_step_accuracy.py's expected_path and structure.
//       FILE: "C T M variant loss N" | "nconst block..." | "nsubset (block mask)..." | "npriors block..." | N x "camera time marker"
//   marker_plan_driver        the cases that reference does not express, built here: subset masks, priors, n_r = 0, a constant time, a
//                             time without slots, the three unsupported returns, 8 and 256 CUs, RSBA_MT_CHUNKS against T.
// Every plan goes through CheckPlan: the contracts the kernels rely on.  A violated check ends the program with a non-zero status.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <set>
#include <string>

#include "ba_marker_plan.hpp"

using namespace rsba;

static long g_checks = 0;
static std::string g_case;
#define CHECK(cond)                                                                                                        \
  do {                                                                                                                     \
    ++g_checks;                                                                                                            \
    if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_case.c_str()); exit(1); }       \
  } while (0)

// variant 0: Main_Calibration's wiring (camera 0 and marker 0 are the base blocks), 1: Test2's (marker 0 free).  keep(t, c, m): observed.
static rsba_problem MakeProblem(int C, int T, int M, int variant, const std::function<bool(int, int, int)>& keep) {
  rsba_problem p;
  p.model = variant == 1 ? RSBA_MODEL_MARKER_CHAIN_TEST2 : RSBA_MODEL_MARKER_CHAIN;
  p.num_cameras = C; p.num_times = T; p.num_markers = M; p.marker_side = 0.1;
  // (camera-major inside a time, the times interleaved: the plan's stable sort by time has work to do)
  for (int c = 0; c < C; ++c) for (int t = 0; t < T; ++t) for (int m = 0; m < M; ++m) if (keep(t, c, m)) {
    p.camera_index.push_back(c); p.time_index.push_back(t); p.marker_index.push_back(m);
  }
  p.num_observations = (int64_t)p.camera_index.size();
  p.observations.resize(8 * p.camera_index.size());
  for (size_t i = 0; i < p.observations.size(); ++i) p.observations[i] = (double)i;
  p.parameters.assign(6 * (size_t)(C + T + M), 0.0);
  p.intrinsics.assign(4 * (size_t)C, 1.0);
  return p;
}
static bool All(int, int, int) { return true; }
static void SetConstant(rsba_problem& p, int block) { p.block_constant.resize(p.num_cameras + p.num_times + p.num_markers, 0); p.block_constant[block] = 1; }
static void SetSubset(rsba_problem& p, int block, int mask) { p.block_subset.resize(p.num_cameras + p.num_times + p.num_markers, 0); p.block_subset[block] = (uint8_t)mask; }

static const char* AccName(const MarkerPlan& P) { return !P.split ? "" : P.acc_tiles == 3 ? "mfma3" : P.acc_tiles == 8 ? "mfma8" : P.lds_s ? "valu_lds" : "valu_mem"; }
static const char* SolveName(const MarkerPlan& P) { return P.nr == 0 ? "none" : P.nr > RSBA_CHOL_MAXN ? "multi" : P.solve_lds ? "lds" : "panel"; }
static const char* BacksubName(const MarkerPlan& P) { return P.split_backsub ? "split" : P.backsub_wg ? "wg" : "terms"; }

// The contracts the kernels rely on, from the problem alone: nothing here reads the planner's intermediate tables.
static void CheckPlan(const rsba_problem& p, bool loss, int cus, const MarkerSwitches& sw, const MarkerPlan& P) {
  const MarkerTables& B = P.tab;
  const int C = p.num_cameras, Tn = p.num_times, N = P.N, T = P.T, G = P.G;
  auto is_const = [&](int block) { return block < (int)p.block_constant.size() && p.block_constant[block] != 0; };
  CHECK(N == (int)p.num_observations && P.nfull == 6 * (C + Tn + p.num_markers) && P.with_loss == loss);
  // ---- the order: a stable sort by time; the observations travel with it
  CHECK((int)P.order.size() == N && (int)B.hmo.size() == N && (int)B.hts.size() == N && B.hobs.size() == 8 * (size_t)N);
  {
    std::vector<char> seen(N, 0);
    for (int k = 0; k < N; ++k) {
      const int i = P.order[k];
      CHECK(i >= 0 && i < N && !seen[i]);
      seen[i] = 1;
      if (k > 0) CHECK(p.time_index[P.order[k - 1]] < p.time_index[i] || (p.time_index[P.order[k - 1]] == p.time_index[i] && P.order[k - 1] < i));
      for (int q = 0; q < 8; ++q) CHECK(B.hobs[8 * (size_t)k + q] == p.observations[8 * (size_t)i + q]);
    }
  }
  // ---- offsets and counts
  auto monotone = [](const std::vector<int>& v, size_t size, int total) {
    if (v.size() != size || v.front() != 0 || v.back() != total) return false;
    for (size_t i = 1; i < v.size(); ++i) if (v[i] < v[i - 1]) return false;
    return true;
  };
  CHECK(T > 0 && monotone(B.tptr, T + 1, N) && monotone(B.sptr, T + 1, (int)B.scol.size()) && monotone(B.csptr, T + 1, (int)B.csfull.size()));
  CHECK(G >= 1 && G <= T && monotone(B.cptr, G + 1, T));
  for (int g = 0; g < G; ++g) CHECK(B.cptr[g] < B.cptr[g + 1]);   // no empty chunk
  CHECK((int)B.tfull.size() == T && (int)B.htc.size() == T && (int)B.htflags.size() == T && (int)B.cf.size() == P.nr && (int)B.hrmask.size() == P.nr / 6);
  // ---- times: ascending, each with its residual blocks; flags
  bool any_tconst = false, any_mask = false;
  for (int t = 0; t < T; ++t) {
    CHECK(B.tptr[t] < B.tptr[t + 1]);
    if (t > 0) CHECK(B.tfull[t - 1] < B.tfull[t]);
    const int blk = B.tfull[t] / 6;
    CHECK(B.tfull[t] % 6 == 0 && blk >= C && blk < C + Tn);
    CHECK(B.htc[t] == (is_const(blk) ? 1 : 0));
    CHECK(B.htflags[t] == (is_const(blk) ? 1 : p.subset_mask(blk) << 8));
    any_tconst = any_tconst || B.htc[t]; any_mask = any_mask || (B.htflags[t] >> 8) != 0;
  }
  // ---- per-time slots and columns
  int dmax = 0, pmax = 0, widest = 0;
  std::vector<char> col_seen(P.nr / 6 + 1, 0);
  std::set<int> cposes;
  for (int t = 0; t < T; ++t) {
    const int ns = B.sptr[t + 1] - B.sptr[t], ncs = B.csptr[t + 1] - B.csptr[t];
    for (int s = 1; s < ns; ++s) CHECK(B.scol[B.sptr[t] + s - 1] < B.scol[B.sptr[t] + s]);
    for (int s = 1; s < ncs; ++s) CHECK(B.csfull[B.csptr[t] + s - 1] < B.csfull[B.csptr[t] + s]);
    std::vector<char> slot_used(ns, 0), cslot_used(ncs, 0);
    for (int k = B.tptr[t]; k < B.tptr[t + 1]; ++k) {
      const int i = P.order[k];
      const MarkerObs& o = B.hmo[k];
      const TimeSlots& s = B.hts[k];
      CHECK(o.full_time == B.tfull[t] && o.full_time == 6 * p.time_block(i) && o.camera == p.camera_index[i] && s.camera == o.camera && o.pad == 0 && s.pad == 0);
      CHECK(o.full_cam == (p.uses_camera(i) ? 6 * p.camera_block(i) : -1) && o.full_marker == (p.uses_marker(i) ? 6 * p.marker_block(i) : -1));
      const int slot[2] = {s.slot_cam, s.slot_marker}, col[2] = {s.col_cam, s.col_marker}, full[2] = {o.full_cam, o.full_marker};
      for (int r = 0; r < 2; ++r) {
        if (slot[r] >= 0) {
          // a free slot of its time, whose column is the block's and maps back to the block
          CHECK(slot[r] < ns && B.scol[B.sptr[t] + slot[r]] == col[r] && col[r] >= 0 && col[r] % 6 == 0 && col[r] < P.nr);
          for (int q = 0; q < 6; ++q) CHECK(B.cf[col[r] + q] == full[r] + q);
          CHECK(!is_const(full[r] / 6));
          slot_used[slot[r]] = 1; col_seen[col[r] / 6] = 1;
        } else if (slot[r] <= -2) {
          const int j = -2 - slot[r];
          CHECK(j < ncs && B.csfull[B.csptr[t] + j] == full[r] && col[r] == -1 && is_const(full[r] / 6));
          cslot_used[j] = 1; cposes.insert(full[r]);
        } else {
          CHECK(slot[r] == -1 && col[r] == -1 && full[r] == -1);
        }
      }
    }
    for (char u : slot_used) CHECK(u);    // no slot without a residual block
    for (char u : cslot_used) CHECK(u);
    dmax = std::max(dmax, 6 * ns); pmax = std::max(pmax, ns + ncs); widest = std::max(widest, B.tptr[t + 1] - B.tptr[t]);
  }
  for (int j = 0; j < P.nr / 6; ++j) CHECK(col_seen[j]);   // every reduced block is one some residual uses
  for (int j = 1; j < P.nr / 6; ++j) CHECK(B.cf[6 * (j - 1)] < B.cf[6 * j]);   // cameras first, ascending
  CHECK(P.dmax == dmax && P.pmax == pmax && P.widest == widest && 6 * P.pmax <= RSBA_MT_MAXD);
  CHECK(P.ncpose == (int)cposes.size() && (int)B.hcpose.size() == P.ncpose && std::set<int>(B.hcpose.begin(), B.hcpose.end()) == cposes && B.cpf.size() == 6 * cposes.size());
  for (int k = 0; k < P.ncpose; ++k) for (int q = 0; q < 6; ++q) CHECK(B.cpf[6 * (size_t)k + q] == (q == 0 ? B.hcpose[k] : 0));
  // ---- flags of the reduced blocks: the problem's masks
  for (int j = 0; j < P.nr / 6; ++j) { CHECK(B.hrmask[j] == p.subset_mask(B.cf[6 * j] / 6)); any_mask = any_mask || B.hrmask[j] != 0; }
  CHECK(P.with_subset == any_mask && P.has_const == (any_mask || any_tconst || P.ncpose > 0) && P.with_dist == p.has_distortion());
  // ---- prior columns: -1 exactly for blocks that are constant as a whole
  CHECK(B.pcols.size() == p.block_priors.size() && P.np == (p.block_priors.empty() ? 0 : 1));
  {
    size_t k = 0;
    for (const auto& kv : p.block_priors) {
      if (is_const(kv.first)) CHECK(B.pcols[k] == -1);
      else CHECK(B.pcols[k] >= 0 && B.pcols[k] < P.nr && B.cf[B.pcols[k]] == 6 * kv.first);
      ++k;
    }
  }
  // ---- the split elimination's tables
  if (P.split) {
    const int nslots = (int)B.scol.size(), nx = P.nx;
    CHECK(P.nslots == nslots && (int)B.h_slot_time.size() == nslots && (int)B.h_order.size() == nslots && monotone(B.h_sb_ptr, nslots + 1, (int)B.h_sb_blk.size()));
    int ncam_cols = 0;
    for (int j = 0; j < P.nr / 6; ++j) if (B.cf[6 * j] < 6 * C) ncam_cols += 6;
    CHECK(P.ncam_cols == ncam_cols);
    // every residual block once in the list of each free slot it touches, in block order, with the other block's pose
    std::vector<int> hits(N, 0);
    for (int S = 0; S < nslots; ++S) {
      const int t = B.h_slot_time[S];
      CHECK(t >= 0 && t < T && S >= B.sptr[t] && S < B.sptr[t + 1]);
      for (int e = B.h_sb_ptr[S]; e < B.h_sb_ptr[S + 1]; ++e) {
        const BlockRef& r = B.h_sb_blk[e];
        CHECK(r.x >= B.tptr[t] && r.x < B.tptr[t + 1] && r.z == B.hts[r.x].camera && r.w == 0);
        if (e > B.h_sb_ptr[S]) CHECK(B.h_sb_blk[e - 1].x < r.x);
        const bool cam = B.hts[r.x].slot_cam == S - B.sptr[t], mar = B.hts[r.x].slot_marker == S - B.sptr[t];
        CHECK(cam != mar);
        const int other = cam ? B.hmo[r.x].full_marker : B.hmo[r.x].full_cam;
        CHECK(r.y == (other >= 0 ? other / 6 : -1));
        ++hits[r.x];
      }
    }
    for (int k = 0; k < N; ++k) CHECK(hits[k] == (B.hts[k].slot_cam >= 0) + (B.hts[k].slot_marker >= 0));
    // slot_order: a permutation, camera columns first, longer lists first
    {
      std::vector<char> seen(nslots, 0);
      auto len = [&](int S) { return B.h_sb_ptr[S + 1] - B.h_sb_ptr[S]; };
      for (int q = 0; q < nslots; ++q) {
        const int S = B.h_order[q];
        CHECK(S >= 0 && S < nslots && !seen[S]);
        seen[S] = 1;
        if (q > 0) {
          const int R = B.h_order[q - 1];
          const bool cr = B.scol[R] < ncam_cols, cs = B.scol[S] < ncam_cols;
          CHECK(cr || !cs);
          if (cr == cs) CHECK(len(R) >= len(S));
        }
      }
    }
    // the camera x marker items: per chunk, sorted by (camera column, marker column), every block with both blocks free exactly once
    CHECK((int)B.h_xi_cc.size() == nx && (int)B.h_xi_cm.size() == nx && monotone(B.h_xi_ptr, nx + 1, (int)B.h_xi_blk.size()) && monotone(B.h_xc_ptr, G + 1, nx));
    std::vector<int> xhits(N, 0);
    for (int g = 0; g < G; ++g)
      for (int it = B.h_xc_ptr[g]; it < B.h_xc_ptr[g + 1]; ++it) {
        CHECK(B.h_xi_ptr[it] < B.h_xi_ptr[it + 1]);
        if (it > B.h_xc_ptr[g]) CHECK(std::make_pair(B.h_xi_cc[it - 1], B.h_xi_cm[it - 1]) < std::make_pair(B.h_xi_cc[it], B.h_xi_cm[it]));
        for (int e = B.h_xi_ptr[it]; e < B.h_xi_ptr[it + 1]; ++e) {
          const BlockRef& r = B.h_xi_blk[e];
          CHECK(r.x >= B.tptr[B.cptr[g]] && r.x < B.tptr[B.cptr[g + 1]] && B.hts[r.x].col_cam == B.h_xi_cc[it] && B.hts[r.x].col_marker == B.h_xi_cm[it]);
          CHECK(r.y == B.hmo[r.x].full_time / 6 && r.z == B.hts[r.x].camera && r.w == 0);
          if (e > B.h_xi_ptr[it]) CHECK(B.h_xi_blk[e - 1].x < r.x);
          ++xhits[r.x];
        }
      }
    for (int k = 0; k < N; ++k) CHECK(xhits[k] == (B.hts[k].col_cam >= 0 && B.hts[k].col_marker >= 0 ? 1 : 0));
    // x_order: every item once; ten blocks or more: the lane pair 4 it + 2, 4 it + 3
    {
      std::vector<int> seen(nx, 0);
      CHECK(P.nx_threads == (int)B.h_xorder.size());
      for (size_t q = 0; q < B.h_xorder.size(); ++q) {
        const int v = B.h_xorder[q], it = v / 4, lanes = v % 4;
        CHECK(it >= 0 && it < nx);
        const bool shared = B.h_xi_ptr[it + 1] - B.h_xi_ptr[it] >= 10;
        if (lanes == 2) { CHECK(shared && q + 1 < B.h_xorder.size() && B.h_xorder[q + 1] == v + 1); ++seen[it]; }
        else if (lanes == 3) CHECK(shared && q > 0 && B.h_xorder[q - 1] == v - 1);
        else { CHECK(lanes == 0 && !shared); ++seen[it]; }
      }
      for (int it = 0; it < nx; ++it) CHECK(seen[it] == 1);
    }
    CHECK(P.lds_acc > 0 && P.lds_acc <= RSBA_LDS_CAP && P.fork == sw.fork);
    if (P.acc_tiles > 0) CHECK(sw.acc_mfma && P.lds_s && (P.acc_tiles == 3 ? P.acc_tb == 2 : P.acc_tiles == 8 && P.acc_tb == 1) && (AccMfmaTiles(P.nr) + 15) / 16 <= P.acc_tiles);
  } else {
    CHECK(!P.with_loss && !P.with_subset && P.acc_tiles == 0 && B.h_sb_blk.empty() && B.h_xi_blk.empty() && !P.fork && P.lds_elim > 0);
  }
  // ---- the path
  if (P.with_loss || P.with_subset) CHECK(P.split && !P.backsub_wg);
  if (P.with_subset) CHECK(P.split_backsub);
  if (P.split_backsub) {
    CHECK(P.split && P.ncand_wg == (N + 255) / 256 && P.nb_time == T + P.ncand_wg && (int)B.h_bt.size() == N);
    for (int t = 0; t < T; ++t) for (int k = B.tptr[t]; k < B.tptr[t + 1]; ++k) CHECK(B.h_bt[k] == t);
  } else {
    CHECK(P.ncand_wg == 0 && P.nb_time == (P.backsub_wg ? T : (T + 3) / 4) && B.h_bt.empty());
  }
  if (P.backsub_wg) CHECK(P.widest <= 128 && sw.backsub_wg);
  CHECK(P.lds_bw == (size_t)(P.pmax + 1) * 50 * sizeof(double));
  // chunks: one per CU (or RSBA_MT_CHUNKS) where the chunk sums live in LDS
  if (P.lds_s) CHECK(G <= (sw.chunks > 0 ? sw.chunks : cus));
  else CHECK(G <= 1024);
  // the reduced solve
  if (P.nr == 0) CHECK(!P.solve_lds && P.lds_solve == 0 && P.tc_tiles == 0 && P.nslots == 0 && P.nx == 0);
  else if (P.nr <= RSBA_CHOL_MAXN) {
    CHECK(P.lds_solve >= 32 * 1024 && P.lds_solve <= RSBA_LDS_CAP && P.tc_tiles == 0 && P.lds_solve_lds == MarkerSolveLdsDoubles(P.nr) * sizeof(double));
    CHECK(P.solve_lds == (sw.solve_lds && P.nr <= 160 && P.lds_solve_lds <= RSBA_LDS_CAP));
  } else {
    const int m = (P.nr + 31) / 32 * 32, nrt = (m + 1 + 63) / 64, ntiles = nrt * (nrt + 1) / 2;
    CHECK(!P.solve_lds && P.lds_finish >= 32 * 1024 && P.lds_finish <= RSBA_LDS_CAP);
    if (!sw.chol_tiles || ntiles > 2 * cus) CHECK(P.tc_tiles == 0 && B.tc_map.empty() && P.tc_flags == 0 && P.tc_hand == 0);
    else {
      CHECK(P.tc_tiles == ntiles && P.tc_nrt == nrt && P.tc_np == m / 32 && P.tc_flags == (size_t)P.tc_np * (nrt + 1) + 1 && P.tc_hand == (size_t)2 * nrt * kTileHandDoubles);
      std::set<int> tiles(B.tc_map.begin(), B.tc_map.end());
      CHECK((int)B.tc_map.size() == ntiles && (int)tiles.size() == ntiles);
      for (int v : B.tc_map) CHECK((v >> 8) < nrt && (v & 255) <= (v >> 8));
    }
  }
}

struct Planned { int rc; MarkerPlan plan; };
static Planned Plan(const std::string& name, const rsba_problem& p, bool loss, int cus, const MarkerSwitches& sw) {
  g_case = name;
  Planned r;
  r.rc = PlanMarkerChain(p, loss, cus, sw, &r.plan);
  if (r.rc == RSBA_OK) CheckPlan(p, loss, cus, sw, r.plan);
  return r;
}

static int RunFile(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  int C, T, M, variant, loss, N, n;
  if (fscanf(f, "%d %d %d %d %d %d", &C, &T, &M, &variant, &loss, &N) != 6) { fclose(f); return 2; }
  rsba_problem p = MakeProblem(C, T, M, variant, [](int, int, int) { return false; });
  bool ok = fscanf(f, "%d", &n) == 1;
  for (int k = 0, b; ok && k < n; ++k) { ok = fscanf(f, "%d", &b) == 1 && b >= 0 && b < C + T + M; if (ok) SetConstant(p, b); }
  ok = ok && fscanf(f, "%d", &n) == 1;
  for (int k = 0, b, mask; ok && k < n; ++k) { ok = fscanf(f, "%d %d", &b, &mask) == 2 && b >= 0 && b < C + T + M; if (ok) SetSubset(p, b, mask); }
  ok = ok && fscanf(f, "%d", &n) == 1;
  for (int k = 0, b; ok && k < n; ++k) { ok = fscanf(f, "%d", &b) == 1 && b >= 0 && b < C + T + M; if (ok) p.block_priors[b] = std::array<double, 42>(); }
  for (int i = 0, c, t, m; ok && i < N; ++i) {
    ok = fscanf(f, "%d %d %d", &c, &t, &m) == 3 && c >= 0 && c < C && t >= 0 && t < T && m >= 0 && m < M;
    if (ok) { p.camera_index.push_back(c); p.time_index.push_back(t); p.marker_index.push_back(m); }
  }
  fclose(f);
  if (!ok) { fprintf(stderr, "malformed %s\n", path); return 2; }
  p.num_observations = N;
  p.observations.resize(8 * (size_t)N);
  for (size_t i = 0; i < p.observations.size(); ++i) p.observations[i] = (double)i;
  const Planned r = Plan(path, p, loss != 0, 256, MarkerSwitches::FromEnv());
  const MarkerPlan& P = r.plan;
  if (r.rc != RSBA_OK) printf("{\"rc\": %d}\n", r.rc);
  else printf("{\"rc\": 0, \"elim\": \"%s\", \"acc\": \"%s\", \"solve\": \"%s\", \"backsub\": \"%s\", \"nr\": %d, \"dmax\": %d, \"pmax\": %d, \"widest\": %d, \"G\": %d, \"T\": %d, \"loss\": %d}\n",
              P.split ? "split" : "k_time_eliminate", AccName(P), SolveName(P), BacksubName(P), P.nr, P.dmax, P.pmax, P.widest, P.G, P.T, (int)P.with_loss);
  return 0;
}

static MarkerSwitches Without(bool MarkerSwitches::*path) { MarkerSwitches sw; sw.*path = false; return sw; }

static void BuiltInCases() {
  const MarkerSwitches def, no_split = Without(&MarkerSwitches::split), no_split_backsub = Without(&MarkerSwitches::split_backsub);
  // ---- subset masks: one component constant on a camera, a time and a marker; the split paths are kept whatever the switches say
  for (int big = 0; big <= 1; ++big) {
    const int C = big ? 6 : 2, T = big ? 8 : 3, M = big ? 6 : 2;
    rsba_problem p = MakeProblem(C, T, M, 0, All);
    SetSubset(p, 1, 1 << 2); SetSubset(p, C + 1, 1 << 4); SetSubset(p, C + T + 1, 1 << 0);
    SetSubset(p, 0, 7);   // (a base block's mask is ignored)
    for (const MarkerSwitches* sw : {&def, &no_split, &no_split_backsub}) {
      if (!big && sw != &def) continue;
      const Planned r = Plan(big ? "subset 6x8x6" : "subset 2x3x2", p, false, 256, *sw);
      CHECK(r.rc == RSBA_OK && r.plan.with_subset && r.plan.has_const && r.plan.split && r.plan.split_backsub && !r.plan.backsub_wg && !r.plan.with_loss);
    }
    // the same masks on blocks that are constant as a whole: ignored
    SetConstant(p, 1); SetConstant(p, C + 1); SetConstant(p, C + T + 1);
    const Planned r = Plan("subset on constant blocks", p, false, 256, no_split);
    CHECK(r.rc == RSBA_OK && !r.plan.with_subset && r.plan.has_const && !r.plan.split);
  }
  // ---- priors: on a free block and on a block that is constant as a whole; a solver with priors is planned with loss = true
  {
    rsba_problem p = MakeProblem(3, 4, 3, 0, All);
    p.block_priors[1] = std::array<double, 42>(); p.block_priors[3 + 4 + 2] = std::array<double, 42>();
    SetConstant(p, 3 + 4 + 2);
    const Planned r = Plan("priors", p, true, 256, no_split);
    CHECK(r.rc == RSBA_OK && r.plan.np == 1 && r.plan.split && r.plan.tab.pcols.size() == 2 && r.plan.tab.pcols[0] == 0 && r.plan.tab.pcols[1] == -1);
  }
  // ---- n_r = 0: every camera and marker constant
  {
    rsba_problem p = MakeProblem(3, 4, 3, 0, All);
    for (int b : {1, 2, 3 + 4 + 1, 3 + 4 + 2}) SetConstant(p, b);
    for (const MarkerSwitches* sw : {&def, &no_split}) {
      const Planned r = Plan("n_r = 0", p, false, 256, *sw);
      CHECK(r.rc == RSBA_OK && r.plan.nr == 0 && r.plan.dmax == 0 && r.plan.pmax == 4 && r.plan.ncpose == 4 && !r.plan.solve_lds && r.plan.tc_tiles == 0 && r.plan.has_const);
    }
  }
  // ---- a constant time; a time seen only through the base camera and the base marker (no slot at all)
  {
    rsba_problem p = MakeProblem(3, 4, 3, 0, [](int t, int c, int m) { return t != 2 || (c == 0 && m == 0); });
    SetConstant(p, 3 + 1);
    for (const MarkerSwitches* sw : {&def, &no_split, &no_split_backsub}) {
      const Planned r = Plan("constant time, empty time", p, false, 256, *sw);
      CHECK(r.rc == RSBA_OK && r.plan.T == 4 && r.plan.has_const && r.plan.ncpose == 0 && r.plan.tab.htc[1] == 1 && r.plan.tab.sptr[2] == r.plan.tab.sptr[3] && r.plan.tab.tptr[3] - r.plan.tab.tptr[2] == 1);
    }
    // a time no observation names leaves the program
    rsba_problem q = MakeProblem(3, 4, 3, 0, [](int t, int, int) { return t != 2; });
    const Planned r = Plan("unused time", q, false, 256, def);
    CHECK(r.rc == RSBA_OK && r.plan.T == 3 && r.plan.tab.tfull[2] == 6 * (3 + 3));
  }
  // ---- the unsupported returns, in their order of precedence, and RSBA_ERR_ARG
  {
    rsba_problem none = MakeProblem(2, 2, 2, 0, [](int, int, int) { return false; });
    CHECK(Plan("no observations", none, false, 256, def).rc == RSBA_ERR_ARG);
    rsba_problem dup = MakeProblem(2, 2, 2, 0, All);
    dup.camera_index.push_back(1); dup.time_index.push_back(0); dup.marker_index.push_back(1);
    dup.num_observations += 1; dup.observations.resize(8 * (size_t)dup.num_observations, 0.0);
    CHECK(Plan("duplicate detection", dup, false, 256, def).rc == RSBA_ERR_UNSUPPORTED);
    // 86 cameras and 85 markers besides the base blocks in one time: 6 x 171 > 1020; one block fewer is planned, for k_time_eliminate
    rsba_problem wide = MakeProblem(87, 1, 86, 0, All);
    CHECK(Plan("171 blocks", wide, false, 256, def).rc == RSBA_ERR_UNSUPPORTED);
    rsba_problem fits = MakeProblem(86, 1, 86, 0, All);
    const Planned r170 = Plan("170 blocks", fits, false, 256, def);
    CHECK(r170.rc == RSBA_OK && r170.plan.pmax == 170 && !r170.plan.split && !r170.plan.backsub_wg);
    CHECK(Plan("170 blocks, loss", fits, true, 256, def).rc == RSBA_ERR_UNSUPPORTED);
    // 62 x 3 x 62, every detection seen: 122 blocks a time, too wide for the split accumulation
    rsba_problem p62 = MakeProblem(62, 3, 62, 0, All);
    CHECK(Plan("62x3x62 loss", p62, true, 256, def).rc == RSBA_ERR_UNSUPPORTED);
    const Planned r62 = Plan("62x3x62", p62, false, 256, def);
    CHECK(r62.rc == RSBA_OK && !r62.plan.split && r62.plan.pmax == 122 && r62.plan.nr == 6 * 122 && r62.plan.tc_tiles > 0);
    rsba_problem m62 = p62;
    SetSubset(m62, 5, 1);
    CHECK(Plan("62x3x62 subset", m62, false, 256, def).rc == RSBA_ERR_UNSUPPORTED);
    // ... and on a chip of 8 CUs its 78 tiles do not fit: the multi-launch factorisation
    const Planned r62s = Plan("62x3x62, 8 CUs", p62, false, 8, def);
    CHECK(r62s.rc == RSBA_OK && r62s.plan.tc_tiles == 0);
    CHECK(Plan("62x3x62, RSBA_CHOL_TILES=0", p62, false, 256, Without(&MarkerSwitches::chol_tiles)).plan.tc_tiles == 0);
  }
  // ---- chunks: one per CU, or RSBA_MT_CHUNKS; every time equally heavy, so G = min(T, cap) after compaction
  for (int T : {3, 24, 60}) {
    const rsba_problem p = MakeProblem(3, T, 4, 0, All);
    for (int cus : {8, 256}) {
      const Planned r = Plan("CUs", p, false, cus, def);
      CHECK(r.rc == RSBA_OK && r.plan.lds_s && r.plan.G == std::min(T, cus));
    }
    for (int chunks : {1, 7, 1000}) {
      MarkerSwitches sw; sw.chunks = chunks;
      const Planned r = Plan("RSBA_MT_CHUNKS", p, false, 256, sw);
      CHECK(r.rc == RSBA_OK && r.plan.lds_s && r.plan.G == std::min(T, chunks));
    }
  }
  // ---- every switch off at once, with a loss and without
  {
    MarkerSwitches off; off.split = off.acc_mfma = off.backsub_wg = off.split_backsub = off.fork = off.solve_lds = off.chol_tiles = false;
    const rsba_problem p = MakeProblem(8, 24, 12, 1, [](int t, int c, int m) { return (t + 2 * c + 3 * m) % 5 != 0; });
    const Planned a = Plan("all off", p, false, 256, off);
    CHECK(a.rc == RSBA_OK && !a.plan.split && !a.plan.split_backsub && !a.plan.backsub_wg && !a.plan.solve_lds && !a.plan.fork);
    const Planned b = Plan("all off, loss", p, true, 256, off);
    CHECK(b.rc == RSBA_OK && b.plan.split && b.plan.acc_tiles == 0 && !b.plan.split_backsub && !b.plan.backsub_wg && !b.plan.fork);
  }
}

int main(int argc, char** argv) {
  const int rc = argc > 1 ? RunFile(argv[1]) : (BuiltInCases(), 0);
  if (rc == 0) fprintf(stderr, "marker plan driver: ok, %ld checks\n", g_checks);
  return rc;
}
