// Stand-alone driver of csrc/ba_marker_plan.hpp with free intrinsics in the plan (PlanMarkerChain's last argument; schur_impl = 3):
// tests/test_marker_intr_plan_host.py builds it with -fsanitize=address,undefined and runs it as a child process.  Every case is built
// here; a violated check ends the program with a non-zero status.  Contracts: the column order, the third slot of every residual
// block, ascending slot lists, every (residual block, pair kind) in exactly one pair item of its chunk, the held components, the width
// refusals, and byte-identical tables where no mask is set or the caller does not ask.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <string>

#include "ba_marker_plan.hpp"

using namespace rsba;

static long g_checks = 0;
static std::string g_case;
#define CHECK(...)                                                                                                                \
  do {                                                                                                                            \
    ++g_checks;                                                                                                                   \
    if (!(__VA_ARGS__)) { fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #__VA_ARGS__, g_case.c_str()); exit(1); } \
  } while (0)

// variant 0: Main_Calibration's wiring (camera 0 and marker 0 are the base blocks), 1: Test2's (marker 0 free).  keep(t, c, m): observed.
static rsba_problem MakeProblem(int C, int T, int M, int variant, const std::function<bool(int, int, int)>& keep) {
  rsba_problem p;
  p.model = variant == 1 ? RSBA_MODEL_MARKER_CHAIN_TEST2 : RSBA_MODEL_MARKER_CHAIN;
  p.num_cameras = C; p.num_times = T; p.num_markers = M; p.marker_side = 0.1;
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
static void SetMasks(rsba_problem& p, const std::vector<int>& masks) {
  p.intrinsics_free.assign((size_t)p.num_cameras, 0);
  for (size_t k = 0; k < masks.size(); ++k) p.intrinsics_free[k] = (uint8_t)masks[k];
}
static void SetConstant(rsba_problem& p, int block) { p.block_constant.resize(p.num_cameras + p.num_times + p.num_markers, 0); p.block_constant[block] = 1; }

template <typename V> static bool SameBytes(const std::vector<V>& a, const std::vector<V>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(V)) == 0);
}
// every table and every scalar of two plans
static void CheckSame(const MarkerPlan& X, const MarkerPlan& Y) {
  const MarkerTables &A = X.tab, &B = Y.tab;
  CHECK(SameBytes(A.hmo, B.hmo) && SameBytes(A.hts, B.hts) && SameBytes(A.hobs, B.hobs) && SameBytes(A.tptr, B.tptr) && SameBytes(A.sptr, B.sptr) && SameBytes(A.scol, B.scol));
  CHECK(SameBytes(A.csptr, B.csptr) && SameBytes(A.csfull, B.csfull) && SameBytes(A.tfull, B.tfull) && SameBytes(A.cf, B.cf) && SameBytes(A.htc, B.htc) && SameBytes(A.htflags, B.htflags));
  CHECK(SameBytes(A.hrmask, B.hrmask) && SameBytes(A.hcpose, B.hcpose) && SameBytes(A.cpf, B.cpf) && SameBytes(A.cptr, B.cptr) && SameBytes(A.h_slot_time, B.h_slot_time));
  CHECK(SameBytes(A.h_sb_ptr, B.h_sb_ptr) && SameBytes(A.h_order, B.h_order) && SameBytes(A.h_xi_ptr, B.h_xi_ptr) && SameBytes(A.h_xi_cc, B.h_xi_cc) && SameBytes(A.h_xi_cm, B.h_xi_cm));
  CHECK(SameBytes(A.h_xc_ptr, B.h_xc_ptr) && SameBytes(A.h_xorder, B.h_xorder) && SameBytes(A.h_sb_blk, B.h_sb_blk) && SameBytes(A.h_xi_blk, B.h_xi_blk) && SameBytes(A.h_bt, B.h_bt));
  CHECK(SameBytes(A.pcols, B.pcols) && SameBytes(A.tc_map, B.tc_map) && SameBytes(X.order, Y.order));
  CHECK(A.hti.empty() && B.hti.empty() && A.h_is_slot.empty() && B.h_is_slot.empty() && A.h_ib_blk.empty() && B.h_ib_blk.empty() && A.h_xs_item.empty() && B.h_xs_item.empty() &&
        A.h_xs_ptr.empty() && B.h_xs_ptr.empty() && A.h_xs_src.empty() && B.h_xs_src.empty() && A.h_ib_ptr.empty() && B.h_ib_ptr.empty() && A.h_is_cam.empty() && B.h_is_cam.empty());
  CHECK(X.N == Y.N && X.T == Y.T && X.nr == Y.nr && X.nfull == Y.nfull && X.G == Y.G && X.dmax == Y.dmax && X.pmax == Y.pmax && X.ncpose == Y.ncpose && X.widest == Y.widest && X.np == Y.np);
  CHECK(X.with_loss == Y.with_loss && X.with_subset == Y.with_subset && X.has_const == Y.has_const && X.with_dist == Y.with_dist && !X.with_intr && !Y.with_intr);
  CHECK(X.split == Y.split && X.acc_tiles == Y.acc_tiles && X.acc_tb == Y.acc_tb && X.lds_s == Y.lds_s && X.solve_lds == Y.solve_lds && X.split_backsub == Y.split_backsub &&
        X.backsub_wg == Y.backsub_wg && X.fork == Y.fork && X.nb_time == Y.nb_time && X.ncand_wg == Y.ncand_wg);
  CHECK(X.nslots == Y.nslots && X.nx == Y.nx && X.ncam_cols == Y.ncam_cols && X.nx_threads == Y.nx_threads && X.nr_pose == X.nr && Y.nr_pose == Y.nr && X.nslots_pose == Y.nslots_pose &&
        (!X.split || X.nslots_pose == X.nslots) && X.nislots == 0 && Y.nislots == 0 && X.nib == 0 && X.nxs == 0);
  CHECK(X.lds_elim == Y.lds_elim && X.lds_acc == Y.lds_acc && X.lds_bw == Y.lds_bw && X.lds_solve_lds == Y.lds_solve_lds && X.lds_solve == Y.lds_solve && X.lds_finish == Y.lds_finish &&
        X.tc_np == Y.tc_np && X.tc_nrt == Y.tc_nrt && X.tc_tiles == Y.tc_tiles && X.tc_flags == Y.tc_flags && X.tc_hand == Y.tc_hand);
}

// The contracts of a plan with intrinsics blocks, from the problem alone.
static void CheckIntrPlan(const rsba_problem& p, const MarkerPlan& P) {
  const MarkerTables& B = P.tab;
  const int C = p.num_cameras, Tn = p.num_times, M = p.num_markers, N = P.N, T = P.T, G = P.G;
  auto is_const = [&](int block) { return block < (int)p.block_constant.size() && p.block_constant[block] != 0; };
  CHECK(P.with_intr && P.with_dist && P.split && P.split_backsub && !P.backsub_wg);
  // ---- column order: the free cameras' pose blocks, the markers', then one block per camera with a mask, ascending camera
  std::vector<char> used(C + M, 0), named(C, 0);
  for (int i = 0; i < N; ++i) {
    if (p.uses_camera(i)) used[p.camera_index[i]] = 1;
    if (p.uses_marker(i)) used[C + p.marker_index[i]] = 1;
    named[p.camera_index[i]] = 1;
  }
  std::vector<int> want_cf, icol(C, -1);
  std::vector<unsigned char> want_mask;
  for (int b = 0; b < C + M; ++b) {
    const int blk = b < C ? b : Tn + b;
    if (used[b] && !is_const(blk)) { for (int q = 0; q < 6; ++q) want_cf.push_back(6 * blk + q); want_mask.push_back((unsigned char)p.subset_mask(blk)); }
  }
  CHECK(P.nr_pose == (int)want_cf.size());
  bool any_held = false;
  for (int k = 0; k < C; ++k) if (p.intrinsics_free_mask(k) != 0) {
    CHECK(named[k]);
    icol[k] = (int)want_cf.size();
    for (int q = 0; q < 6; ++q) want_cf.push_back(P.nfull + 6 * k + q);
    want_mask.push_back((unsigned char)(~p.intrinsics_free_mask(k) & 0x3F));     // held components: the complement of the mask
    any_held = any_held || want_mask.back() != 0;
  }
  CHECK(P.nr == (int)want_cf.size() && B.cf == want_cf && B.hrmask == want_mask);
  if (any_held) CHECK(P.with_subset && P.has_const);
  // ---- the third slot, the slot lists
  CHECK((int)B.hti.size() == N && (int)B.h_slot_time.size() == P.nslots && P.nslots == (int)B.scol.size());
  int dmax = 0, nislots = 0;
  for (int t = 0; t < T; ++t) {
    const int s0 = B.sptr[t], ns = B.sptr[t + 1] - s0;
    for (int s = 1; s < ns; ++s) CHECK(B.scol[s0 + s - 1] < B.scol[s0 + s]);     // ascending: the intrinsics blocks land last
    std::vector<char> slot_used(ns, 0);
    for (int k = B.tptr[t]; k < B.tptr[t + 1]; ++k) {
      const int i = P.order[k];
      const IntrSlots& u = B.hti[k];
      const TimeSlots& s = B.hts[k];
      if (p.intrinsics_free_mask(p.camera_index[i]) == 0) CHECK(u.slot_intr == -1 && u.col_intr == -1);
      else {
        CHECK(u.col_intr == icol[p.camera_index[i]] && u.slot_intr >= 0 && u.slot_intr < ns && B.scol[s0 + u.slot_intr] == u.col_intr && u.col_intr >= P.nr_pose);
        slot_used[u.slot_intr] = 1;
      }
      if (s.slot_cam >= 0) { CHECK(s.slot_cam < ns && B.scol[s0 + s.slot_cam] == s.col_cam && s.col_cam < P.nr_pose); slot_used[s.slot_cam] = 1; }
      if (s.slot_marker >= 0) { CHECK(s.slot_marker < ns && B.scol[s0 + s.slot_marker] == s.col_marker && s.col_marker < P.nr_pose); slot_used[s.slot_marker] = 1; }
    }
    for (char v : slot_used) CHECK(v);
    for (int s = 0; s < ns; ++s) { CHECK(B.h_slot_time[s0 + s] == t); nislots += B.scol[s0 + s] >= P.nr_pose ? 1 : 0; }
    dmax = std::max(dmax, 6 * ns);
  }
  // ---- the widths count the intrinsics blocks
  CHECK(P.dmax == dmax && 6 * P.pmax <= RSBA_MT_MAXD && P.pmax >= dmax / 6 && P.lds_acc <= RSBA_LDS_CAP);
  if (P.acc_tiles > 0) CHECK(P.lds_acc == AccMfmaLdsBytes(P.nr, P.acc_tb) && AccMfmaTiles(P.nr) <= 16 * P.acc_tiles);
  else CHECK(P.lds_acc == AccLdsBytes(dmax, P.lds_s ? PartLayout{P.nr}.packed() + 3 * (size_t)P.nr : 0));
  // ---- the threads of k_mc_slot_products: the pose slots, each once; an intrinsics slot has no residual block in sb_blk
  CHECK((int)B.h_order.size() == P.nslots_pose && P.nslots_pose + nislots == P.nslots && P.nislots == nislots);
  {
    std::vector<char> seen(P.nslots, 0);
    for (int S : B.h_order) { CHECK(S >= 0 && S < P.nslots && !seen[S] && B.scol[S] < P.nr_pose); seen[S] = 1; }
    for (int S = 0; S < P.nslots; ++S) if (B.scol[S] >= P.nr_pose) CHECK(B.h_sb_ptr[S] == B.h_sb_ptr[S + 1]);
  }
  // ---- the intrinsics slots: every slot once, ascending; its residual blocks are the camera's at that time, in block order
  CHECK((int)B.h_is_slot.size() == nislots && (int)B.h_is_cam.size() == nislots && (int)B.h_ib_ptr.size() == nislots + 1 && (int)B.h_ib_blk.size() == P.nib && B.h_ib_ptr.back() == P.nib);
  std::vector<int> entry_of(N, -1), islot_of(N, -1);
  for (int j = 0; j < nislots; ++j) {
    const int S = B.h_is_slot[j], t = B.h_slot_time[S];
    if (j > 0) CHECK(B.h_is_slot[j - 1] < S);
    CHECK(B.scol[S] >= P.nr_pose && icol[B.h_is_cam[j]] == B.scol[S] && B.h_ib_ptr[j] < B.h_ib_ptr[j + 1]);
    int e = B.h_ib_ptr[j];
    for (int k = B.tptr[t]; k < B.tptr[t + 1]; ++k) if (B.hti[k].col_intr == B.scol[S]) {
      CHECK(e < B.h_ib_ptr[j + 1] && B.h_ib_blk[e] == k && B.hmo[k].camera == B.h_is_cam[j]);
      entry_of[k] = e; islot_of[k] = j; ++e;
    }
    CHECK(e == B.h_ib_ptr[j + 1]);
  }
  for (int k = 0; k < N; ++k) CHECK((entry_of[k] >= 0) == (B.hti[k].col_intr >= 0));
  // ---- pair items: every (residual block, kind) in exactly one item of its chunk; rows below columns
  CHECK((int)B.h_xc_ptr.size() == G + 1 && B.h_xc_ptr.back() == P.nx && (int)B.h_xi_cc.size() == P.nx && (int)B.h_xi_cm.size() == P.nx && (int)B.h_xi_ptr.size() == P.nx + 1);
  CHECK((int)B.h_xs_item.size() == P.nxs && (int)B.h_xs_ptr.size() == P.nxs + 1 && B.h_xs_ptr.back() == (int)B.h_xs_src.size());
  std::map<int, int> xs_of;
  for (int i = 0; i < P.nxs; ++i) { CHECK(xs_of.count(B.h_xs_item[i]) == 0); xs_of[B.h_xs_item[i]] = i; }
  std::vector<int> cover(3 * (size_t)N, 0), chunk_of_time(T, -1);
  for (int g = 0; g < G; ++g) for (int t = B.cptr[g]; t < B.cptr[g + 1]; ++t) chunk_of_time[t] = g;
  std::vector<int> time_of(N, -1);
  for (int t = 0; t < T; ++t) for (int k = B.tptr[t]; k < B.tptr[t + 1]; ++k) time_of[k] = t;
  for (int g = 0; g < G; ++g) {
    std::map<std::pair<int, int>, int> keys;
    for (int it = B.h_xc_ptr[g]; it < B.h_xc_ptr[g + 1]; ++it) {
      const int cc = B.h_xi_cc[it], cm = B.h_xi_cm[it];
      CHECK(cc >= 0 && cm > cc && cm + 6 <= P.nr && keys[{cm, cc}]++ == 0);      // the lower triangle; one item per pair and chunk
      if (B.h_xi_ptr[it] < B.h_xi_ptr[it + 1]) {
        CHECK(xs_of.count(it) == 0 && cm < P.nr_pose && cc < P.ncam_cols);
        for (int e = B.h_xi_ptr[it]; e < B.h_xi_ptr[it + 1]; ++e) {
          const int k = B.h_xi_blk[e].x;
          CHECK(k >= 0 && k < N && chunk_of_time[time_of[k]] == g && B.hts[k].col_cam == cc && B.hts[k].col_marker == cm);
          cover[3 * (size_t)k]++;
        }
      } else {
        CHECK(xs_of.count(it) == 1 && cm >= P.nr_pose && cc < P.nr_pose);
        const int i = xs_of[it];
        CHECK(B.h_xs_ptr[i] < B.h_xs_ptr[i + 1]);
        for (int e = B.h_xs_ptr[i]; e < B.h_xs_ptr[i + 1]; ++e) {
          const int src = B.h_xs_src[e];
          if (e > B.h_xs_ptr[i]) CHECK(B.h_xs_src[e - 1] < src);      // a fixed order: ascending = time order
          CHECK(src >= 0 && src < nislots + P.nib);
          if (src < nislots) {
            CHECK(cc < P.ncam_cols && B.scol[B.h_is_slot[src]] == cm && chunk_of_time[B.h_slot_time[B.h_is_slot[src]]] == g);
            bool any = false;
            for (int q = B.h_ib_ptr[src]; q < B.h_ib_ptr[src + 1]; ++q) if (B.hts[B.h_ib_blk[q]].col_cam >= 0) { CHECK(B.hts[B.h_ib_blk[q]].col_cam == cc); cover[3 * (size_t)B.h_ib_blk[q] + 1]++; any = true; }
            CHECK(any);
          } else {
            const int k = B.h_ib_blk[src - nislots];
            CHECK(cc >= P.ncam_cols && B.hts[k].col_marker == cc && B.hti[k].col_intr == cm && chunk_of_time[time_of[k]] == g);
            cover[3 * (size_t)k + 2]++;
          }
        }
      }
    }
  }
  for (int k = 0; k < N; ++k) {
    const TimeSlots& s = B.hts[k];
    const int ci = B.hti[k].col_intr;
    CHECK(cover[3 * (size_t)k] == (s.col_cam >= 0 && s.col_marker >= 0 ? 1 : 0));
    CHECK(cover[3 * (size_t)k + 1] == (s.col_cam >= 0 && ci >= 0 ? 1 : 0));
    CHECK(cover[3 * (size_t)k + 2] == (s.col_marker >= 0 && ci >= 0 ? 1 : 0));
  }
  // ---- the threads of k_mc_cross: the items with residual blocks of their own, each on one lane or on two
  {
    std::vector<int> lanes(P.nx, 0);
    CHECK((int)B.h_xorder.size() == P.nx_threads);
    for (int code : B.h_xorder) { const int it = code >> 2; CHECK(it >= 0 && it < P.nx && B.h_xi_ptr[it] < B.h_xi_ptr[it + 1]); lanes[it]++; }
    for (int it = 0; it < P.nx; ++it) CHECK(lanes[it] == (B.h_xi_ptr[it] < B.h_xi_ptr[it + 1] ? (B.h_xi_ptr[it + 1] - B.h_xi_ptr[it] >= 10 ? 2 : 1) : 0));
  }
  // ---- priors keep their columns (pose blocks only)
  for (int c : B.pcols) CHECK(c < P.nr_pose);
}

static MarkerPlan Plan(const rsba_problem& p, bool loss, int cus, const MarkerSwitches& sw, bool intr, int want_rc = RSBA_OK) {
  MarkerPlan P;
  const int rc = intr ? PlanMarkerChain(p, loss, cus, sw, &P, true) : PlanMarkerChain(p, loss, cus, sw, &P);
  CHECK(rc == want_rc);
  return P;
}

static void Case(const char* name, rsba_problem p, const std::vector<int>& masks, bool loss = false, MarkerSwitches sw = MarkerSwitches(), int cus = 256) {
  g_case = name;
  // without the opt-in, and with no mask set: today's plan, byte for byte
  rsba_problem bare = p;
  bare.intrinsics_free.clear();
  const MarkerPlan base = Plan(bare, loss, cus, sw, false);
  rsba_problem zero = p;
  SetMasks(zero, std::vector<int>(p.num_cameras, 0));
  CheckSame(base, Plan(zero, loss, cus, sw, true));
  SetMasks(p, masks);
  CheckSame(base, Plan(p, loss, cus, sw, false));
  const MarkerPlan P = Plan(p, loss, cus, sw, true);
  CheckIntrPlan(p, P);
  int nblocks = 0;
  for (int m : masks) nblocks += m != 0 ? 1 : 0;
  CHECK(P.nr == base.nr + 6 * nblocks && P.T == base.T && P.tab.cptr.size() >= 2);
}

int main() {
  MarkerSwitches off;   // the switches this path ignores
  off.split = false; off.split_backsub = false; off.backsub_wg = false;
  MarkerSwitches chunks3; chunks3.chunks = 3;
  Case("3x12x4 3f", MakeProblem(3, 12, 4, 0, All), {0x3F, 0x3F, 0x3F});
  Case("3x12x4 mixed", MakeProblem(3, 12, 4, 0, All), {0x0F, 0, 0x33});
  Case("3x12x4 mixed, switches off", MakeProblem(3, 12, 4, 0, All), {0x0F, 0, 0x33}, false, off);
  Case("3x12x4 3f, three chunks", MakeProblem(3, 12, 4, 0, All), {0x3F, 0x3F, 0x3F}, false, chunks3);
  Case("3x12x4 3f, a loss, 8 CUs", MakeProblem(3, 12, 4, 0, All), {0x3F, 0x3F, 0x3F}, true, MarkerSwitches(), 8);
  {
    rsba_problem p = MakeProblem(3, 12, 4, 0, All);
    SetConstant(p, 1);      // a constant camera pose with a free block
    Case("3x12x4 camera 1 constant", p, {0x0F, 0x3F, 0x33});
    g_case = "3x12x4 camera 1 constant: the block has no camera item";
    SetMasks(p, {0x0F, 0x3F, 0x33});
    const MarkerPlan P = Plan(p, false, 256, MarkerSwitches(), true);
    CHECK(P.nr == 42 && P.nr_pose == 24 && P.ncam_cols == 6);
    for (int i = 0; i < P.nxs; ++i) if (P.tab.h_xi_cm[P.tab.h_xs_item[i]] == 30) CHECK(P.tab.h_xi_cc[P.tab.h_xs_item[i]] >= P.ncam_cols);   // camera 1's block couples with markers only
  }
  Case("test2 wiring 3x12x4", MakeProblem(3, 12, 4, 1, All), {0x3F, 0x3F, 0x3F});
  Case("sparse detections 4x9x5", MakeProblem(4, 9, 5, 0, [](int t, int c, int m) { return (t + 2 * c + 3 * m) % 3 != 0; }), {0x3F, 0, 0x01, 0x30});
  Case("T = 1", MakeProblem(3, 1, 4, 0, All), {0x3F, 0x3F, 0x3F});
  Case("one camera", MakeProblem(1, 6, 4, 0, All), {0x3F});
  Case("one camera, T = 1", MakeProblem(1, 1, 3, 0, All), {0x03});
  Case("4x10x24 (mfma8)", MakeProblem(4, 10, 24, 0, All), {0x3F, 0x3F, 0x3F, 0x3F});
  Case("6x8x40 (valu, panel solve)", MakeProblem(6, 8, 40, 0, All), {0x0F, 0, 0x33, 0x3F, 0x03, 0x30});
  {
    g_case = "2x1400x2";
    rsba_problem p = MakeProblem(2, 1400, 2, 0, All);
    Case("2x1400x2", p, {0, 0x03});
    SetMasks(p, {0, 0x03});
    const MarkerPlan P = Plan(p, false, 256, MarkerSwitches(), true);
    CHECK(P.nr == 18 && 6 * (P.T + 2) + P.nr > 8192 && P.G <= 256);   // the dense system would have more than 8192 columns
  }
  {
    // a mask on a camera no observation names
    g_case = "unobserved camera";
    rsba_problem p = MakeProblem(3, 4, 3, 0, [](int, int c, int) { return c != 2; });
    SetMasks(p, {0x0F, 0, 0x01});
    Plan(p, false, 256, MarkerSwitches(), true, RSBA_ERR_UNSUPPORTED);
    SetMasks(p, {0x0F, 0, 0});
    CheckIntrPlan(p, Plan(p, false, 256, MarkerSwitches(), true));
  }
  {
    // a duplicated detection stays refused
    g_case = "duplicate";
    rsba_problem p = MakeProblem(3, 4, 3, 0, All);
    p.camera_index.push_back(p.camera_index[0]); p.time_index.push_back(p.time_index[0]); p.marker_index.push_back(p.marker_index[0]);
    p.observations.resize(p.observations.size() + 8, 0.0); p.num_observations++;
    SetMasks(p, {0x3F, 0x3F, 0x3F});
    Plan(p, false, 256, MarkerSwitches(), true, RSBA_ERR_UNSUPPORTED);
  }
  {
    // the width limit: one time, C cameras, M markers: (C - 1) + (M - 1) pose slots and C intrinsics slots.  The plan holds while the
    // split accumulation's records fit (AccLdsBytes over ALL slots) and the pose cache does (RSBA_MT_MAXD); one more marker: refused,
    // where the same problem without the blocks is still planned.
    g_case = "width limit";
    const int C = 8;
    int last_ok = -1;
    for (int M = 60; M < 200; ++M) {
      rsba_problem p = MakeProblem(C, 2, M, 0, All);
      SetMasks(p, std::vector<int>(C, 0x3F));
      MarkerPlan P;
      const int rc = PlanMarkerChain(p, false, 256, MarkerSwitches(), &P, true);
      const int slots = (C - 1) + (M - 1) + C, nr = 6 * slots;
      const size_t s_doubles = PartLayout{nr}.packed() + 3 * (size_t)nr;
      const bool fits = 6 * slots <= RSBA_MT_MAXD && std::min(AccLdsBytes(6 * slots, 0), AccLdsBytes(6 * slots, s_doubles)) <= RSBA_LDS_CAP;
      CHECK((rc == RSBA_OK) == fits && (rc == RSBA_OK || rc == RSBA_ERR_UNSUPPORTED));
      if (rc == RSBA_OK) { CHECK(last_ok == M - 1 || last_ok == -1); last_ok = M; CHECK(P.dmax == 6 * slots); if (M % 16 == 0) CheckIntrPlan(p, P); }
      else {
        CHECK(last_ok == M - 1);
        rsba_problem bare = p;
        bare.intrinsics_free.clear();
        MarkerPlan Q;
        CHECK(PlanMarkerChain(bare, false, 256, MarkerSwitches(), &Q) == RSBA_OK && Q.dmax == 6 * (slots - C));   // the blocks are what no longer fits
        {
          rsba_problem q = MakeProblem(C, 2, last_ok, 0, All);
          SetMasks(q, std::vector<int>(C, 0x3F));
          CheckIntrPlan(q, Plan(q, false, 256, MarkerSwitches(), true));      // the time AT the limit
        }
        break;
      }
    }
    CHECK(last_ok > 60 && last_ok < 199);
  }
  fprintf(stderr, "marker intr plan driver: ok (%ld checks)\n", g_checks);
  return 0;
}
