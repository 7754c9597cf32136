// Stand-alone check of the planar marker's second pose (csrc/ba_marker_pose.hpp: MirrorMarkerPose, SecondMarkerPose, FitMarkerPoseBoth; the
// C entry rsba_marker_pose_from_corners_both; include/rsba/correspondencer.h EstimatePoseSingleMarkerBoth) and of the block resection with
// both solutions among a block's candidates (csrc/ba_resection.hpp, kBoth), built with -fsanitize=address,undefined by
// tests/test_marker_pose_both_host.py and run as a program:
//   fit FILE     one detection per line — fx fy ppx ppy, has_dist, k1 k2 p1 p2 k3, side, the eight corner values.  FitMarkerPoseBoth on each;
//                checked here: solution 0 is FitMarkerPose's and rsba_marker_pose_from_corners' bits, the C entry and the C++ mirror return
//                the header routine's bits, statuses 2 and 3 come with pose zeros and RMS -1.  Printed per line as JSON for the test: both
//                poses, RMS and statuses, MirrorMarkerPose of solution 0, how far the mirror of the mirror is from each solution, det R'.
//   start FILE   one problem in tests/scene_start_driver.cpp's format: "all_markers C T M N has_dist side sweeps has_known", intrinsics,
//                coefficients, parameters, flags, then N lines "camera time marker" + eight corner values; then "K" and K lines
//                "block v0 .. v5": blocks (indices into [C | T | M]) to be refitted from the given value afterwards.  The whole scene start
//                runs serially twice, without and with both solutions: FitMarkerPoseBoth per detection, then every launch of the plan
//                block by block through ResectBlock<kBoth>, summing in observation order.  Checked here: every chosen start's block cost
//                with both solutions is not higher than without while the two runs still hold the same blocks.  Printed: blocks,
//                statuses, RMS, each block's chosen start cost for both runs, and the refits from the given values.
//   (no argument)   the argument checks of rsba_marker_pose_from_corners_both.
// With -DRSBA_DRIVER_HEADERS_ONLY the C entries and the C++ mirror are left out and the program needs the three headers alone: what the GPU
// tests build for `start`, the serial host path their device results are held to.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "ba_marker_pose.hpp"
#include "ba_resection.hpp"
#include "ba_scene_start_plan.hpp"
#ifndef RSBA_DRIVER_HEADERS_ONLY
#include "ba_problem.hpp"
#include "rsba.h"
#include "rsba/correspondencer.h"

namespace rsba { int DeviceCount() { return 0; } }   // (the kernels are not in this build)
#endif

namespace {

int g_fail = 0;
void Expect(bool ok, const char* what, int where) {
  if (!ok) { ++g_fail; if (g_fail < 20) fprintf(stderr, "FAIL %s (%d)\n", what, where); }
}

double PoseDistance(const double* a, const double* b) {
  double Ra[9], Rb[9], ta[3], tb[3], d = 0.0;
  rsba::PoseRotationTranslation(a, Ra, ta); rsba::PoseRotationTranslation(b, Rb, tb);
  for (int i = 0; i < 9; ++i) d = std::fmax(d, std::fabs(Ra[i] - Rb[i]));
  for (int i = 3; i < 6; ++i) d = std::fmax(d, std::fabs(a[i] - b[i]));
  return d;
}

void PrintDoubles(const char* name, const double* v, size_t n, const char* tail) {
  printf("\"%s\": [", name);
  for (size_t k = 0; k < n; ++k) printf("%s%.17g", k ? ", " : "", v[k]);
  printf("]%s", tail);
}
void PrintInts(const char* name, const int32_t* v, size_t n, const char* tail) {
  printf("\"%s\": [", name);
  for (size_t k = 0; k < n; ++k) printf("%s%d", k ? ", " : "", v[k]);
  printf("]%s", tail);
}

int Fit(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  int id = 0;
  for (;; ++id) {
    double k4[4], k5[5], side, c8[8];
    int has_dist;
    int got = fscanf(f, "%lf %lf %lf %lf %d", &k4[0], &k4[1], &k4[2], &k4[3], &has_dist);
    if (got != 5) break;
    for (double& v : k5) got += fscanf(f, "%lf", &v);
    got += fscanf(f, "%lf", &side);
    for (double& v : c8) got += fscanf(f, "%lf", &v);
    if (got != 19) { fprintf(stderr, "malformed case file\n"); fclose(f); return 2; }
    const double* dist = has_dist ? k5 : nullptr;
    double poses[12], rms[2];
    int st[2];
    rsba::FitMarkerPoseBoth(c8, k4, dist, side, poses, rms, st);
    // solution 0: the single fit's bits, from the header routine and from the C entry
    double single[6], single_rms = 0.0;
    const int single_st = rsba::FitMarkerPose(c8, k4, dist, side, single, &single_rms);
    Expect(memcmp(single, poses, sizeof(single)) == 0 && single_rms == rms[0] && single_st == st[0], "solution 0 is FitMarkerPose", id);
#ifndef RSBA_DRIVER_HEADERS_ONLY
    double entry[6], entry_rms = 0.0;
    int32_t entry_st = -1;
    const int rc1 = rsba_marker_pose_from_corners(c8, k4, dist, side, entry, &entry_rms, &entry_st);
    Expect(memcmp(entry, poses, sizeof(entry)) == 0 && entry_rms == rms[0] && entry_st == st[0], "solution 0 is rsba_marker_pose_from_corners", id);
    // the C entry and the mirror
    double poses_c[12] = {7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7}, rms_c[2] = {7, 7};
    int32_t st_c[2] = {7, 7};
    const int rc2 = rsba_marker_pose_from_corners_both(c8, k4, dist, side, poses_c, rms_c, st_c);
    Expect(rc2 == rc1 && rc2 == (st[0] == rsba::MARKER_POSE_DEGENERATE ? RSBA_ERR_UNSUPPORTED : RSBA_OK), "return code", id);
    Expect(memcmp(poses_c, poses, sizeof(poses)) == 0 && rms_c[0] == rms[0] && rms_c[1] == rms[1] && st_c[0] == st[0] && st_c[1] == st[1], "C entry bits", id);
    Expect(rsba_marker_pose_from_corners_both(c8, k4, dist, side, poses_c, nullptr, nullptr) == rc2, "rms and status are optional", id);
    {
      std::vector<std::array<double, 5>> dv;
      if (dist) dv.push_back({{k5[0], k5[1], k5[2], k5[3], k5[4]}});
      RSCalibration::Correspondencer corr({{{k4[0], k4[1], k4[2], k4[3]}}}, side, dv);
      std::array<RSCalibration::Point2d, 4> q;
      for (int j = 0; j < 4; ++j) q[j] = RSCalibration::Point2d{c8[2 * j], c8[2 * j + 1]};
      bool threw = false;
      try {
        std::array<double, 2> e;
        std::array<int32_t, 2> s;
        const std::array<RSCalibration::Transform, 2> tr = corr.EstimatePoseSingleMarkerBoth(q, 0, &e, &s);
        bool same = e[0] == rms[0] && e[1] == rms[1] && s[0] == st[0] && s[1] == st[1];
        for (int k = 0; k < 2; ++k)
          for (int j = 0; j < 3; ++j) same = same && tr[k].rvec[j] == poses[6 * k + j] && tr[k].tvec[j] == poses[6 * k + 3 + j];
        Expect(same, "mirror class bits", id);
      } catch (const std::runtime_error&) { threw = true; }
      Expect(threw == (st[0] == rsba::MARKER_POSE_DEGENERATE), "the mirror class throws on a degenerate solution 0 only", id);
    }
#endif
    // what a status means for the outputs
    for (int k = 0; k < 2; ++k) {
      bool zeros = rms[k] == -1.0;
      for (int j = 0; j < 6; ++j) zeros = zeros && poses[6 * k + j] == 0.0;
      Expect((st[k] <= rsba::MARKER_POSE_ITERATION_CAP) == !zeros, "pose zeros and RMS -1 exactly for statuses 2 and 3", id);
      Expect(st[k] >= 0 && st[k] <= (k == 0 ? 2 : 3), "status range", id);
    }
    if (st[0] == rsba::MARKER_POSE_DEGENERATE) Expect(st[1] == rsba::MARKER_POSE_DEGENERATE, "no solution 0, no solution 1", id);
    if (st[1] <= rsba::MARKER_POSE_ITERATION_CAP) Expect(PoseDistance(poses, poses + 6) >= rsba::kMarkerPoseSameBelow, "two distinct solutions", id);
    // the mirror: an involution, a proper rotation
    double mirror0[6] = {0, 0, 0, 0, 0, 0}, back[6], twice[2] = {-1.0, -1.0}, det = 0.0;
    for (int k = 0; k < 2; ++k) {
      if (st[k] > rsba::MARKER_POSE_ITERATION_CAP) continue;
      double m[6];
      rsba::MirrorMarkerPose(poses + 6 * k, m);
      rsba::MirrorMarkerPose(m, back);
      twice[k] = PoseDistance(back, poses + 6 * k);
      if (k == 0) {
        memcpy(mirror0, m, sizeof(m));
        double R[9], t[3];
        rsba::PoseRotationTranslation(m, R, t);
        det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        // in place
        double inplace[6];
        memcpy(inplace, poses, sizeof(inplace));
        rsba::MirrorMarkerPose(inplace, inplace);
        Expect(memcmp(inplace, m, sizeof(m)) == 0, "MirrorMarkerPose in place", id);
      }
    }
    printf("{");
    PrintDoubles("poses", poses, 12, ", ");
    PrintDoubles("rms", rms, 2, ", ");
    const int32_t st32[2] = {st[0], st[1]};
    PrintInts("status", st32, 2, ", ");
    PrintDoubles("mirror0", mirror0, 6, ", ");
    PrintDoubles("twice", twice, 2, ", ");
    printf("\"det\": %.17g}\n", det);
  }
  fclose(f);
  if (id == 0) { fprintf(stderr, "no cases\n"); return 2; }
  return 0;
}

// One caller summing in observation order that remembers the start a block took from its candidates.
struct ObservingLanes : rsba::SerialLanes {
  bool have = false;
  double cost = -1.0, pose[6] = {0, 0, 0, 0, 0, 0};
  void ChosenStart(bool h, double c, const double* p) {
    have = h;
    cost = h ? c : -1.0;
    for (int q = 0; q < 6; ++q) pose[q] = h ? p[q] : 0.0;
  }
};

struct StartRun {
  std::vector<double> params, rms, start_cost;
  std::vector<int32_t> status, iterations;
};

int Start(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  int all_markers, C, T, M, has_dist, sweeps, has_known;
  long long N;
  double side;
  if (fscanf(f, "%d %d %d %d %lld %d %lf %d %d", &all_markers, &C, &T, &M, &N, &has_dist, &side, &sweeps, &has_known) != 9) { fclose(f); return 2; }
  const size_t nb = (size_t)C + T + M, n = (size_t)N;
  std::vector<double> intr(4 * (size_t)C), dist(5 * (size_t)C), params0(6 * nb), obs(8 * n);
  std::vector<uint8_t> known(nb, 0);
  std::vector<int32_t> cam(n), tim(n), mar(n);
  bool ok = true;
  for (double& v : intr) ok = ok && fscanf(f, "%lf", &v) == 1;
  if (has_dist) for (double& v : dist) ok = ok && fscanf(f, "%lf", &v) == 1;
  for (double& v : params0) ok = ok && fscanf(f, "%lf", &v) == 1;
  if (has_known) for (uint8_t& v : known) { int x = 0; ok = ok && fscanf(f, "%d", &x) == 1; v = (uint8_t)x; }
  for (size_t i = 0; i < n; ++i) {
    ok = ok && fscanf(f, "%d %d %d", &cam[i], &tim[i], &mar[i]) == 3;
    for (int q = 0; q < 8; ++q) ok = ok && fscanf(f, "%lf", &obs[8 * i + (size_t)q]) == 1;
  }
  int K = 0;
  ok = ok && fscanf(f, "%d", &K) == 1 && K >= 0;
  std::vector<int> from_block((size_t)std::max(K, 0));
  std::vector<double> from_value(6 * (size_t)std::max(K, 0));
  for (int k = 0; ok && k < K; ++k) {
    ok = fscanf(f, "%d", &from_block[(size_t)k]) == 1 && from_block[(size_t)k] >= 0 && (size_t)from_block[(size_t)k] < nb;
    for (int q = 0; q < 6; ++q) ok = ok && fscanf(f, "%lf", &from_value[6 * (size_t)k + (size_t)q]) == 1;
  }
  fclose(f);
  if (!ok) { fprintf(stderr, "malformed problem file\n"); return 2; }
  rsba::SceneStartPlan plan;
  const uint8_t* flags = has_known ? known.data() : nullptr;
  if (!rsba::PlanSceneStart(C, T, M, N, cam.data(), tim.data(), mar.data(), flags, all_markers == 0, sweeps, has_dist != 0, &plan)) return 2;
  // both solutions of every detection; solution 0 in arrays of its own, as the unflagged start reads it
  std::vector<double> own_pose(6 * n), own_rms(n), own_pose2(6 * n);
  std::vector<int32_t> own_status(n), own_status2(n);
  for (size_t i = 0; i < n; ++i) {
    double poses[12], e[2];
    int st[2];
    rsba::FitMarkerPoseBoth(&obs[8 * i], &intr[4 * (size_t)cam[i]], has_dist ? &dist[5 * (size_t)cam[i]] : nullptr, side, poses, e, st);
    memcpy(&own_pose[6 * i], poses, 48); memcpy(&own_pose2[6 * i], poses + 6, 48);
    own_rms[i] = e[0]; own_status[i] = st[0]; own_status2[i] = st[1];
  }
  auto which_of = [&](size_t pb, int* block) {
    if (pb < (size_t)C) { *block = (int)pb; return (int)rsba::RESECT_CAMERA; }
    if (pb < (size_t)C + T) { *block = (int)pb - C; return (int)rsba::RESECT_TIME; }
    *block = (int)pb - C - T;
    return (int)rsba::RESECT_MARKER;
  };
  StartRun run[2];
  std::vector<double> refits(6 * from_block.size()), refit_rms(from_block.size());
  std::vector<int32_t> refit_status(from_block.size());
  for (int both = 0; both < 2; ++both) {
    StartRun& r = run[both];
    r.params = params0; r.rms.assign(nb, -1.0); r.start_cost.assign(nb, -1.0); r.status.assign(nb, 0); r.iterations.assign(nb, 0);
    for (size_t b = 0; b < nb; ++b) r.status[b] = plan.given[b] ? rsba::BLOCK_GIVEN : rsba::BLOCK_UNREACHED;
    std::vector<uint8_t> state(plan.given);
    rsba::ResectionArgs a{};
    a.all_markers = all_markers; a.C = C; a.T = T; a.half = 0.5 * side;
    a.camera_index = cam.data(); a.time_index = tim.data(); a.marker_index = mar.data();
    a.observations = obs.data(); a.intrinsics = intr.data(); a.distortion = has_dist ? dist.data() : nullptr;
    a.own_pose = own_pose.data(); a.own_rms = own_rms.data(); a.own_status = own_status.data();
    a.own_pose2 = both ? own_pose2.data() : nullptr; a.own_status2 = both ? own_status2.data() : nullptr;
    a.parameters = r.params.data(); a.known = state.data(); a.status = r.status.data(); a.rms = r.rms.data(); a.iterations = r.iterations.data();
    a.markers_flagged = 1;
    auto lists = [&](int which) {
      a.list_ptr = which == rsba::RESECT_TIME ? plan.time_ptr.data() : which == rsba::RESECT_CAMERA ? plan.camera_ptr.data() : plan.marker_ptr.data();
      a.list_obs = which == rsba::RESECT_TIME ? plan.time_obs.data() : which == rsba::RESECT_CAMERA ? plan.camera_obs.data() : plan.marker_obs.data();
    };
    // (the two runs hold the same blocks until the first block whose chosen starts differ; up to there the candidates' costs are comparable)
    bool comparable = true;
    for (const rsba::RigStartLaunch& l : plan.launches) {
      a.blocks = plan.blocks.data() + l.first;
      a.num_blocks = l.count;
      const int which = l.which == rsba::kRigStartTime ? rsba::RESECT_TIME : l.which == rsba::kRigStartCamera ? rsba::RESECT_CAMERA : rsba::RESECT_MARKER;
      lists(which);
      for (int k = 0; k < l.count; ++k) {
        const int block = a.blocks[k];
        const size_t pb = which == rsba::RESECT_MARKER ? (size_t)C + T + block : which == rsba::RESECT_TIME ? (size_t)C + block : (size_t)block;
        const bool first_fit = state[pb] == 0;
        ObservingLanes lanes;
        if (both) rsba::ResectBlock<true>(a, which, block, lanes);
        else rsba::ResectBlock<false>(a, which, block, lanes);
        if (!first_fit) continue;
        r.start_cost[pb] = lanes.cost;
        if (both && comparable) {
          const double without = run[0].start_cost[pb];
          if (without >= 0.0) Expect(lanes.have && lanes.cost <= without, "the chosen start's cost with both solutions is not higher", (int)pb);
          comparable = lanes.cost == without;
        }
      }
    }
    if (!both) continue;
    // the minimisers reached from the given values, with the flagged run's other blocks
    for (size_t k = 0; k < from_block.size(); ++k) {
      const size_t pb = (size_t)from_block[k];
      std::vector<double> params(r.params);
      std::vector<double> rms2(r.rms);
      std::vector<int32_t> status2(r.status), iterations2(r.iterations);
      std::vector<uint8_t> state2(state);
      memcpy(&params[6 * pb], &from_value[6 * k], 48);
      state2[pb] = 1;
      a.parameters = params.data(); a.known = state2.data(); a.status = status2.data(); a.rms = rms2.data(); a.iterations = iterations2.data();
      int block = 0;
      const int which = which_of(pb, &block);
      lists(which);
      a.blocks = &block; a.num_blocks = 1;
      ObservingLanes lanes;
      rsba::ResectBlock<true>(a, which, block, lanes);
      memcpy(&refits[6 * k], &params[6 * pb], 48);
      refit_rms[k] = rms2[pb]; refit_status[k] = status2[pb];
    }
  }
  printf("{");
  for (int both = 0; both < 2; ++both) {
    const StartRun& r = run[both];
    printf("\"%s\": {", both ? "both" : "single");
    PrintDoubles("blocks", r.params.data(), 6 * nb, ", ");
    PrintDoubles("rms", r.rms.data(), nb, ", ");
    PrintInts("status", r.status.data(), nb, ", ");
    PrintInts("iterations", r.iterations.data(), nb, ", ");
    PrintDoubles("start_cost", r.start_cost.data(), nb, "}, ");
  }
  PrintDoubles("own_pose", own_pose.data(), 6 * n, ", ");
  PrintDoubles("own_pose2", own_pose2.data(), 6 * n, ", ");
  PrintInts("own_status2", own_status2.data(), n, ", ");
  PrintDoubles("refits", refits.data(), refits.size(), ", ");
  PrintDoubles("refit_rms", refit_rms.data(), refit_rms.size(), ", ");
  PrintInts("refit_status", refit_status.data(), refit_status.size(), "}\n");
  return 0;
}

void Builtin() {
#ifndef RSBA_DRIVER_HEADERS_ONLY
  const double k4[4] = {620.0, 620.0, 320.0, 240.0}, c8[8] = {300, 200, 340, 202, 338, 243, 299, 240}, side = 0.05;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double poses[12], rms[2];
  int32_t st[2];
  for (double& v : poses) v = 7.0;
  Expect(rsba_marker_pose_from_corners_both(nullptr, k4, nullptr, side, poses, rms, st) == RSBA_ERR_ARG, "null corners", 0);
  Expect(rsba_marker_pose_from_corners_both(c8, nullptr, nullptr, side, poses, rms, st) == RSBA_ERR_ARG, "null intrinsics", 0);
  Expect(rsba_marker_pose_from_corners_both(c8, k4, nullptr, side, nullptr, rms, st) == RSBA_ERR_ARG, "null poses", 0);
  for (double s : {0.0, -1.0, nan, inf}) Expect(rsba_marker_pose_from_corners_both(c8, k4, nullptr, s, poses, rms, st) == RSBA_ERR_ARG, "side", 0);
  for (double v : {nan, inf, -inf}) {
    double c[8], k[4], d[5] = {0, 0, 0, 0, 0};
    memcpy(c, c8, sizeof(c)); memcpy(k, k4, sizeof(k));
    c[5] = v;
    Expect(rsba_marker_pose_from_corners_both(c, k, d, side, poses, rms, st) == RSBA_ERR_ARG, "non-finite corner", 0);
    c[5] = c8[5]; k[3] = v;
    Expect(rsba_marker_pose_from_corners_both(c, k, d, side, poses, rms, st) == RSBA_ERR_ARG, "non-finite intrinsics", 0);
    k[3] = k4[3]; d[4] = v;
    Expect(rsba_marker_pose_from_corners_both(c, k, d, side, poses, rms, st) == RSBA_ERR_ARG, "non-finite coefficient", 0);
  }
  const double zero_f[4] = {0.0, 620.0, 320.0, 240.0};
  Expect(rsba_marker_pose_from_corners_both(c8, zero_f, nullptr, side, poses, rms, st) == RSBA_ERR_ARG, "zero focal length", 0);
  for (double v : poses) Expect(v == 7.0, "a refused call writes nothing", 0);
  Expect(rsba_marker_pose_from_corners_both(c8, k4, nullptr, side, poses, rms, st) == RSBA_OK && st[0] == 0, "the same arguments in range", 0);
#else
  const double k4[4] = {620.0, 620.0, 320.0, 240.0}, c8[8] = {300, 200, 340, 202, 338, 243, 299, 240}, side = 0.05;
  double poses[12], rms[2];
  int st[2];
  rsba::FitMarkerPoseBoth(c8, k4, nullptr, side, poses, rms, st);
#endif
  // a first solution that is no solution gives no second one, whatever the pose array holds
  double p1[6] = {7, 7, 7, 7, 7, 7}, e1 = 7.0;
  Expect(rsba::SecondMarkerPose(c8, k4, nullptr, side, poses, rsba::MARKER_POSE_DEGENERATE, p1, &e1) == rsba::MARKER_POSE_DEGENERATE && e1 == -1.0 && p1[0] == 0.0,
         "status 2 in, status 2 out", 0);
  // a first solution at the camera's centre has no line of sight: the mirrored start is not finite
  const double at_origin[6] = {0.1, 0.2, 0.3, 0.0, 0.0, 0.0};
  Expect(rsba::SecondMarkerPose(c8, k4, nullptr, side, at_origin, rsba::MARKER_POSE_CONVERGED, p1, &e1) == rsba::MARKER_POSE_DEGENERATE && e1 == -1.0,
         "unusable mirrored start", 0);
  // a first solution whose mirror image puts a corner behind the camera
  const double grazing[6] = {0.0, 1.5, 0.0, 0.0, 0.0, 0.02};
  Expect(rsba::SecondMarkerPose(c8, k4, nullptr, side, grazing, rsba::MARKER_POSE_CONVERGED, p1, &e1) == rsba::MARKER_POSE_DEGENERATE && e1 == -1.0 && p1[5] == 0.0,
         "a corner behind the camera at the mirrored start", 0);
}

}  // namespace

int main(int argc, char** argv) {
  int rc = 0;
  if (argc == 3 && std::string(argv[1]) == "fit") rc = Fit(argv[2]);
  else if (argc == 3 && std::string(argv[1]) == "start") rc = Start(argv[2]);
  else if (argc == 1) Builtin();
  else { fprintf(stderr, "usage: marker_pose_both_driver [fit FILE | start FILE]\n"); return 2; }
  if (rc) return rc;
  if (g_fail) { fprintf(stderr, "marker pose both driver: %d failures\n", g_fail); return 1; }
  fprintf(stderr, "marker pose both driver: ok\n");
  return 0;
}
