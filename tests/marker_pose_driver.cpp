// Stand-alone check of the single-marker pose fit of the host build (csrc/ba_marker_pose.hpp FitMarkerPose, ba_initial_guess.cpp
// MarkerPoseFromCorners / InitialTimePoses, include/rsba/correspondencer.h EstimatePoseSingleMarkers), built with
// -fsanitize=address,undefined by tests/test_marker_pose_host.py and run on the cases that test writes:
//   argv[1]: one detection per line — fx fy ppx ppy, has_dist, k1 k2 p1 p2 k3, side, the eight corner values, the reference's pose6 and rms
//   1. FitMarkerPose on every line: converged, the reference's pose (as rotation matrix and translation) and RMS to 1e-6; the C entry
//      and the C++ mirror return the header routine's bits;
//   2. degenerate inputs (four equal corners, three collinear corners in both arrangements, a corner at a radius where the undistortion
//      has no fixed point): status 2, pose zeros, RMS -1, RSBA_ERR_UNSUPPORTED from the C entry, an exception from the mirror;
//   3. the argument checks of rsba_marker_pose_from_corners and rsba_problem_initial_time_poses, and the latter on a one-camera problem
//      made of the lines: every time block is the header routine's pose, a collapsed detection is counted and keeps its block's bits.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ba_marker_pose.hpp"
#include "ba_problem.hpp"
#include "rsba.h"
#include "rsba/correspondencer.h"

namespace rsba { int DeviceCount() { return 0; } }   // (the kernels are not in this build)

namespace {

int g_fail = 0;
void Expect(bool ok, const char* what, int line) {
  if (!ok) { ++g_fail; if (g_fail < 20) printf("FAIL %s (case %d)\n", what, line); }
}

struct Case { double k4[4]; int has_dist; double k5[5], side, c8[8], pose[6], rms; };

double PoseDistance(const double* a, const double* b) {
  double Ra[9], Rb[9], d = 0.0;
  rsba::Rodrigues(a, Ra); rsba::Rodrigues(b, Rb);
  for (int i = 0; i < 9; ++i) d = std::fmax(d, std::fabs(Ra[i] - Rb[i]));
  for (int i = 3; i < 6; ++i) d = std::fmax(d, std::fabs(a[i] - b[i]));
  return d;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: marker_pose_driver cases.txt\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
  std::vector<Case> cases;
  for (;;) {
    Case c;
    int got = fscanf(f, "%lf %lf %lf %lf %d", &c.k4[0], &c.k4[1], &c.k4[2], &c.k4[3], &c.has_dist);
    if (got != 5) break;
    for (double& v : c.k5) got += fscanf(f, "%lf", &v);
    got += fscanf(f, "%lf", &c.side);
    for (double& v : c.c8) got += fscanf(f, "%lf", &v);
    for (double& v : c.pose) got += fscanf(f, "%lf", &v);
    got += fscanf(f, "%lf", &c.rms);
    if (got != 26) { printf("malformed case file\n"); fclose(f); return 2; }
    cases.push_back(c);
  }
  fclose(f);
  if (cases.empty()) { printf("no cases\n"); return 2; }

  // 1. the synthetic set
  double worst = 0.0, worst_rms = 0.0;
  for (size_t i = 0; i < cases.size(); ++i) {
    const Case& c = cases[i];
    const double* k5 = c.has_dist ? c.k5 : nullptr;
    double pose[6], rms = 0.0;
    const int st = rsba::FitMarkerPose(c.c8, c.k4, k5, c.side, pose, &rms);
    Expect(st == rsba::MARKER_POSE_CONVERGED, "status", (int)i);
    worst = std::fmax(worst, PoseDistance(pose, c.pose));
    worst_rms = std::fmax(worst_rms, std::fabs(rms - c.rms));
    double pose2[6], rms2 = 0.0;
    int32_t st2 = -1;
    Expect(rsba_marker_pose_from_corners(c.c8, c.k4, k5, c.side, pose2, &rms2, &st2) == RSBA_OK, "C entry", (int)i);
    Expect(memcmp(pose, pose2, sizeof(pose)) == 0 && rms == rms2 && st2 == st, "C entry bits", (int)i);
    std::vector<std::array<double, 5>> dist;
    if (k5) dist.push_back({{c.k5[0], c.k5[1], c.k5[2], c.k5[3], c.k5[4]}});
    RSCalibration::Correspondencer corr({{{c.k4[0], c.k4[1], c.k4[2], c.k4[3]}}}, c.side, dist);
    std::array<RSCalibration::Point2d, 4> q;
    for (int j = 0; j < 4; ++j) q[j] = RSCalibration::Point2d{c.c8[2 * j], c.c8[2 * j + 1]};
    std::vector<double> e;
    const std::vector<RSCalibration::Transform> tr = corr.EstimatePoseSingleMarkers({q, q}, 0, &e);
    Expect(tr.size() == 2 && e.size() == 2 && e[1] == rms, "mirror size", (int)i);
    for (int j = 0; j < 3; ++j) Expect(tr[1].rvec[j] == pose[j] && tr[1].tvec[j] == pose[3 + j], "mirror bits", (int)i);
  }
  printf("largest pose difference %.3g, largest rms difference %.3g px over %zu cases\n", worst, worst_rms, cases.size());
  Expect(worst < 1e-6 && worst_rms < 1e-6, "accuracy", -1);

  // 2. degenerate inputs
  const Case& c0 = cases[0];
  const double strong[5] = {-0.28, 0.09, 1e-3, -5e-4, -0.01};
  double far8[8];
  memcpy(far8, c0.c8, sizeof(far8));
  far8[0] = far8[1] = 5000.0;
  const double equal8[8] = {100, 100, 100, 100, 100, 100, 100, 100};
  const double line_a[8] = {100, 100, 200, 100, 300, 100, 200, 200}, line_b[8] = {100, 100, 200, 100, 200, 200, 300, 300};
  const double line_c[8] = {150, 250, 100, 100, 200, 100, 300, 100};
  struct { const double* c8; const double* k5; } bad[] = {{equal8, nullptr}, {line_a, nullptr}, {line_b, nullptr}, {line_c, nullptr}, {far8, strong}, {equal8, strong}};
  for (int i = 0; i < 6; ++i) {
    double pose[6] = {7, 7, 7, 7, 7, 7}, rms = 7.0;
    Expect(rsba::FitMarkerPose(bad[i].c8, c0.k4, bad[i].k5, c0.side, pose, &rms) == rsba::MARKER_POSE_DEGENERATE, "degenerate status", i);
    bool zeros = rms == -1.0;
    for (double v : pose) zeros = zeros && v == 0.0;
    Expect(zeros, "degenerate outputs", i);
    int32_t st = -1;
    Expect(rsba_marker_pose_from_corners(bad[i].c8, c0.k4, bad[i].k5, c0.side, pose, &rms, &st) == RSBA_ERR_UNSUPPORTED && st == 2 && rms == -1.0,
           "degenerate C entry", i);
    bool threw = false;
    try {
      std::vector<std::array<double, 5>> dist;
      if (bad[i].k5) dist.push_back({{strong[0], strong[1], strong[2], strong[3], strong[4]}});
      RSCalibration::Correspondencer corr({{{c0.k4[0], c0.k4[1], c0.k4[2], c0.k4[3]}}}, c0.side, dist);
      std::array<RSCalibration::Point2d, 4> q;
      for (int j = 0; j < 4; ++j) q[j] = RSCalibration::Point2d{bad[i].c8[2 * j], bad[i].c8[2 * j + 1]};
      corr.EstimatePoseSingleMarkers({q}, 0);
    } catch (const std::runtime_error&) { threw = true; }
    Expect(threw, "degenerate mirror", i);
  }

  // 3. argument checks
  {
    double pose[6] = {7, 7, 7, 7, 7, 7};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    Expect(rsba_marker_pose_from_corners(nullptr, c0.k4, nullptr, c0.side, pose, nullptr, nullptr) == RSBA_ERR_ARG, "null corners", 0);
    Expect(rsba_marker_pose_from_corners(c0.c8, nullptr, nullptr, c0.side, pose, nullptr, nullptr) == RSBA_ERR_ARG, "null intrinsics", 0);
    Expect(rsba_marker_pose_from_corners(c0.c8, c0.k4, nullptr, c0.side, nullptr, nullptr, nullptr) == RSBA_ERR_ARG, "null pose", 0);
    for (double side : {0.0, -1.0, nan, inf})
      Expect(rsba_marker_pose_from_corners(c0.c8, c0.k4, nullptr, side, pose, nullptr, nullptr) == RSBA_ERR_ARG, "side", 0);
    for (double v : {nan, inf, -inf}) {
      double c8[8], k4[4], k5[5] = {0, 0, 0, 0, 0};
      memcpy(c8, c0.c8, sizeof(c8)); memcpy(k4, c0.k4, sizeof(k4));
      c8[5] = v;
      Expect(rsba_marker_pose_from_corners(c8, k4, k5, c0.side, pose, nullptr, nullptr) == RSBA_ERR_ARG, "non-finite corner", 0);
      c8[5] = c0.c8[5]; k4[3] = v;
      Expect(rsba_marker_pose_from_corners(c8, k4, k5, c0.side, pose, nullptr, nullptr) == RSBA_ERR_ARG, "non-finite intrinsics", 0);
      k4[3] = c0.k4[3]; k5[4] = v;
      Expect(rsba_marker_pose_from_corners(c8, k4, k5, c0.side, pose, nullptr, nullptr) == RSBA_ERR_ARG, "non-finite coefficient", 0);
    }
    for (double v : pose) Expect(v == 7.0, "a refused call writes nothing", 0);
    Expect(rsba_problem_initial_time_poses(nullptr, nullptr) == RSBA_ERR_ARG, "null problem", 0);
  }
  {
    // the lines that share the first line's camera as one-camera, one-marker problem: time t = detection t
    std::vector<double> obs, want;
    for (const Case& c : cases) {
      if (memcmp(c.k4, c0.k4, sizeof(c.k4)) != 0 || c.has_dist != c0.has_dist || memcmp(c.k5, c0.k5, sizeof(c.k5)) != 0) continue;
      obs.insert(obs.end(), c.c8, c.c8 + 8);
      double pose[6], rms;
      rsba::FitMarkerPose(c.c8, c.k4, c.has_dist ? c.k5 : nullptr, c.side, pose, &rms);
      want.insert(want.end(), pose, pose + 6);
    }
    const int T = (int)(obs.size() / 8);
    for (int k = 0; k < 8; ++k) obs[8 + k] = obs[8 + (k & 1)];   // detection 1 collapses to a point
    std::vector<int32_t> ti(T), zero(T, 0);
    for (int t = 0; t < T; ++t) ti[t] = t;
    std::vector<double> params(6 * (size_t)(1 + T + 1), 0.5);
    rsba_problem* p = nullptr;
    Expect(rsba_problem_create_marker_chain(RSBA_MODEL_MARKER_CHAIN, 1, T, 1, T, ti.data(), zero.data(), zero.data(), obs.data(), params.data(), c0.k4,
                                            c0.side, &p) == RSBA_OK, "create", 0);
    if (p) {
      if (c0.has_dist) Expect(rsba_problem_set_distortion(p, c0.k5) == RSBA_OK, "set distortion", 0);
      int32_t missing = -1;
      Expect(rsba_problem_initial_time_poses(p, &missing) == RSBA_OK && missing == 1, "initial time poses", missing);
      const double* got = rsba_problem_parameters(p);
      for (int t = 0; t < T; ++t)
        for (int k = 0; k < 6; ++k) Expect(got[6 * (1 + t) + k] == (t == 1 ? 0.5 : want[6 * t + k]), "time block", t);
      for (int k = 0; k < 6; ++k) Expect(got[k] == 0.5 && got[6 * (1 + T) + k] == 0.5, "camera and marker blocks untouched", k);
      rsba_problem_free(p);
    }
    printf("%d time blocks checked\n", T);
  }
  if (g_fail) { printf("marker pose driver: %d failures\n", g_fail); return 1; }
  printf("marker pose driver: ok\n");
  return 0;
}
