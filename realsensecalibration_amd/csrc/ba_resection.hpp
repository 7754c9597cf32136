// Block resection: ONE pose block of a marker-chain problem (a time, a camera or a marker) fitted to all the detections that name it, the
// other two blocks of each detection held at their current values — ceres::Solve with every other block constant, one block at a time, and
// the step of the whole-rig start (rsba_problem_start_rig; the rounds are planned in ba_rig_start_plan.hpp) and of the scene start, which
// fits the marker blocks too (rsba_problem_start_scene; ba_scene_start_plan.hpp).
//
//   objective   the marker-chain reprojection cost of the block's usable detections, eight residuals each, through the functor the model
//               selects: corner --marker--> --time--> --camera--> projection, a base block (camera 0; marker 0 of RSBA_MODEL_MARKER_CHAIN)
//               acting as the identity, ProjectCorner<true> with the detecting camera's coefficients (zeros: the pinhole camera)
//   usable      a detection whose OTHER variable block (a time's detecting camera, a camera's time) is flagged in known[]; marker blocks are
//               inputs and always known.  The scene start flags the marker blocks too, known[C + T + M]:
//               a detection is usable for a block when BOTH its other blocks are flagged, and a marker block is fitted like the others
//   rows        a pose block's rule of ba_math.hpp, as MarkerPoseLinearise applies it to a single marker: with Q the sensitivity of the
//               residual to the point leaving the fitted transform, d r / d t = Q, d r / d w = [w* x Q_i] Jl
//   step        MarkerPoseMinimise (ba_marker_pose.hpp): FitMarkerPose's loop, step, accept / reject / lambda and convergence rule, with its
//               sufficient-decrease test switched on (a block's residuals at its minimum are pixels, not noise: see there)
//   start       a block that is already known starts from its value (a refining sweep).  Another block starts from the best of up to four
//               candidates: the usable detections with the lowest own-fit RMS (k_marker_pose's; ties to the lower observation index), each
//               own-fit pose composed with the detection's two known blocks, the block cost evaluated at each, the lowest taken.  A second
//               detection therefore resolves the planar two-fold ambiguity of the first: the wrong basin of a small frontal marker fits
//               that marker almost as well as the right one, and the rest of the board not at all.
//   both        kBoth (RSBA_START_BOTH_SOLUTIONS): the same up-to-four detections, chosen in the same order, each contributing its own fit
//               and then, where it has one (own_status2 0 or 1), its second solution (k_marker_pose_mirror's: ba_marker_pose.hpp) — up to
//               eight candidates, the strict < keeping the earlier one on a tie.  The list without the flag is a sublist of the list with
//               it, in the same order, and the cost of each candidate is the same function of the same pose, so THE CHOSEN START'S BLOCK
//               COST WITH THE FLAG IS NEVER HIGHER THAN WITHOUT IT (tests/marker_pose_both_driver.cpp holds the host to that).  A block
//               whose detections all fell into the wrong basin, or that has a single detection, so has the right one among its starts.
//               Refits, the minimiser, statuses and RMS are the same code with and without.
//
// ResectBlock is plain host / device code over a `Lanes` policy: which of a block's detections this caller accumulates (first(), stride())
// and how partial sums meet (Sum, Min, ArgMin).  SerialLanes is one caller summing in observation order (the host: tests/
// rig_start_plan_driver.cpp); DeviceLanes<false> is a wavefront, DeviceLanes<true> a 256-lane workgroup.  ChosenStart(have, cost, pose) is
// told the start a block that is not yet known takes from its candidates and that start's block cost: nothing on the device, what a host
// test records (tests/marker_pose_both_driver.cpp).  Every lane of the device forms
// the same reduced system — an xor butterfly adds the same pairs in every lane, and the four wavefronts' sums meet in LDS in wavefront
// order — and solves the 6 x 6 redundantly, so control flow is uniform, nothing is broadcast, and a block's bits depend on its own list
// alone: not on its place in the launch, not on the call.  No atomics, no spin waits: the flags a launch sets are read by the next launch
// of the stream.
#pragma once
#include <climits>
#include <cstdint>

#include "ba_marker_pose.hpp"

namespace rsba {

enum {
  RESECT_TIME = 0,
  RESECT_CAMERA = 1,
  RESECT_MARKER = 2,         // the scene start only
  BLOCK_CONVERGED = 0,       // MARKER_POSE_CONVERGED
  BLOCK_ITERATION_CAP = 1,   // MARKER_POSE_ITERATION_CAP
  BLOCK_DEGENERATE = 2,      // usable detections, but no candidate with a finite cost and every point in front: the block keeps its bits
  BLOCK_UNREACHED = 3,       // no usable detection: the block keeps its bits
  BLOCK_GIVEN = 4,           // flagged by the caller, or a base block
  kResectionSums = 28        // cost, J'J (21), J'r (6)
};

// What a resection launch reads and writes (device pointers on the device).  Parameters are [C | T | M] x 6 as in the problem.
struct ResectionArgs {
  int all_markers;                 // 1: marker 0 is a block like the others (the Test2 wiring); 0: it is the base marker, the identity
  int C, T;
  double half;                     // half the marker's side
  const int* list_ptr;             // CSR by the fitted kind of block: [T + 1] or [C + 1]
  const int* list_obs;             // [N] observation indices, ascending inside a block
  const int32_t* camera_index;     // [N]
  const int32_t* time_index;       // [N]
  const int32_t* marker_index;     // [N]
  const double* observations;      // [N][8]
  const double* intrinsics;        // [C][4]
  const double* distortion;        // [C][5] or null
  const double* own_pose;          // [N][6] k_marker_pose's fit of each detection alone
  const double* own_rms;           // [N]
  const int32_t* own_status;       // [N]
  double* parameters;
  uint8_t* known;                  // [C + T]; the scene start: [C + T + M] and one more that is never set; so the three arrays below
  int32_t* status;                 // [C + T]
  double* rms;                     // [C + T]
  int32_t* iterations;             // [C + T]
  const int* blocks;               // the launch's blocks: time, camera or marker indices
  int num_blocks;
  int markers_flagged;             // the host: 0: marker blocks are inputs, always known (the whole-rig start); 1: known[C + T + m] says so
  const double* own_pose2;         // [N][6] kBoth only: each detection's second solution (k_marker_pose_mirror's), zeros where there is none
  const int32_t* own_status2;      // [N]    kBoth only: 0 or 1 where there is one
};

// Rotation matrix (row-major) and translation of a pose block as the functors apply it (CameraConstants: the first-order form at
// theta^2 <= DBL_EPSILON); a null pose is a base block, the identity.
RSBA_HD void PoseRotationTranslation(const double* pose6, double R[9], double t[3]) {
  if (!pose6) {
    RSBA_UNROLL
    for (int q = 0; q < 9; ++q) R[q] = (q == 0 || q == 4 || q == 8) ? 1.0 : 0.0;
    t[0] = t[1] = t[2] = 0.0;
    return;
  }
  const double none[4] = {0.0, 0.0, 0.0, 0.0};
  double cc[CC_STRIDE];
  CameraConstants(pose6, none, cc);
  RSBA_UNROLL
  for (int q = 0; q < 9; ++q) R[q] = cc[CC_R + q];
  RSBA_UNROLL
  for (int q = 0; q < 3; ++q) t[q] = cc[CC_T + q];
}

RSBA_HD void Mat3Mul(const double* A, const double* B, double* out) {   // A B
  RSBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    RSBA_UNROLL
    for (int j = 0; j < 3; ++j) out[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
  }
}
RSBA_HD void Mat3MulTransposed(const double* A, const double* B, double* out) {   // A B'
  RSBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    RSBA_UNROLL
    for (int j = 0; j < 3; ++j) out[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
  }
}
RSBA_HD void Mat3Vec(const double* A, const double* x, double* y) {
  RSBA_UNROLL
  for (int i = 0; i < 3; ++i) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
}
RSBA_HD void Mat3TransposedVec(const double* A, const double* x, double* y) {
  RSBA_UNROLL
  for (int i = 0; i < 3; ++i) y[i] = A[i] * x[0] + A[3 + i] * x[1] + A[6 + i] * x[2];
}

// The three pose blocks of observation o as the model wires them: null for a block the functor does not apply.
RSBA_HD void ObservationBlocks(const ResectionArgs& a, int o, const double** cam, const double** tim, const double** mar) {
  const int c = a.camera_index[o], m = a.marker_index[o];
  *cam = c != 0 ? a.parameters + 6 * (size_t)c : nullptr;
  *tim = a.parameters + 6 * (size_t)(a.C + a.time_index[o]);
  *mar = (a.all_markers != 0 || m != 0) ? a.parameters + 6 * (size_t)(a.C + a.T + m) : nullptr;
}

// What one detection contributes that does not move with the fitted pose: the four points ENTERING the fitted transform and the known
// transform behind it.  A time: the corners through the marker block, then the camera block behind (absent for the base camera).  A camera:
// the corners through marker and time, nothing behind.  A marker: the raw corners, camera o time behind (the time alone for the base camera).
struct ResectionFrame {
  double x[12];
  double Ro[9], to[3];
  bool outer;
};

// (kMarkerToo = false: the caller never asks for a marker, and the instance carries no code of that kind)
template <bool kMarkerToo = true>
RSBA_HD void ResectionFrameOf(int which, const double* cam6, const double* time6, const double* marker6, double half, ResectionFrame* f) {
  if (kMarkerToo && which == RESECT_MARKER) {
    RSBA_UNROLL
    for (int j = 0; j < 4; ++j) {
      f->x[3 * j] = (j == 1 || j == 2) ? half : -half; f->x[3 * j + 1] = j < 2 ? half : -half; f->x[3 * j + 2] = 0.0;
    }
    f->outer = true;
    if (cam6) {   // Ro = Rc Rt, to = Rc tt + tc
      double Rc[9], tc[3], Rt[9], tt[3], s[3];
      PoseRotationTranslation(cam6, Rc, tc);
      PoseRotationTranslation(time6, Rt, tt);
      Mat3Mul(Rc, Rt, f->Ro);
      Mat3Vec(Rc, tt, s);
      f->to[0] = s[0] + tc[0]; f->to[1] = s[1] + tc[1]; f->to[2] = s[2] + tc[2];
    } else {
      PoseRotationTranslation(time6, f->Ro, f->to);
    }
    return;
  }
  double Rm[9], tm[3];
  PoseRotationTranslation(marker6, Rm, tm);
  double Rt[9], tt[3];
  if (which == RESECT_CAMERA) PoseRotationTranslation(time6, Rt, tt);
  RSBA_UNROLL
  for (int j = 0; j < 4; ++j) {
    const double X = (j == 1 || j == 2) ? half : -half, Y = j < 2 ? half : -half;
    double pm[3];
    pm[0] = Rm[0] * X + Rm[1] * Y + tm[0];
    pm[1] = Rm[3] * X + Rm[4] * Y + tm[1];
    pm[2] = Rm[6] * X + Rm[7] * Y + tm[2];
    if (which == RESECT_CAMERA) {
      double q[3];
      Mat3Vec(Rt, pm, q);
      f->x[3 * j] = q[0] + tt[0]; f->x[3 * j + 1] = q[1] + tt[1]; f->x[3 * j + 2] = q[2] + tt[2];
    } else {
      f->x[3 * j] = pm[0]; f->x[3 * j + 1] = pm[1]; f->x[3 * j + 2] = pm[2];
    }
  }
  f->outer = which == RESECT_TIME && cam6 != nullptr;
  PoseRotationTranslation(f->outer ? cam6 : nullptr, f->Ro, f->to);
}

// One detection's share of the cost, J'J (packed, 21), J'r and the smallest depth at the fitted pose whose constants are cc
// (CameraConstants); the sums are added to.
RSBA_HD void ResectionAccumulate(const double* cc, const ResectionFrame& f, const double* intr4, const double k5[5], const double* c8,
                                 double* cost_io, double A[21], double g[6], double* min_depth) {
  const double* R = cc + CC_R;
  const double* K = cc + CC_K;
  const bool small = cc[CC_SMALL] != 0.0;
  const double fx = intr4[0], fy = intr4[1], ppx = intr4[2], ppy = intr4[3];
  double cost = *cost_io, minz = *min_depth;
  RSBA_UNROLL
  for (int j = 0; j < 4; ++j) {
    const double x0 = f.x[3 * j], x1 = f.x[3 * j + 1], x2 = f.x[3 * j + 2];
    const double q0 = R[0] * x0 + R[1] * x1 + R[2] * x2, q1 = R[3] * x0 + R[4] * x1 + R[5] * x2, q2 = R[6] * x0 + R[7] * x1 + R[8] * x2;
    double P[3] = {q0 + cc[CC_T], q1 + cc[CC_T + 1], q2 + cc[CC_T + 2]};
    if (f.outer) {
      double Po[3];
      Mat3Vec(f.Ro, P, Po);
      P[0] = Po[0] + f.to[0]; P[1] = Po[1] + f.to[1]; P[2] = Po[2] + f.to[2];
    }
    double r[2], Qc[6], Q[6];
    ProjectCorner<true>(P[0], P[1], P[2], fx, fy, ppx, ppy, k5, c8[2 * j], c8[2 * j + 1], r, Qc);
    minz = fmin(minz, P[2]);
    if (f.outer) {
      CarryQ(Qc, f.Ro, Q);
    } else {
      RSBA_UNROLL
      for (int q = 0; q < 6; ++q) Q[q] = Qc[q];
    }
    const double w0 = small ? x0 : q0, w1 = small ? x1 : q1, w2 = small ? x2 : q2;
    RSBA_UNROLL
    for (int i = 0; i < 2; ++i) {
      const double Q0 = Q[3 * i], Q1 = Q[3 * i + 1], Q2 = Q[3 * i + 2];
      const double a0 = w1 * Q2 - w2 * Q1, a1 = w2 * Q0 - w0 * Q2, a2 = w0 * Q1 - w1 * Q0;   // w* x Q_i
      double J[6];
      J[0] = a0 * K[0] + a1 * K[3] + a2 * K[6];
      J[1] = a0 * K[1] + a1 * K[4] + a2 * K[7];
      J[2] = a0 * K[2] + a1 * K[5] + a2 * K[8];
      J[3] = Q0; J[4] = Q1; J[5] = Q2;
      cost += r[i] * r[i];
      RSBA_UNROLL
      for (int a = 0; a < 6; ++a) {
        g[a] += J[a] * r[i];
        RSBA_UNROLL
        for (int b = a; b < 6; ++b) A[Sym6(a, b)] += J[a] * J[b];
      }
    }
  }
  *cost_io = cost;
  *min_depth = minz;
}

// The candidate a detection gives for the fitted block: its own-fit pose D (marker frame -> detecting camera's frame) composed with its two
// known blocks, D = camera o time o marker solved for the time, for the camera or for the marker.
template <bool kMarkerToo = true>
RSBA_HD void ResectionCandidate(int which, const double* own6, const double* cam6, const double* time6, const double* marker6, double pose[6]) {
  double Rd[9], td[3], Rm[9], tm[3];
  PoseRotationTranslation(own6, Rd, td);
  double R[9], t[3];
  if (kMarkerToo && which == RESECT_MARKER) {
    double Rc[9], tc[3], Rt[9], tt[3], Rct[9], s[3], d[3];
    PoseRotationTranslation(cam6, Rc, tc);
    PoseRotationTranslation(time6, Rt, tt);
    // R_m = (R_c R_t)' R_d,  t_m = (R_c R_t)' (t_d - R_c t_t - t_c)
    Mat3Mul(Rc, Rt, Rct);
    RSBA_UNROLL
    for (int i = 0; i < 3; ++i) {
      RSBA_UNROLL
      for (int j = 0; j < 3; ++j) R[3 * i + j] = Rct[i] * Rd[j] + Rct[3 + i] * Rd[3 + j] + Rct[6 + i] * Rd[6 + j];
    }
    Mat3Vec(Rc, tt, s);
    d[0] = td[0] - s[0] - tc[0]; d[1] = td[1] - s[1] - tc[1]; d[2] = td[2] - s[2] - tc[2];
    Mat3TransposedVec(Rct, d, t);
    RotationMatrixToRvec(R, pose);
    pose[3] = t[0]; pose[4] = t[1]; pose[5] = t[2];
    return;
  }
  PoseRotationTranslation(marker6, Rm, tm);
  if (which == RESECT_TIME) {
    double Rc[9], tc[3], RcD[9], d[3], e[3], s[3];
    PoseRotationTranslation(cam6, Rc, tc);
    // R_t = R_c' R_d R_m',  t_t = R_c' (t_d - t_c) - R_t t_m
    RSBA_UNROLL
    for (int i = 0; i < 3; ++i) {
      RSBA_UNROLL
      for (int j = 0; j < 3; ++j) RcD[3 * i + j] = Rc[i] * Rd[j] + Rc[3 + i] * Rd[3 + j] + Rc[6 + i] * Rd[6 + j];
    }
    Mat3MulTransposed(RcD, Rm, R);
    d[0] = td[0] - tc[0]; d[1] = td[1] - tc[1]; d[2] = td[2] - tc[2];
    Mat3TransposedVec(Rc, d, e);
    Mat3Vec(R, tm, s);
    t[0] = e[0] - s[0]; t[1] = e[1] - s[1]; t[2] = e[2] - s[2];
  } else {
    double Rt[9], tt[3], Rtm[9], ttm[3], s[3];
    PoseRotationTranslation(time6, Rt, tt);
    // (time o marker) = (R_t R_m, R_t t_m + t_t);  R_c = R_d (R_t R_m)',  t_c = t_d - R_c (R_t t_m + t_t)
    Mat3Mul(Rt, Rm, Rtm);
    Mat3Vec(Rt, tm, ttm);
    ttm[0] += tt[0]; ttm[1] += tt[1]; ttm[2] += tt[2];
    Mat3MulTransposed(Rd, Rtm, R);
    Mat3Vec(R, ttm, s);
    t[0] = td[0] - s[0]; t[1] = td[1] - s[1]; t[2] = td[2] - s[2];
  }
  RotationMatrixToRvec(R, pose);
  pose[3] = t[0]; pose[4] = t[1]; pose[5] = t[2];
}

// One caller, every detection, sums in observation order: the host.
struct SerialLanes {
  RSBA_HD int first() const { return 0; }
  RSBA_HD int stride() const { return 1; }
  template <int N> RSBA_HD void Sum(double (&)[N]) const {}
  RSBA_HD void Min(double*) const {}
  RSBA_HD void ArgMin(double*, int*) const {}
  RSBA_HD void ChosenStart(bool, double, const double*) const {}
};

// The fit of one block (a.blocks[] entry `block`: a time, a camera or a marker index).  Every lane of `lanes` calls it with the same
// arguments and leaves with the same result; the lane whose first() is 0 writes it.  kKinds says which kinds the caller can ask for, so
// that a kernel carries the code of its own kinds only:
//   RESECT_ANY              the host: three kinds, markers_flagged read
//   RESECT_TIME_OR_CAMERA   the two kernels BOTH starts launch for times and cameras — the whole-rig start's code as it was before markers
//                           were fitted, instruction for instruction, so that start keeps its bits and the scene start with every marker
//                           flagged gives the same ones.  markers_flagged is not read: the scene start hides a detection whose marker is
//                           not known behind the index of a flag that is never set (k_scene_mask_index below)
//   RESECT_MARKER           the marker launches
enum { RESECT_ANY = -1, RESECT_TIME_OR_CAMERA = -2 };
template <int kKinds, bool kBoth = false, class Lanes>
RSBA_HD void ResectBlockOf(const ResectionArgs& a, int which, int block, Lanes& lanes) {
  constexpr bool kMarkerToo = kKinds != RESECT_TIME_OR_CAMERA;
  const bool marker = kKinds == RESECT_MARKER || (kKinds == RESECT_ANY && which == RESECT_MARKER);
  const int kind = marker ? RESECT_MARKER : which;
  const bool flagged = kKinds == RESECT_ANY && a.markers_flagged != 0;
  const int pb = marker ? a.C + a.T + block : which == RESECT_TIME ? a.C + block : block;   // the block's place in [C | T | M]
  const int lo = a.list_ptr[block], hi = a.list_ptr[block + 1];
  const bool refit = a.known[pb] != 0;
  auto usable = [&](int o) {
    if (marker) return a.known[a.camera_index[o]] != 0 && a.known[a.C + a.time_index[o]] != 0;
    const bool other = a.known[which == RESECT_TIME ? a.camera_index[o] : a.C + a.time_index[o]] != 0;
    return flagged ? other && a.known[a.C + a.T + a.marker_index[o]] != 0 : other;
  };

  double counted[1] = {0.0};   // the usable detections: how many
  for (int k = lo + lanes.first(); k < hi; k += lanes.stride()) counted[0] += usable(a.list_obs[k]) ? 1.0 : 0.0;
  lanes.Sum(counted);
  const double usable_count = counted[0];

  // the block's cost, J'J, J'r and smallest depth at a pose over its usable detections
  auto lin = [&](const double* at, double* cost, double* A, double* g, double* minz) {
    const double none[4] = {0.0, 0.0, 0.0, 0.0};
    double cc[CC_STRIDE], v[kResectionSums], z = DBL_MAX;
    CameraConstants(at, none, cc);
    RSBA_UNROLL
    for (int q = 0; q < kResectionSums; ++q) v[q] = 0.0;
    for (int k = lo + lanes.first(); k < hi; k += lanes.stride()) {
      const int o = a.list_obs[k];
      if (!usable(o)) continue;
      const double *cam, *tim, *mar;
      ObservationBlocks(a, o, &cam, &tim, &mar);
      ResectionFrame f;
      ResectionFrameOf<kMarkerToo>(kind, cam, tim, mar, a.half, &f);
      const int c = a.camera_index[o];
      double k5[5], c8[8];
      RSBA_UNROLL
      for (int q = 0; q < 5; ++q) k5[q] = a.distortion ? a.distortion[5 * (size_t)c + q] : 0.0;
      RSBA_UNROLL
      for (int q = 0; q < 8; ++q) c8[q] = a.observations[8 * (size_t)o + q];
      ResectionAccumulate(cc, f, a.intrinsics + 4 * (size_t)c, k5, c8, &v[0], v + 1, v + 22, &z);
    }
    lanes.Sum(v);
    lanes.Min(&z);
    *cost = v[0];
    RSBA_UNROLL
    for (int q = 0; q < 21; ++q) A[q] = v[1 + q];
    RSBA_UNROLL
    for (int q = 0; q < 6; ++q) g[q] = v[22 + q];
    *minz = z;
  };

  double p[6], best = DBL_MAX;
  bool have = false;
  if (refit) {
    double c0, A[21], g[6], z;
    RSBA_UNROLL
    for (int q = 0; q < 6; ++q) p[q] = a.parameters[6 * (size_t)pb + q];
    lin(p, &c0, A, g, &z);
    have = usable_count > 0.0 && FiniteValue(c0) && z > 0.0;
  } else {
    double prev_key = -1.0;   // (an own-fit RMS is >= 0)
    int prev_o = -1;
    for (int k4 = 0; k4 < 4; ++k4) {
      // the next detection in (own-fit RMS, observation index) order
      double key = DBL_MAX;
      int idx = INT_MAX;
      for (int k = lo + lanes.first(); k < hi; k += lanes.stride()) {
        const int o = a.list_obs[k];
        if (!usable(o) || a.own_status[o] > MARKER_POSE_ITERATION_CAP) continue;
        const double e = a.own_rms[o];
        const bool after = e > prev_key || (e == prev_key && o > prev_o);
        if (after && (e < key || (e == key && o < idx))) { key = e; idx = o; }
      }
      lanes.ArgMin(&key, &idx);
      if (idx == INT_MAX) break;
      prev_key = key; prev_o = idx;
      const double *cam, *tim, *mar;
      ObservationBlocks(a, idx, &cam, &tim, &mar);
      if constexpr (kBoth) {
        // the detection's own fit, then its second solution where it has one
        for (int sol = 0; sol < 2; ++sol) {
          if (sol == 1 && a.own_status2[idx] > MARKER_POSE_ITERATION_CAP) break;
          const double* from = sol == 1 ? a.own_pose2 : a.own_pose;
          double own[6], cand[6], c0, A[21], g[6], z;
          RSBA_UNROLL
          for (int q = 0; q < 6; ++q) own[q] = from[6 * (size_t)idx + q];
          ResectionCandidate<kMarkerToo>(kind, own, cam, tim, mar, cand);
          bool fine = true;
          RSBA_UNROLL
          for (int q = 0; q < 6; ++q) fine = fine && FiniteValue(cand[q]);
          if (!fine) continue;
          lin(cand, &c0, A, g, &z);
          if (FiniteValue(c0) && z > 0.0 && (!have || c0 < best)) {
            have = true;
            best = c0;
            RSBA_UNROLL
            for (int q = 0; q < 6; ++q) p[q] = cand[q];
          }
        }
        continue;
      }
      // Without kBoth: these lines as they always were, NOT folded into the loop above as its one-trip case.  Folded, the three unflagged
      // kernels came out with other register names and two moves in another order — the same arithmetic, but no longer the code that
      // the whole-rig start's bits were recorded with; as they stand, those kernels match their earlier code instruction for instruction.
      double own[6], cand[6], c0, A[21], g[6], z;
      RSBA_UNROLL
      for (int q = 0; q < 6; ++q) own[q] = a.own_pose[6 * (size_t)idx + q];
      ResectionCandidate<kMarkerToo>(kind, own, cam, tim, mar, cand);
      bool fine = true;
      RSBA_UNROLL
      for (int q = 0; q < 6; ++q) fine = fine && FiniteValue(cand[q]);
      if (!fine) continue;
      lin(cand, &c0, A, g, &z);
      if (FiniteValue(c0) && z > 0.0 && (!have || c0 < best)) {
        have = true;
        best = c0;
        RSBA_UNROLL
        for (int q = 0; q < 6; ++q) p[q] = cand[q];
      }
    }
  }
  if (!refit) lanes.ChosenStart(have, best, p);
  bool ok = have;
  double cost = 0.0;
  int iterations = 0;
  const int st = MarkerPoseMinimise<true>(lin, &ok, p, &cost, &iterations);
  if (lanes.first() != 0) return;
  if (ok) {
    RSBA_UNROLL
    for (int q = 0; q < 6; ++q) a.parameters[6 * (size_t)pb + q] = p[q];
    a.status[pb] = st;
    a.rms[pb] = sqrt(cost / (8.0 * usable_count));
    a.iterations[pb] = iterations;
    a.known[pb] = 1;
  } else if (!refit) {
    a.status[pb] = usable_count > 0.0 ? BLOCK_DEGENERATE : BLOCK_UNREACHED;
    a.rms[pb] = -1.0;
    a.iterations[pb] = 0;
  }
}

template <bool kBoth = false, class Lanes>
RSBA_HD void ResectBlock(const ResectionArgs& a, int which, int block, Lanes& lanes) {
  ResectBlockOf<RESECT_ANY, kBoth>(a, which, block, lanes);
}

#if defined(__HIPCC__)
// A wavefront (kWorkgroup = false) or the four wavefronts of a 256-lane workgroup (true) as the lanes of one block.  Sums meet by an xor
// butterfly: lane i adds lane i ^ 32's value, then i ^ 16's, ... — the same pairs in every lane (a + b == b + a), so all 64 hold the
// same bits.  The wavefronts' sums are then added in wavefront order from LDS by every lane.
template <bool kWorkgroup>
struct DeviceLanes {
  double* lds;   // kWorkgroup: 4 x kResectionSums doubles
  __device__ int first() const { return kWorkgroup ? (int)threadIdx.x : (int)(threadIdx.x & 63); }
  __device__ int stride() const { return kWorkgroup ? 256 : 64; }
  __device__ void ChosenStart(bool, double, const double*) const {}
  template <int N> __device__ void Sum(double (&v)[N]) const {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
      for (int q = 0; q < N; ++q) v[q] += __shfl_xor(v[q], off, 64);
    }
    if constexpr (kWorkgroup) {
      const int wave = threadIdx.x >> 6;
      if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) lds[wave * N + q] = v[q];
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < N; ++q) v[q] = ((lds[q] + lds[N + q]) + lds[2 * N + q]) + lds[3 * N + q];
      __syncthreads();
    }
  }
  __device__ void Min(double* z) const {
    double v = *z;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    if constexpr (kWorkgroup) {
      if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
      __syncthreads();
      v = fmin(fmin(lds[0], lds[1]), fmin(lds[2], lds[3]));
      __syncthreads();
    }
    *z = v;
  }
  __device__ void ArgMin(double* key, int* idx) const {
    double k = *key;
    int i = *idx;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double k2 = __shfl_xor(k, off, 64);
      const int i2 = __shfl_xor(i, off, 64);
      if (k2 < k || (k2 == k && i2 < i)) { k = k2; i = i2; }
    }
    if constexpr (kWorkgroup) {
      if ((threadIdx.x & 63) == 0) { lds[2 * (threadIdx.x >> 6)] = k; lds[2 * (threadIdx.x >> 6) + 1] = (double)i; }
      __syncthreads();
      k = lds[0]; i = (int)lds[1];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const double k2 = lds[2 * w];
        const int i2 = (int)lds[2 * w + 1];
        if (k2 < k || (k2 == k && i2 < i)) { k = k2; i = i2; }
      }
      __syncthreads();
    }
    *key = k;
    *idx = i;
  }
};

// kWorkgroup = false: a block per wavefront, four to a workgroup (times: tens of detections each); true: a block per workgroup (cameras:
// tens of thousands).  A wavefront past the launch's last block leaves at once; inside a workgroup-wide block every barrier is reached by
// all four wavefronts, since they hold the same sums and take the same branches.  kMarker = true: the scene start's marker launches — a
// marker, like a camera, is a block per workgroup (in a large rig it is named by up to C x T detections).  kBoth = true: the three
// instances of the flagged start, with both solutions of a detection among a block's candidates; the three without it carry none of that.
template <bool kWorkgroup, bool kMarker = false, bool kBoth = false>
__global__ __launch_bounds__(256) void k_block_resection(ResectionArgs a, int which) {
  __shared__ double lds[kWorkgroup ? 4 * kResectionSums : 1];
  const int i = kWorkgroup ? (int)blockIdx.x : (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (i >= a.num_blocks) return;
  DeviceLanes<kWorkgroup> lanes{lds};
  ResectBlockOf<kMarker ? RESECT_MARKER : RESECT_TIME_OR_CAMERA, kBoth>(a, which, a.blocks[i], lanes);
}

// The scene start's rule for a time or a camera block — a detection counts only when its marker is known too — without another
// instruction in the two kernels above: before such a launch, out[o] is index[o] (the camera index for a time launch, the time index for
// a camera launch) where the detection's marker is flagged, and `hidden` where it is not — the index at which those kernels find the
// one flag of known[] that no launch sets.  They read an index further only for a usable detection.  A thread per detection.
__global__ __launch_bounds__(256) void k_scene_mask_index(int64_t n, const int32_t* index, const int32_t* marker_index, const uint8_t* marker_known,
                                                          int32_t hidden, int32_t* out) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= n) return;
  out[o] = marker_known[marker_index[o]] != 0 ? index[o] : hidden;
}
#endif

}  // namespace rsba
