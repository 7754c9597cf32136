// Pose of ONE square marker from its four image corners: what aruco::estimatePoseSingleMarkers computes per detection
// (Main_Calibration/correspondencer.cpp:80 of the reference), the step between the detected corners and the time blocks
// (:100-127).  Plain C++ for host and device (RSBA_HD), no HIP calls: rsba_marker_pose_from_corners and
// rsba_problem_initial_time_poses run it on the host, k_marker_pose (ba_solver.hip) one detection per thread.
//
//   object points   the marker's corners in its own frame, (-s/2, s/2, 0), (s/2, s/2, 0), (s/2, -s/2, 0), (-s/2, -s/2, 0):
//                   top-left, top-right, bottom-right, bottom-left, the order of the detections
//   pose            (rvec, tvec) with p_cam = R(rvec) p_marker + tvec
//   contract        the local minimiser of the four corners' reprojection error under the project's camera model
//                   (ProjectCorner<true> / DistortNormalised) reached from the homography of the square: what OpenCV 4.0.1's
//                   SOLVEPNP_ITERATIVE does for a planar target.  No digit-for-digit claim against OpenCV; the time rows of the
//                   committed hongo correspondence.txt pin the basin (tests/test_capi_marker_pose_host.py).
//
//   1. the corners' normalised points of the ideal pinhole camera: UndistortPoints' fixed-point iteration (ba_initial_guess.cpp);
//      all-zero coefficients skip it
//   2. the homography of the square onto them.  Four points fix it exactly, so the null vector of the 8 x 9 DLT system IS the
//      projective map of the unit square onto the quadrilateral, which has a closed form (Heckbert 1989, "Fundamentals of texture
//      mapping and image warping", §2.2.3): two 2 x 2 determinant quotients, no decomposition, nothing indexed.  It is normalised so that
//      the bottom-left corner has depth factor one; the other three must be positive with it.
//   3. r1 = h1 / |h1|, r2 = h2 / |h2|, t = 2 h3 / (|h1| + |h2|), and the rotation nearest to [r1 r2 r1 x r2]: M'M of that matrix is
//      [[1 c 0] [c 1 0] [0 0 1 - c^2]], so its polar factor is the symmetric orthonormalisation of the pair — the unit bisectors
//      of r1 and r2 turned back by 45 degrees — and their cross product
//   4. Levenberg-Marquardt on (rvec, tvec) with the analytic rows of ba_math.hpp (a pose block's rule: d r / d t = Q,
//      d r / d w = [w* x Q_i] Jl): damping lambda diag(J'J), lambda0 = 1e-3; a candidate is accepted when the cost does not rise;
//      lambda /= 10 (floor 1e-15) on acceptance, *= 10 on rejection; stop when the step's max-norm is below 1e-12 (1 + max |p|);
//      at most kMarkerPoseMaxIterations steps.  The loop is MarkerPoseMinimise, shared with the block resection (ba_resection.hpp).
//
// Everything is scalars and fixed-size arrays indexed by constants once the loops are unrolled: on the device the 21 entries of
// J'J, the gradient, the pose and the 6 x 6 Cholesky factor live in registers (profiles/marker_pose_kernel_resources.txt: no scratch).
// A lane that has finished leaves the loop; nothing is exchanged between lanes, so a detection's bits do not depend on its place.
//
// The two-fold ambiguity of a planar target: FitMarkerPose returns the minimiser of the basin its homography start falls into, which for
// a small or nearly frontal marker is the mirror image in a quarter to a third of the cases, at an RMS that does not give it away.
// FitMarkerPoseBoth (below) returns the other minimiser too, reached from the mirrored start (MirrorMarkerPose; no IPPE closed form).
// Which of the two is the marker's pose one detection cannot say: the block resection decides by a block's cost over several detections.
#pragma once
#include <cfloat>
#include <cmath>

#include "ba_math.hpp"

#if defined(__HIPCC__)
#define RSBA_UNROLL _Pragma("unroll")
#else
#define RSBA_UNROLL
#endif

namespace rsba {

enum {
  MARKER_POSE_CONVERGED = 0,    // the step fell below the tolerance
  MARKER_POSE_ITERATION_CAP = 1,   // the last iterate and its RMS
  MARKER_POSE_DEGENERATE = 2,   // singular homography, non-positive depth, a non-finite intermediate, an undistortion that did not converge:
                                // pose zeros, RMS -1
  kMarkerPoseMaxIterations = 400   // well-posed detections take ~15 steps; frontal 30-pixel markers creep along a flat valley: of 60 000 detections of the
                                   // 8 x 5000 x 16 problem 165 are unfinished after 100 steps, 38 after 200, 7 after 400 (and hongo has one that takes 191)
};

RSBA_HD bool FiniteValue(double x) { return fabs(x) <= DBL_MAX; }   // false for NaN too

// One point of UndistortPoints: the distorted normalised point (xd, yd) -> the ideal one, the same iteration and stopping rule (until
// both updates are below 1e-14 within 50 steps, then up to four more until nothing moves).
RSBA_HD bool UndistortNormalisedPoint(double xd, double yd, const double k[5], double* xo, double* yo) {
  const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4];
  double x = xd, y = yd;
  int polish = 0;
  for (int it = 0; it < 54; ++it) {
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    if (!(rad > 0.0)) return false;
    const double xn = (xd - (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) / rad;
    const double yn = (yd - (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)) / rad;
    if (!FiniteValue(xn) || !FiniteValue(yn)) return false;
    const bool same = xn == x && yn == y;
    const bool small = fabs(xn - x) < 1e-14 && fabs(yn - y) < 1e-14;
    x = xn; y = yn;
    if (small) {
      if (same || ++polish > 4) { *xo = x; *yo = y; return true; }
    } else if (polish > 0 || it >= 49) {
      return false;   // no contraction at this radius
    }
  }
  return false;
}

// Angle-axis of a rotation matrix (row-major) through the quaternion, as ceres::RotationMatrixToAngleAxis goes: stable at every angle, no
// indexed access.
RSBA_HD void RotationMatrixToRvec(const double* R, double* w) {
  const double tr = R[0] + R[4] + R[8];
  double qw, qx, qy, qz;   // four times the quaternion times its largest component
  if (tr > 0.0) { qw = 1.0 + tr; qx = R[7] - R[5]; qy = R[2] - R[6]; qz = R[3] - R[1]; }
  else if (R[0] >= R[4] && R[0] >= R[8]) { qx = 1.0 + R[0] - R[4] - R[8]; qy = R[3] + R[1]; qz = R[6] + R[2]; qw = R[7] - R[5]; }
  else if (R[4] >= R[8]) { qy = 1.0 + R[4] - R[0] - R[8]; qx = R[1] + R[3]; qz = R[7] + R[5]; qw = R[2] - R[6]; }
  else { qz = 1.0 + R[8] - R[0] - R[4]; qx = R[2] + R[6]; qy = R[5] + R[7]; qw = R[3] - R[1]; }
  if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
  const double s = sqrt(qx * qx + qy * qy + qz * qz);
  const double f = s > 1e-12 * qw ? 2.0 * atan2(s, qw) / s : 2.0 / qw;   // theta / sin(theta / 2) -> 2 at theta = 0
  w[0] = f * qx; w[1] = f * qy; w[2] = f * qz;
}

// The start of the fit from the four normalised corners (x[j], y[j]: top-left, top-right, bottom-right, bottom-left).
RSBA_HD bool MarkerPoseFromHomography(const double x[4], const double y[4], double side, double pose[6]) {
  // Heckbert's square-to-quadrilateral map, (0,0) (1,0) (1,1) (0,1) -> bottom-left, bottom-right, top-right, top-left:
  // [a b c; d e f; g h 1] (u, v, 1)' with the marker's X = s (u - 1/2), Y = s (v - 1/2)
  const double x0 = x[3], y0 = y[3], x1 = x[2], y1 = y[2], x2 = x[1], y2 = y[1], x3 = x[0], y3 = y[0];
  const double sx = (x0 - x1) + (x2 - x3), sy = (y0 - y1) + (y2 - y3);
  const double dx1 = x1 - x2, dx2 = x3 - x2, dy1 = y1 - y2, dy2 = y3 - y2;
  const double m0 = dx1 * dy2, m1 = dx2 * dy1, den = m0 - m1;
  if (!(fabs(den) > 1e-12 * (fabs(m0) + fabs(m1)))) return false;   // three corners on a line (or all equal; NaN lands here too)
  const double g = (sx * dy2 - dx2 * sy) / den, h = (dx1 * sy - sx * dy1) / den;
  // depth factors of the corners (bottom-left: 1): of one sign and none vanishing, or the quadrilateral is no image of a square in front
  const double w1 = 1.0 + g, w2 = 1.0 + g + h, w3 = 1.0 + h;
  const double wmax = fmax(fmax(1.0, w1), fmax(w2, w3)), wmin = fmin(fmin(1.0, w1), fmin(w2, w3));
  if (!(wmin > 1e-9 * wmax) || !FiniteValue(wmax)) return false;
  const double a = (x1 - x0) + g * x1, b = (x3 - x0) + h * x3, d = (y1 - y0) + g * y1, e = (y3 - y0) + h * y3;
  const double is = 1.0 / side;
  const double h1x = a * is, h1y = d * is, h1z = g * is;
  const double h2x = b * is, h2y = e * is, h2z = h * is;
  const double h3x = 0.5 * (a + b) + x0, h3y = 0.5 * (d + e) + y0, h3z = 0.5 * (g + h) + 1.0;
  const double n1 = sqrt(h1x * h1x + h1y * h1y + h1z * h1z), n2 = sqrt(h2x * h2x + h2y * h2y + h2z * h2z);
  if (!(n1 > 0.0) || !(n2 > 0.0)) return false;
  const double i1 = 1.0 / n1, i2 = 1.0 / n2, ts = 2.0 / (n1 + n2);
  const double r1x = h1x * i1, r1y = h1y * i1, r1z = h1z * i1, r2x = h2x * i2, r2y = h2y * i2, r2z = h2z * i2;
  // unit bisectors of the pair (orthogonal: |r1| = |r2|)
  const double cx = r1x + r2x, cy = r1y + r2y, cz = r1z + r2z, dx = r1x - r2x, dy = r1y - r2y, dz = r1z - r2z;
  const double nc = sqrt(cx * cx + cy * cy + cz * cz), nd = sqrt(dx * dx + dy * dy + dz * dz);
  if (!(nc > 1e-9) || !(nd > 1e-9)) return false;   // h1 and h2 parallel
  const double ic = 0.70710678118654752440 / nc, id = 0.70710678118654752440 / nd;
  double R[9];
  R[0] = cx * ic + dx * id; R[3] = cy * ic + dy * id; R[6] = cz * ic + dz * id;
  R[1] = cx * ic - dx * id; R[4] = cy * ic - dy * id; R[7] = cz * ic - dz * id;
  R[2] = R[3] * R[7] - R[6] * R[4]; R[5] = R[6] * R[1] - R[0] * R[7]; R[8] = R[0] * R[4] - R[3] * R[1];
  RotationMatrixToRvec(R, pose);
  pose[3] = h3x * ts; pose[4] = h3y * ts; pose[5] = h3z * ts;
  bool ok = pose[5] > 0.0;
  RSBA_UNROLL
  for (int q = 0; q < 6; ++q) ok = ok && FiniteValue(pose[q]);
  return ok;
}

// index of (a, b), a <= b, in the packed upper triangle of a symmetric 6 x 6
RSBA_HD constexpr int Sym6(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }

// Cost (sum of the eight squared residuals), J'J (packed, 21), J'r and the smallest depth at the pose p.
RSBA_HD void MarkerPoseLinearise(const double p[6], const double* c8, const double* intr4, const double k5[5], double half,
                                 double* cost_out, double A[21], double g[6], double* min_depth) {
  double cc[CC_STRIDE];
  CameraConstants(p, intr4, cc);
  const double* R = cc + CC_R;
  const double* K = cc + CC_K;
  const bool small = cc[CC_SMALL] != 0.0;
  const double fx = intr4[0], fy = intr4[1], ppx = intr4[2], ppy = intr4[3];
  double cost = 0.0, minz = DBL_MAX;
  RSBA_UNROLL
  for (int q = 0; q < 21; ++q) A[q] = 0.0;
  RSBA_UNROLL
  for (int q = 0; q < 6; ++q) g[q] = 0.0;
  RSBA_UNROLL
  for (int j = 0; j < 4; ++j) {
    const double X = (j == 1 || j == 2) ? half : -half, Y = j < 2 ? half : -half;
    const double q0 = R[0] * X + R[1] * Y, q1 = R[3] * X + R[4] * Y, q2 = R[6] * X + R[7] * Y;
    const double P0 = q0 + cc[CC_T], P1 = q1 + cc[CC_T + 1], P2 = q2 + cc[CC_T + 2];
    double r[2], Q[6];
    ProjectCorner<true>(P0, P1, P2, fx, fy, ppx, ppy, k5, c8[2 * j], c8[2 * j + 1], r, Q);
    minz = fmin(minz, P2);
    const double w0 = small ? X : q0, w1 = small ? Y : q1, w2 = small ? 0.0 : q2;
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
  *cost_out = cost;
  *min_depth = minz;
}

// d = -(A + lambda diag(A))^-1 g by Cholesky; false (d zeros) when a pivot is not positive or the step is not finite.
RSBA_HD bool MarkerPoseStep(const double A[21], const double g[6], double lambda, double d[6]) {
  double L[21];   // lower triangle by rows: L(i, j) at i (i + 1) / 2 + j
  bool ok = true;
  RSBA_UNROLL
  for (int j = 0; j < 6; ++j) {
    double s = A[Sym6(j, j)] * (1.0 + lambda);
    RSBA_UNROLL
    for (int k = 0; k < j; ++k) s -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
    ok = ok && s > 0.0;
    const double l = sqrt(ok ? s : 1.0), il = 1.0 / l;
    L[j * (j + 1) / 2 + j] = l;
    RSBA_UNROLL
    for (int i = j + 1; i < 6; ++i) {
      double t = A[Sym6(j, i)];
      RSBA_UNROLL
      for (int k = 0; k < j; ++k) t -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
      L[i * (i + 1) / 2 + j] = t * il;
    }
  }
  double z[6];
  RSBA_UNROLL
  for (int i = 0; i < 6; ++i) {
    double t = -g[i];
    RSBA_UNROLL
    for (int k = 0; k < i; ++k) t -= L[i * (i + 1) / 2 + k] * z[k];
    z[i] = t / L[i * (i + 1) / 2 + i];
  }
  RSBA_UNROLL
  for (int i = 5; i >= 0; --i) {
    double t = z[i];
    RSBA_UNROLL
    for (int k = i + 1; k < 6; ++k) t -= L[k * (k + 1) / 2 + i] * d[k];
    d[i] = t / L[i * (i + 1) / 2 + i];
  }
  RSBA_UNROLL
  for (int i = 0; i < 6; ++i) ok = ok && FiniteValue(d[i]);
  RSBA_UNROLL
  for (int i = 0; i < 6; ++i) d[i] = ok ? d[i] : 0.0;
  return ok;
}

// The Levenberg-Marquardt loop on six pose parameters, shared by the single-marker fit below and the block resection
// (ba_resection.hpp): lin(p, &cost, A, g, &min_depth) linearises the objective at p.  From p (when *ok) the loop damps with
// lambda diag(J'J), accepts a candidate whose cost does not rise and whose points stay in front, and stops on a small step or at the
// iteration cap.  *ok ends false when the start, or the last iterate, is unusable; p, *cost and *iterations are the last accepted
// iterate's.  Returns MARKER_POSE_CONVERGED or MARKER_POSE_ITERATION_CAP.
// kSufficientDecrease (the block resection): a candidate must also realise a quarter of the decrease the damped model predicts,
// cost - cn >= (-2 g'd - d'Ad) / 4, the usual trust-region threshold below which the damping is raised.  With residuals of several pixels
// at the minimum J'J underestimates the curvature along a board's tilt by a factor near two; a step twice too long leaves the cost where
// it was, is accepted under "does not rise", lambda relaxes, the next step is rejected, and the pair repeats at the edge of stability
// (measured: a factor 0.99 a step, 1.6e-4 from the minimiser after 400 steps).  The single-marker fit, whose eight residuals are noise at
// its minimum, keeps its rule and its bits: the test is compiled out.
template <bool kSufficientDecrease = false, class Linearise>
RSBA_HD int MarkerPoseMinimise(Linearise&& lin, bool* ok_io, double p[6], double* cost_out, int* iterations) {
  bool ok = *ok_io;
  double cost = 0.0, A[21], g[6], minz = 0.0;
  if (ok) {
    lin(p, &cost, A, g, &minz);
    ok = FiniteValue(cost) && minz > 0.0;
  }
  int status = MARKER_POSE_ITERATION_CAP, it = 0;
  double lambda = 1e-3;
  for (; ok && it < kMarkerPoseMaxIterations; ++it) {
    double d[6], pn[6], An[21], gn[6], cn, zn;
    const bool solved = MarkerPoseStep(A, g, lambda, d);
    double dmax = 0.0, pmax = 0.0;
    RSBA_UNROLL
    for (int q = 0; q < 6; ++q) { dmax = fmax(dmax, fabs(d[q])); pmax = fmax(pmax, fabs(p[q])); pn[q] = p[q] + d[q]; }
    lin(pn, &cn, An, gn, &zn);
    bool accept = solved && FiniteValue(cn) && zn > 0.0 && cn <= cost;
    if constexpr (kSufficientDecrease) {
      double gd = 0.0, dAd = 0.0;
      RSBA_UNROLL
      for (int a = 0; a < 6; ++a) {
        gd += g[a] * d[a];
        RSBA_UNROLL
        for (int b = 0; b < 6; ++b) dAd += d[a] * A[a <= b ? Sym6(a, b) : Sym6(b, a)] * d[b];
      }
      accept = accept && 4.0 * (cost - cn) >= -2.0 * gd - dAd;
    }
    if (accept) {
      cost = cn;
      RSBA_UNROLL
      for (int q = 0; q < 6; ++q) { p[q] = pn[q]; g[q] = gn[q]; }
      RSBA_UNROLL
      for (int q = 0; q < 21; ++q) A[q] = An[q];
      lambda = fmax(lambda * 0.1, 1e-15);
    } else {
      lambda *= 10.0;
    }
    if (solved && dmax < 1e-12 * (1.0 + pmax)) { status = MARKER_POSE_CONVERGED; break; }
  }
  RSBA_UNROLL
  for (int q = 0; q < 6; ++q) ok = ok && FiniteValue(p[q]);
  *ok_io = ok;
  *cost_out = cost;
  *iterations = it;
  return status;
}

// The fit.  corners8: 4 x (u, v); dist5 may be null (no distortion).  Returns the status; pose6 and *rms are always written.
RSBA_HD int FitMarkerPose(const double* corners8, const double* intr4, const double* dist5, double marker_side, double* pose6, double* rms) {
  double k5[5];
  bool any = false;
  RSBA_UNROLL
  for (int q = 0; q < 5; ++q) { k5[q] = dist5 ? dist5[q] : 0.0; any = any || k5[q] != 0.0; }
  const double fx = intr4[0], fy = intr4[1], ppx = intr4[2], ppy = intr4[3];
  double x[4], y[4], p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok = true;
  RSBA_UNROLL
  for (int j = 0; j < 4; ++j) {
    x[j] = (corners8[2 * j] - ppx) / fx;
    y[j] = (corners8[2 * j + 1] - ppy) / fy;
    if (any) ok = UndistortNormalisedPoint(x[j], y[j], k5, &x[j], &y[j]) && ok;
  }
  ok = ok && MarkerPoseFromHomography(x, y, marker_side, p);
  const double half = 0.5 * marker_side;
  double cost = 0.0;
  int iterations = 0;
  const int status = MarkerPoseMinimise([&](const double* at, double* c, double* A, double* g, double* z) {
    MarkerPoseLinearise(at, corners8, intr4, k5, half, c, A, g, z);
  }, &ok, p, &cost, &iterations);
  if (!ok) {
    RSBA_UNROLL
    for (int q = 0; q < 6; ++q) pose6[q] = 0.0;
    *rms = -1.0;
    return MARKER_POSE_DEGENERATE;
  }
  RSBA_UNROLL
  for (int q = 0; q < 6; ++q) pose6[q] = p[q];
  *rms = sqrt(cost * 0.125);
  return status;
}

// The other pose of a planar target.  With R = R(rvec), t = tvec and v = t / |t| (the line of sight to the marker's centre):
//   R' = (I - 2 v v') R diag(1, 1, -1),   t' = t
// The marker's two in-plane axes are reflected in the plane perpendicular to the line of sight (its normal follows as their cross
// product: the third column changes sign once more), so the tilt about the line of sight changes sign and the corners' image under
// weak perspective stays where it was.  Two reflections: a proper rotation; applied twice it returns the pose up to rounding.
// out6 may be pose6.  t = 0 gives a non-finite pose (the caller's start check refuses it).
RSBA_HD void MirrorMarkerPose(const double* pose6, double* out6) {
  const double none[4] = {0.0, 0.0, 0.0, 0.0};
  double cc[CC_STRIDE];
  CameraConstants(pose6, none, cc);
  const double* R = cc + CC_R;
  const double t0 = pose6[3], t1 = pose6[4], t2 = pose6[5];
  const double in = 1.0 / sqrt(t0 * t0 + t1 * t1 + t2 * t2);
  const double v0 = t0 * in, v1 = t1 * in, v2 = t2 * in;
  double M[9];   // R diag(1, 1, -1), then M - 2 v (v' M)
  RSBA_UNROLL
  for (int i = 0; i < 3; ++i) { M[3 * i] = R[3 * i]; M[3 * i + 1] = R[3 * i + 1]; M[3 * i + 2] = -R[3 * i + 2]; }
  RSBA_UNROLL
  for (int j = 0; j < 3; ++j) {
    const double s = 2.0 * (v0 * M[j] + v1 * M[3 + j] + v2 * M[6 + j]);
    M[j] -= v0 * s; M[3 + j] -= v1 * s; M[6 + j] -= v2 * s;
  }
  double w[3];
  RotationMatrixToRvec(M, w);
  out6[0] = w[0]; out6[1] = w[1]; out6[2] = w[2];
  out6[3] = t0; out6[4] = t1; out6[5] = t2;
}

enum {
  MARKER_POSE_SAME = 3   // the second solution only: the fit from the mirrored start ended at the first solution; pose zeros, RMS -1
};

// Two fits of one detection count as one solution when no entry of their rotation matrices or translations differs by this much.  A
// definition: the stopping rule leaves about 1e-9 between two runs into the same minimiser, and a mirror image is about 0.1 rad away.
constexpr double kMarkerPoseSameBelow = 1e-5;

// The second solution of a detection whose first one (pose0, status0: FitMarkerPose's) is at hand: MarkerPoseMinimise — FitMarkerPose's
// instance and its linearisation — started from MirrorMarkerPose(pose0).  Returns its status, pose1 and *rms1 are always written:
//   0, 1   as FitMarkerPose: the minimiser reached from the mirrored start (1: the last iterate at the cap)
//   2      there is no first solution (status0 = 2), or the mirrored start is unusable (not finite, or a corner behind the camera):
//          pose zeros, RMS -1
//   3      MARKER_POSE_SAME: the fit slid back to the first solution (a close-up, where perspective leaves one minimum): pose zeros, RMS -1
// Shared by FitMarkerPoseBoth (the host) and k_marker_pose_mirror (ba_solver.hip), so both run the same arithmetic.
RSBA_HD int SecondMarkerPose(const double* corners8, const double* intr4, const double* dist5, double marker_side, const double* pose0, int status0,
                             double* pose1, double* rms1) {
  double k5[5], p[6];
  RSBA_UNROLL
  for (int q = 0; q < 5; ++q) k5[q] = dist5 ? dist5[q] : 0.0;
  bool ok = status0 == MARKER_POSE_CONVERGED || status0 == MARKER_POSE_ITERATION_CAP;
  int status = MARKER_POSE_DEGENERATE;
  double cost = 0.0;
  if (ok) {
    MirrorMarkerPose(pose0, p);
    RSBA_UNROLL
    for (int q = 0; q < 6; ++q) ok = ok && FiniteValue(p[q]);
    const double half = 0.5 * marker_side;
    int iterations = 0;
    status = MarkerPoseMinimise([&](const double* at, double* c, double* A, double* g, double* z) {
      MarkerPoseLinearise(at, corners8, intr4, k5, half, c, A, g, z);
    }, &ok, p, &cost, &iterations);
    if (!ok) status = MARKER_POSE_DEGENERATE;
  }
  if (ok) {
    const double none[4] = {0.0, 0.0, 0.0, 0.0};
    double ca[CC_STRIDE], cb[CC_STRIDE], far = 0.0;
    CameraConstants(pose0, none, ca);
    CameraConstants(p, none, cb);
    RSBA_UNROLL
    for (int q = 0; q < 9; ++q) far = fmax(far, fabs(ca[CC_R + q] - cb[CC_R + q]));
    RSBA_UNROLL
    for (int q = 0; q < 3; ++q) far = fmax(far, fabs(pose0[3 + q] - p[3 + q]));
    if (far < kMarkerPoseSameBelow) { ok = false; status = MARKER_POSE_SAME; }
  }
  RSBA_UNROLL
  for (int q = 0; q < 6; ++q) pose1[q] = ok ? p[q] : 0.0;
  *rms1 = ok ? sqrt(cost * 0.125) : -1.0;
  return status;
}

// Both poses of a planar marker.  Solution 0 is FitMarkerPose, called as it is (its bits are that routine's); solution 1 is
// SecondMarkerPose.  poses12 = (solution 0, solution 1), rms2 and status2 likewise, in that fixed order: not sorted — a caller compares
// the two RMS values, or, better, the cost of a block over several detections (ba_resection.hpp), since one marker's RMS does not
// tell a small, nearly frontal marker's pose from its mirror image.
RSBA_HD void FitMarkerPoseBoth(const double* corners8, const double* intr4, const double* dist5, double marker_side, double* poses12, double* rms2,
                               int* status2) {
  status2[0] = FitMarkerPose(corners8, intr4, dist5, marker_side, poses12, &rms2[0]);
  status2[1] = SecondMarkerPose(corners8, intr4, dist5, marker_side, poses12, status2[0], poses12 + 6, &rms2[1]);
}

}  // namespace rsba
