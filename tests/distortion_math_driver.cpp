// Stand-alone check of the lens-distortion arithmetic of the host build (csrc/ba_math.hpp ProjectCorner / DistortNormalised,
// ba_initial_guess.cpp UndistortPoints), built with -fsanitize=address,undefined by tests/test_distortion_math_host.py:
//   1. ProjectCorner<true>'s Q (2 x 3) against a dual-number evaluation of the same projection (DistortNormalised on Dual3), over a
//      grid of the image and the test coefficient sets;
//   2. ProjectCorner<true> with zero coefficients against ProjectCorner<false> (rounding, not bits) and ProjectCorner<false> against
//      the pinhole expressions written out (bits); MarkerCornerResidualJacobian<true> with zero coefficients against <false>;
//   3. rsba_undistort_points: distort o undistort = identity to 1e-12 px on the coefficient sets, zero coefficients return the
//      input's bits, a set that cannot converge returns RSBA_ERR_UNSUPPORTED: once through rad <= 0 and once with rad positive all the
//      way and fifty iterations that never meet the test.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ba_math.hpp"
#include "rsba.h"

namespace rsba { int DeviceCount() { return 0; } }   // (the kernels are not in this build)

namespace {

struct Dual3 {
  double a, v[3];
};
Dual3 operator+(const Dual3& f, const Dual3& g) { Dual3 r; r.a = f.a + g.a; for (int i = 0; i < 3; ++i) r.v[i] = f.v[i] + g.v[i]; return r; }
Dual3 operator*(const Dual3& f, const Dual3& g) { Dual3 r; r.a = f.a * g.a; for (int i = 0; i < 3; ++i) r.v[i] = f.a * g.v[i] + f.v[i] * g.a; return r; }
Dual3 Const(double x) { return Dual3{x, {0.0, 0.0, 0.0}}; }
Dual3 Var(double x, int k) { Dual3 r = Const(x); r.v[k] = 1.0; return r; }
Dual3 Recip(const Dual3& g) { Dual3 r; r.a = 1.0 / g.a; for (int i = 0; i < 3; ++i) r.v[i] = -g.v[i] * r.a * r.a; return r; }

int g_fail = 0;
void Expect(bool ok, const char* what, double got, double want) {
  if (!ok) { ++g_fail; if (g_fail < 20) printf("FAIL %s: got %.17g want %.17g\n", what, got, want); }
}

// the coefficient sets of tests/marker_distortion_ref.py::coefficients' ranges: extremes, tangential only, k3 only, zeros
const double kSets[][5] = {
    {0.0, 0.0, 0.0, 0.0, 0.0},
    {0.0, 0.0, 2e-3, -2e-3, 0.0},
    {0.0, 0.0, 0.0, 0.0, 0.05},
    {-0.30, 0.10, 2e-3, 2e-3, -0.05},
    {0.15, -0.10, -2e-3, 1e-3, 0.05},
    {-0.30, -0.10, -2e-3, -2e-3, -0.05},
    {-0.12, 0.03, 5e-4, -7e-4, 0.01},
};
const int kNumSets = sizeof(kSets) / sizeof(kSets[0]);

}  // namespace

int main() {
  const double fx = 612.5, fy = 608.25, ppx = 322.75, ppy = 236.5;
  int checked = 0;
  // 1, 2: over the image (normalised points up to the corners), three depths
  for (int s = 0; s < kNumSets; ++s) {
    const double* d = kSets[s];
    for (int iu = 0; iu <= 8; ++iu) {
      for (int iv = 0; iv <= 6; ++iv) {
        for (int iz = 0; iz < 3; ++iz) {
          const double Z = 0.4 + 0.9 * iz, x = (80.0 * iu - ppx) / fx, y = (80.0 * iv - ppy) / fy;
          const double X = x * Z, Y = y * Z, u = 300.0 + iu, v = 200.0 - iv;
          double r[2], Q[6];
          rsba::ProjectCorner<true>(X, Y, Z, fx, fy, ppx, ppy, d, u, v, r, Q);
          // the same projection on dual numbers: (X, Y, Z) -> (x, y) -> DistortNormalised -> pixels
          const Dual3 Xd = Var(X, 0), Yd = Var(Y, 1), Zd = Var(Z, 2), izd = Recip(Zd);
          Dual3 k[5], xd, yd;
          for (int q = 0; q < 5; ++q) k[q] = Const(d[q]);
          rsba::DistortNormalised(Xd * izd, Yd * izd, k, Const(1.0), Const(2.0), &xd, &yd);
          const Dual3 ud = Const(fx) * xd + Const(ppx), vd = Const(fy) * yd + Const(ppy);
          // values: a few ulps of a pixel coordinate (~1e3); derivatives: relative to the row's largest entry (~fx / Z)
          Expect(std::fabs(r[0] - (ud.a - u)) <= 2e-12, "r0", r[0], ud.a - u);
          Expect(std::fabs(r[1] - (vd.a - v)) <= 2e-12, "r1", r[1], vd.a - v);
          double big = 0.0;
          for (int q = 0; q < 3; ++q) big = std::fmax(big, std::fmax(std::fabs(ud.v[q]), std::fabs(vd.v[q])));
          for (int q = 0; q < 3; ++q) {
            Expect(std::fabs(Q[q] - ud.v[q]) <= 1e-13 * big, "Q row 0", Q[q], ud.v[q]);
            Expect(std::fabs(Q[3 + q] - vd.v[q]) <= 1e-13 * big, "Q row 1", Q[3 + q], vd.v[q]);
          }
          if (s == 0) {
            // zero coefficients: the pinhole form to rounding ...
            double rp[2], Qp[6];
            rsba::ProjectCorner<false>(X, Y, Z, fx, fy, ppx, ppy, nullptr, u, v, rp, Qp);
            for (int q = 0; q < 2; ++q) Expect(std::fabs(r[q] - rp[q]) <= 1e-12, "zero coefficients, r", r[q], rp[q]);
            for (int q = 0; q < 6; ++q) Expect(std::fabs(Q[q] - Qp[q]) <= 1e-13 * big, "zero coefficients, Q", Q[q], Qp[q]);
            // ... and the pinhole instance is the functors' expressions, bit for bit
            const double z1 = 1.0 / Z, al = fx * z1, be = fy * z1;
            const double want_r[2] = {fx * X * z1 + ppx - u, fy * Y * z1 + ppy - v};
            const double want_Q[6] = {al, 0.0, -al * X * z1, 0.0, be, -be * Y * z1};
            Expect(std::memcmp(rp, want_r, sizeof(want_r)) == 0, "pinhole bits, r", rp[0], want_r[0]);
            Expect(std::memcmp(Qp, want_Q, sizeof(want_Q)) == 0, "pinhole bits, Q", Qp[2], want_Q[2]);
            double a0, a1;
            rsba::ProjectCornerResidual<false>(X, Y, Z, fx, fy, ppx, ppy, nullptr, u, v, &a0, &a1);
            Expect(a0 == fx * X / Z + ppx - u && a1 == fy * Y / Z + ppy - v, "pinhole bits, residual-only", a0, fx * X / Z + ppx - u);
          }
          ++checked;
        }
      }
    }
  }
  // 2b: a whole corner through the chain: <true> with zeros against <false>, and Qt's middle-row term (a camera with tangential terms
  //     makes Q full: the time block of <true> must differ from what the pinhole carry would give)
  {
    const double cam6[6] = {0.11, -0.07, 0.05, 0.3, -0.2, 0.05}, tim6[6] = {0.2, 0.15, -0.3, 0.1, -0.05, 1.6}, mar6[6] = {0.02, -0.03, 0.04, 0.13, 0.0, 0.01};
    const double zero4[4] = {0, 0, 0, 0}, intr4[4] = {fx, fy, ppx, ppy};
    double cc[rsba::CC_STRIDE], ct[rsba::CC_STRIDE], cm[rsba::CC_STRIDE];
    rsba::CameraConstants(cam6, zero4, cc); rsba::CameraConstants(tim6, zero4, ct); rsba::CameraConstants(mar6, zero4, cm);
    double r0[2], J0[36], r1[2], J1[36];
    rsba::MarkerCornerResidualJacobian<false>(cc, ct, cm, intr4, -0.04, 0.04, 310.0, 250.0, r0, J0);
    rsba::MarkerCornerResidualJacobian<true>(cc, ct, cm, intr4, -0.04, 0.04, 310.0, 250.0, r1, J1, kSets[0]);
    double big = 0.0;
    for (int q = 0; q < 36; ++q) big = std::fmax(big, std::fabs(J0[q]));
    for (int q = 0; q < 2; ++q) Expect(std::fabs(r0[q] - r1[q]) <= 1e-12, "chain, zero coefficients, r", r1[q], r0[q]);
    for (int q = 0; q < 36; ++q) Expect(std::fabs(J0[q] - J1[q]) <= 1e-13 * big, "chain, zero coefficients, J", J1[q], J0[q]);
    // the written-out pinhole branches the product runs, against ProjectCorner<false> (bits): the camera block's translation columns
    // of a corner are Q itself, and the per-part twin repeats the rows
    {
      const double X[3] = {-0.04, 0.04, 0.0};
      double pm[3], pt[3], pc[3];
      auto apply = [](const double* c, const double* in, double* out) {
        for (int i = 0; i < 3; ++i) out[i] = c[rsba::CC_R + 3 * i] * in[0] + c[rsba::CC_R + 3 * i + 1] * in[1] + c[rsba::CC_R + 3 * i + 2] * in[2] + c[rsba::CC_T + i];
      };
      apply(cm, X, pm); apply(ct, pm, pt); apply(cc, pt, pc);
      double rq[2], Qq[6];
      rsba::ProjectCorner<false>(pc[0], pc[1], pc[2], fx, fy, ppx, ppy, nullptr, 310.0, 250.0, rq, Qq);
      Expect(rq[0] == r0[0] && rq[1] == r0[1], "written-out pinhole branch, r", r0[0], rq[0]);
      for (int i = 0; i < 2; ++i)
        for (int q = 0; q < 3; ++q) Expect(J0[18 * i + 3 + q] == Qq[3 * i + q], "written-out pinhole branch, Q", J0[18 * i + 3 + q], Qq[3 * i + q]);
      for (int part = 0; part < 3; ++part) {
        double rp[2] = {0, 0}, Jp[36];
        for (double& v : Jp) v = 0.0;
        rsba::MarkerCornerJacobianPart<false>(part, cc, ct, cm, fx, fy, ppx, ppy, -0.04, 0.04, 310.0, 250.0, rp, Jp);
        for (int i = 0; i < 2; ++i)
          for (int q = 0; q < 6; ++q) Expect(Jp[18 * i + 6 * part + q] == J0[18 * i + 6 * part + q], "per-part twin, pinhole", Jp[18 * i + 6 * part + q], J0[18 * i + 6 * part + q]);
        if (part == 0) Expect(rp[0] == r0[0] && rp[1] == r0[1], "per-part twin, pinhole, r", rp[0], r0[0]);
      }
    }
    for (int part = 0; part < 3; ++part) {
      double rp[2] = {0, 0}, Jp[36];
      for (double& v : Jp) v = 0.0;
      rsba::MarkerCornerJacobianPart<true>(part, cc, ct, cm, fx, fy, ppx, ppy, -0.04, 0.04, 310.0, 250.0, rp, Jp, kSets[3]);
      double rw[2], Jw[36];
      rsba::MarkerCornerResidualJacobian<true>(cc, ct, cm, intr4, -0.04, 0.04, 310.0, 250.0, rw, Jw, kSets[3]);
      for (int i = 0; i < 2; ++i)
        for (int q = 0; q < 6; ++q) Expect(Jp[18 * i + 6 * part + q] == Jw[18 * i + 6 * part + q], "per-part twin", Jp[18 * i + 6 * part + q], Jw[18 * i + 6 * part + q]);
      if (part == 0) Expect(rp[0] == rw[0] && rp[1] == rw[1], "per-part twin, r", rp[0], rw[0]);
    }
  }
  // 3: undistort.  Round trip over the image for every set, in pixels.
  double worst = 0.0;
  const double k4[4] = {fx, fy, ppx, ppy};
  for (int s = 0; s < kNumSets; ++s) {
    std::vector<double> ideal, dist_px;
    for (int iu = 0; iu <= 16; ++iu)
      for (int iv = 0; iv <= 12; ++iv) {
        const double x = (40.0 * iu - ppx) / fx, y = (40.0 * iv - ppy) / fy;
        double xd, yd;
        const double one = 1.0, two = 2.0;
        rsba::DistortNormalised(x, y, kSets[s], one, two, &xd, &yd);
        ideal.push_back(40.0 * iu); ideal.push_back(40.0 * iv);
        dist_px.push_back(fx * xd + ppx); dist_px.push_back(fy * yd + ppy);
      }
    std::vector<double> back(ideal.size(), -1.0);
    const int rc = rsba_undistort_points((int32_t)(ideal.size() / 2), dist_px.data(), k4, kSets[s], back.data());
    Expect(rc == RSBA_OK, "undistort return code", rc, RSBA_OK);
    for (size_t i = 0; i < ideal.size(); ++i) worst = std::fmax(worst, std::fabs(back[i] - ideal[i]));
    if (s == 0) Expect(std::memcmp(back.data(), dist_px.data(), back.size() * sizeof(double)) == 0, "zero coefficients: the input's bits", back[0], dist_px[0]);
  }
  Expect(worst <= 1e-12, "undistort round trip (px)", worst, 1e-12);
  {
    // in place, and a set the iteration cannot solve at this radius (rad(r2) reaches zero inside the image: no contraction)
    double p[4] = {10.0, 20.0, 600.0, 450.0};
    Expect(rsba_undistort_points(2, p, k4, kSets[4], p) == RSBA_OK, "in place", 0, 0);
    const double strong[5] = {-3.5, 0.0, 0.0, 0.0, 0.0};
    double q[2] = {5.0, 5.0}, out[2] = {-7.0, -7.0};
    Expect(rsba_undistort_points(1, q, k4, strong, out) == RSBA_ERR_UNSUPPORTED, "non-convergence code", 0, RSBA_ERR_UNSUPPORTED);
    // k1 = +2: rad = 1 + 2 r2 stays above one, but x -> xd / rad(x) is no contraction at these radii (the iterates alternate around the
    // solution): fifty iterations pass without an update below 1e-14
    const double wide[5] = {2.0, 0.0, 0.0, 0.0, 0.0};
    double qq[4] = {5.0, 5.0, 620.0, 460.0};
    for (int i = 0; i < 2; ++i) {
      double o2[2] = {-7.0, -7.0};
      Expect(rsba_undistort_points(1, qq + 2 * i, k4, wide, o2) == RSBA_ERR_UNSUPPORTED, "fifty iterations without convergence, rad > 0", 0, RSBA_ERR_UNSUPPORTED);
      Expect(o2[0] == -7.0 && o2[1] == -7.0, "a failed point leaves out as it was", o2[0], -7.0);
    }
    const double bad[5] = {NAN, 0, 0, 0, 0};
    Expect(rsba_undistort_points(1, q, k4, bad, out) == RSBA_ERR_ARG, "non-finite coefficient", 0, RSBA_ERR_ARG);
    Expect(rsba_undistort_points(0, nullptr, k4, kSets[1], nullptr) == RSBA_OK, "no points", 0, 0);
  }
  printf("distortion math driver: %d projections checked, undistort round trip worst %.3g px, %d failures\n", checked, worst, g_fail);
  if (g_fail == 0) printf("distortion math driver: ok\n");
  return g_fail == 0 ? 0 : 1;
}
