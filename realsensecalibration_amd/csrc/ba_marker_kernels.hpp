// Marker-chain model on the device (BASELINE config 1; the model Main_Calibration actually solves).
//
// Residual: 4 marker corners (-h,+h) (+h,+h) (+h,-h) (-h,-h) pushed through up to three rigid
// transforms marker -> base marker -> base camera -> target camera, then the pinhole projection
// (the four functors of /root/reference/Main_Calibration/bundle_adjustment.h:56-343 and their wiring in
// bundle_adjustment_manager.cpp:21-88; Test2 variant: Test2_BundleAdjustment/main.cpp:64-96).
// Derivatives are taken with forward-mode dual numbers on the GPU, i.e. the same arithmetic Ceres'
// AutoDiffCostFunction<.,8,6,6,6> performs, including the first-order branch of AngleAxisRotatePoint.
//
// The problem is tiny (68 residual blocks, 114 parameters on the committed data) and does not shard:
// one kernel evaluates the blocks (one thread each), one workgroup assembles the dense normal
// equations in a fixed order (bitwise reproducible), damps, factors (the same blocked Cholesky the
// reduced camera system uses) and forms the candidate; a third evaluates the candidate.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ba_marker_plan.hpp"
#include "ba_point_kernels.hpp"
#include "ba_problem.hpp"

namespace rsba {

template <int N>
struct DJet {
  double a;
  double v[N];
};
template <int N> __device__ __forceinline__ DJet<N> JConst(double x) { DJet<N> r; r.a = x; for (int i = 0; i < N; ++i) r.v[i] = 0.0; return r; }
template <int N> __device__ __forceinline__ DJet<N> JVar(double x, int k) { DJet<N> r = JConst<N>(x); r.v[k] = 1.0; return r; }
template <int N> __device__ __forceinline__ DJet<N> operator+(const DJet<N>& f, const DJet<N>& g) { DJet<N> r; r.a = f.a + g.a; for (int i = 0; i < N; ++i) r.v[i] = f.v[i] + g.v[i]; return r; }
template <int N> __device__ __forceinline__ DJet<N> operator-(const DJet<N>& f, const DJet<N>& g) { DJet<N> r; r.a = f.a - g.a; for (int i = 0; i < N; ++i) r.v[i] = f.v[i] - g.v[i]; return r; }
template <int N> __device__ __forceinline__ DJet<N> operator*(const DJet<N>& f, const DJet<N>& g) { DJet<N> r; r.a = f.a * g.a; for (int i = 0; i < N; ++i) r.v[i] = f.a * g.v[i] + f.v[i] * g.a; return r; }
template <int N> __device__ __forceinline__ DJet<N> operator/(const DJet<N>& f, const DJet<N>& g) {
  DJet<N> r; const double gi = 1.0 / g.a; const double fg = f.a * gi; r.a = fg;
  for (int i = 0; i < N; ++i) r.v[i] = (f.v[i] - fg * g.v[i]) * gi; return r; }
template <int N> __device__ __forceinline__ DJet<N> JSqrt(const DJet<N>& f) { DJet<N> r; const double t = sqrt(f.a); const double s = 1.0 / (2.0 * t); r.a = t; for (int i = 0; i < N; ++i) r.v[i] = f.v[i] * s; return r; }
template <int N> __device__ __forceinline__ DJet<N> JCos(const DJet<N>& f) { DJet<N> r; r.a = cos(f.a); const double s = -sin(f.a); for (int i = 0; i < N; ++i) r.v[i] = s * f.v[i]; return r; }
template <int N> __device__ __forceinline__ DJet<N> JSin(const DJet<N>& f) { DJet<N> r; r.a = sin(f.a); const double c = cos(f.a); for (int i = 0; i < N; ++i) r.v[i] = c * f.v[i]; return r; }
__device__ __forceinline__ double JConstD(double x) { return x; }

// Rotate p by the angle-axis w (in place), both branches; T = double or DJet<N>.
template <int N>
__device__ void RotateJet(const DJet<N> w[3], DJet<N> p[3]) {
  const DJet<N> t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  if (t2.a > DBL_EPSILON) {
    const DJet<N> th = JSqrt(t2), c = JCos(th), s = JSin(th), it = JConst<N>(1.0) / th;
    const DJet<N> k0 = w[0] * it, k1 = w[1] * it, k2 = w[2] * it;
    const DJet<N> x0 = k1 * p[2] - k2 * p[1], x1 = k2 * p[0] - k0 * p[2], x2 = k0 * p[1] - k1 * p[0];
    const DJet<N> tmp = (k0 * p[0] + k1 * p[1] + k2 * p[2]) * (JConst<N>(1.0) - c);
    const DJet<N> r0 = p[0] * c + x0 * s + k0 * tmp, r1 = p[1] * c + x1 * s + k1 * tmp, r2 = p[2] * c + x2 * s + k2 * tmp;
    p[0] = r0; p[1] = r1; p[2] = r2;
  } else {
    const DJet<N> r0 = p[0] + (w[1] * p[2] - w[2] * p[1]), r1 = p[1] + (w[2] * p[0] - w[0] * p[2]), r2 = p[2] + (w[0] * p[1] - w[1] * p[0]);
    p[0] = r0; p[1] = r1; p[2] = r2;
  }
}
__device__ inline void RotateD(const double w[3], double p[3]) {
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double r0, r1, r2;
  if (t2 > DBL_EPSILON) {
    const double th = sqrt(t2), c = cos(th), s = sin(th), it = 1.0 / th;
    const double k0 = w[0] * it, k1 = w[1] * it, k2 = w[2] * it;
    const double x0 = k1 * p[2] - k2 * p[1], x1 = k2 * p[0] - k0 * p[2], x2 = k0 * p[1] - k1 * p[0];
    const double tmp = (k0 * p[0] + k1 * p[1] + k2 * p[2]) * (1.0 - c);
    r0 = p[0] * c + x0 * s + k0 * tmp; r1 = p[1] * c + x1 * s + k1 * tmp; r2 = p[2] * c + x2 * s + k2 * tmp;
  } else {
    r0 = p[0] + (w[1] * p[2] - w[2] * p[1]); r1 = p[1] + (w[2] * p[0] - w[0] * p[2]); r2 = p[2] + (w[0] * p[1] - w[1] * p[0]);
  }
  p[0] = r0; p[1] = r1; p[2] = r2;
}

// (MarkerObs, the per-observation wiring: ba_marker_plan.hpp)
#define RSBA_SUBSET_BIT (1 << 30)        // act_to_full: the active column is a constant component of a partly constant block

// A partly constant block (rsba_problem_set_parameter_subset_constant): the columns of its constant components leave the stored rows
// as exact zeros — what seeding the component as a constant in the dual-number pass gives — after k_marker_eval (and its corrector's
// scaling) wrote them.  Thread per entry of the N x 8 x 18 rows.
__global__ void __launch_bounds__(256) k_marker_subset_rows(int N, const MarkerObs* __restrict__ mo, double* __restrict__ Jbuf) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)N * 144) return;
  const int i = (int)(e / 144), q = (int)(e - (size_t)i * 144) % 18;
  if ((mo[i].pad >> q) & 1) Jbuf[e] = 0.0;
}

// Evaluate residual blocks.  with_jacobian: J (8 x 18, columns camera|time|marker) and r (8) are stored.
// kLoss: the residual block (one observation, 8 residuals) is robustified as Ceres' corrector does it for rho'' <= 0 (Huber,
// Cauchy): s = |r|^2 over the 8 residuals, J and r stored scaled by sqrt(rho'(s)), rho(s) (the cost) into rho_per_obs;
// sumsq_per_obs keeps the raw s (the RMS metric).  loss: the signed parameter of LossAndScale (0: rho(s) = s).  wts: the blocks'
// weights a_i (ceres::ScaledLoss), the problem's order: the cost a_i rho(s), the rows scaled by sqrt(a_i rho'(s)) — formed as
// sqrt(a_i) sqrt(rho'), so a weight of one changes no bit and a weight of zero leaves exact zeros.
// kDist: dist = the cameras' five distortion coefficients [C][5], indexed as intr; the dual-number pass runs DistortNormalised
// (ba_math.hpp) on the normalised point, the value pass ProjectCorner's residuals.
template <bool kLoss, bool kDist = false>
__global__ void __launch_bounds__(64) k_marker_eval(int N, const MarkerObs* __restrict__ mo, const double* __restrict__ obs8,
                              const double* __restrict__ params, typename IntrArg<kDist>::type intr, double half_side,
                              int with_jacobian, double* __restrict__ Jbuf, double* __restrict__ rbuf,
                              double* __restrict__ sumsq_per_obs, double loss = 0.0, double* __restrict__ rho_per_obs = nullptr,
                              const double* __restrict__ wts = nullptr) {
  // Jacobian rows leave through LDS: a thread's 36 doubles per corner would otherwise be 64 scattered 288-byte pieces per
  // store instruction (1152 B between neighbouring lanes); staged, consecutive lanes write consecutive words
  __shared__ double stage[64 * 37];
  const int i0 = blockIdx.x * blockDim.x, i = i0 + threadIdx.x;
  const bool live = i < N;
  const int ii = live ? i : N - 1;   // lanes past the end keep going for the barriers, on the last block's data
  const MarkerObs o = mo[ii];
  const double fx = IntrOf(intr)[4 * o.camera], fy = IntrOf(intr)[4 * o.camera + 1], ppx = IntrOf(intr)[4 * o.camera + 2], ppy = IntrOf(intr)[4 * o.camera + 3];
  const double cx[4] = {-half_side, half_side, half_side, -half_side};
  const double cy[4] = {half_side, half_side, -half_side, -half_side};
  double ss = 0.0;
  if (!with_jacobian) {
    for (int k = 0; k < 4; ++k) {
      double p[3] = {cx[k], cy[k], 0.0};
      if (o.full_marker >= 0) { const double* m = params + o.full_marker; RotateD(m, p); p[0] += m[3]; p[1] += m[4]; p[2] += m[5]; }
      { const double* t = params + o.full_time; RotateD(t, p); p[0] += t[3]; p[1] += t[4]; p[2] += t[5]; }
      if (o.full_cam >= 0) { const double* c = params + o.full_cam; RotateD(c, p); p[0] += c[3]; p[1] += c[4]; p[2] += c[5]; }
      double r0, r1;
      ProjectCornerResidual<kDist>(p[0], p[1], p[2], fx, fy, ppx, ppy, DistOf(intr, o.camera),
                                   obs8[8 * (size_t)ii + 2 * k], obs8[8 * (size_t)ii + 2 * k + 1], &r0, &r1);
      ss += r0 * r0 + r1 * r1;
    }
  } else {
    typedef DJet<18> J;
    J cam[6], tim[6], mar[6];
    for (int q = 0; q < 6; ++q) {
      cam[q] = o.full_cam >= 0 ? JVar<18>(params[o.full_cam + q], q) : JConst<18>(0.0);
      tim[q] = JVar<18>(params[o.full_time + q], 6 + q);
      mar[q] = o.full_marker >= 0 ? JVar<18>(params[o.full_marker + q], 12 + q) : JConst<18>(0.0);
    }
    for (int k = 0; k < 4; ++k) {
      J p[3] = {JConst<18>(cx[k]), JConst<18>(cy[k]), JConst<18>(0.0)};
      if (o.full_marker >= 0) { RotateJet<18>(mar, p); p[0] = p[0] + mar[3]; p[1] = p[1] + mar[4]; p[2] = p[2] + mar[5]; }
      RotateJet<18>(tim, p); p[0] = p[0] + tim[3]; p[1] = p[1] + tim[4]; p[2] = p[2] + tim[5];
      if (o.full_cam >= 0) { RotateJet<18>(cam, p); p[0] = p[0] + cam[3]; p[1] = p[1] + cam[4]; p[2] = p[2] + cam[5]; }
      J xp, yp;
      if constexpr (kDist) {
        J kd[5], xd, yd;
        for (int q = 0; q < 5; ++q) kd[q] = JConst<18>(DistOf(intr, o.camera)[q]);
        DistortNormalised(p[0] / p[2], p[1] / p[2], kd, JConst<18>(1.0), JConst<18>(2.0), &xd, &yd);
        xp = JConst<18>(fx) * xd + JConst<18>(ppx);
        yp = JConst<18>(fy) * yd + JConst<18>(ppy);
      } else {
        xp = JConst<18>(fx) * p[0] / p[2] + JConst<18>(ppx);
        yp = JConst<18>(fy) * p[1] / p[2] + JConst<18>(ppy);
      }
      const double r0 = xp.a - obs8[8 * (size_t)ii + 2 * k], r1 = yp.a - obs8[8 * (size_t)ii + 2 * k + 1];
      if (live) { rbuf[8 * (size_t)i + 2 * k] = r0; rbuf[8 * (size_t)i + 2 * k + 1] = r1; }
      for (int q = 0; q < 18; ++q) { stage[threadIdx.x * 37 + q] = xp.v[q]; stage[threadIdx.x * 37 + 18 + q] = yp.v[q]; }
      __syncthreads();
      {
        const int nlive = min(64, N - i0);
        for (int e = threadIdx.x; e < nlive * 36; e += 64) { const int t = e / 36, q = e - 36 * t; Jbuf[(size_t)(i0 + t) * 144 + 36 * k + q] = stage[t * 37 + q]; }
      }
      __syncthreads();
      ss += r0 * r0 + r1 * r1;
    }
    if constexpr (kLoss) {
      // s is known only after the fourth corner: the block's stored rows are scaled in place (its r by the thread that wrote
      // them; its J through the same coalesced walk that stored it, sqrt(rho') handed over in the staging row's unused word).
      // Scaling before the store would need s first, i.e. a value pass over the corners ahead of the dual-number one; the
      // re-read of the block's 1152 bytes is the cheaper of the two on this one-workgroup-system path.
      double sq;
      const double a = wts[ii];
      const double rho = a * LossAndScale(loss, ss, &sq);
      sq *= sqrt(a);
      if (live) {
        rho_per_obs[i] = rho;
        for (int e = 0; e < 8; ++e) rbuf[8 * (size_t)i + e] *= sq;
      }
      stage[threadIdx.x * 37 + 36] = sq;
      __threadfence_block();
      __syncthreads();
      const int nlive = min(64, N - i0);
      for (int e = threadIdx.x; e < nlive * 144; e += 64) Jbuf[(size_t)i0 * 144 + e] *= stage[(e / 144) * 37 + 36];
    }
  }
  if constexpr (kLoss) {
    if (!with_jacobian && live) { double sq; rho_per_obs[i] = wts[i] * LossAndScale(loss, ss, &sq); }
  }
  if (live) sumsq_per_obs[i] = ss;
}

// One workgroup: normal equations in a fixed order, Jacobi scale, LM damping, Cholesky, step, candidate.
//   A : (n+1) x n work matrix; H/g accumulated by thread-per-entry loops over the observations in order.
// kSub: some active column is a constant component (RSBA_SUBSET_BIT in act_to_full; its rows' entries are exact zeros,
// k_marker_subset_rows): it gets a unit diagonal before the Jacobi scale is taken — row, column and gradient are zero, so it is
// decoupled from the free columns whatever the damping options are, and its step is an exact zero.  It stays in |x| (Ceres' norms
// are those of the ambient vector).
template <int kThreads, bool kSub = false>
__global__ void __launch_bounds__(kThreads)
k_marker_system(int N, int n, const MarkerObs* __restrict__ mo, const double* __restrict__ Jbuf, const double* __restrict__ rbuf,
                const double* __restrict__ sumsq_per_obs, double* __restrict__ A, double* __restrict__ scale,
                double* __restrict__ grad, const int* __restrict__ act_to_full, const double* __restrict__ params_x,
                double* __restrict__ params_c, double* __restrict__ delta_act, double* __restrict__ res, IterParams ip) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  __shared__ int s_ok;
  // per-observation column map: active offset of each of the 18 local columns (or -1)
  auto col_of = [&](const MarkerObs& o, int q) { const int b = q / 6; const int base = b == 0 ? o.act_cam : (b == 1 ? o.act_time : o.act_marker); return base < 0 ? -1 : base + (q - 6 * b); };
  // H (unscaled) lower+upper, and g: each thread owns entries and walks the observations in order
  for (size_t e = tid; e < (size_t)n * n; e += nt) A[e] = 0.0;
  for (int i = tid; i < n; i += nt) { A[(size_t)n * n + i] = 0.0; }
  __syncthreads();
  for (int ob = 0; ob < N; ++ob) {
    const MarkerObs o = mo[ob];
    // 18 x 18 local block, 324 entries over the threads
    for (int e = tid; e < 324; e += nt) {
      const int a = e / 18, b = e - 18 * a;
      const int ca = col_of(o, a), cb = col_of(o, b);
      if (ca < 0 || cb < 0) continue;
      double s = 0.0;
      for (int r = 0; r < 8; ++r) s += Jbuf[(size_t)(8 * ob + r) * 18 + a] * Jbuf[(size_t)(8 * ob + r) * 18 + b];
      A[(size_t)ca * n + cb] += s;
    }
    for (int a = tid; a < 18; a += nt) {
      const int ca = col_of(o, a);
      if (ca < 0) continue;
      double s = 0.0;
      for (int r = 0; r < 8; ++r) s += Jbuf[(size_t)(8 * ob + r) * 18 + a] * rbuf[8 * (size_t)ob + r];
      A[(size_t)n * n + ca] += s;
    }
    __threadfence_block();
    __syncthreads();
  }
  if constexpr (kSub) {
    for (int i = tid; i < n; i += nt) if (act_to_full[i] & RSBA_SUBSET_BIT) A[(size_t)i * n + i] = 1.0;
    __threadfence_block();
    __syncthreads();
  }
  // gradient (unscaled), scale (iteration 0), damping
  for (int i = tid; i < n; i += nt) {
    grad[i] = A[(size_t)n * n + i];
    if (ip.first) scale[i] = ip.jacobi_scaling ? 1.0 / (1.0 + sqrt(A[(size_t)i * n + i])) : 1.0;
  }
  __threadfence_block();
  __syncthreads();
  for (size_t e = tid; e < (size_t)n * n; e += nt) {
    const int i = (int)(e / n), j = (int)(e - (size_t)i * n);
    double v = A[e] * (scale[i] * scale[j]);
    if (i == j) v += fmin(fmax(v, ip.min_lm_diagonal), ip.max_lm_diagonal) / ip.radius;
    A[e] = v;
  }
  for (int i = tid; i < n; i += nt) A[(size_t)n * n + i] *= scale[i];
  __threadfence_block();
  __syncthreads();
  double* ysol = A + (size_t)n * n;
  if (kThreads == 512) CholeskySolvePanelLDS(n, A, ysol, &s_ok, lds, PanelSource{nullptr, nullptr, nullptr, 0.0, 0.0, 0.0, nullptr, nullptr, 0});
  else CholeskySolveBlocked<kSub ? 1 : 0>(n, A, ysol, &s_ok, lds);
  __syncthreads();
  // step, candidate, norms, cost at x
  double* scr = lds;
  double d2 = 0, x2 = 0, xc2 = 0, gm = 0;
  for (int i = tid; i < n; i += nt) {
    const double d = -scale[i] * ysol[i];
    delta_act[i] = d;
    const int fi = kSub ? act_to_full[i] & ~RSBA_SUBSET_BIT : act_to_full[i];
    const double x = params_x[fi], xc = x + d;
    params_c[fi] = xc;
    d2 += d * d; x2 += x * x; xc2 += xc * xc; gm = fmax(gm, fabs(grad[i]));
  }
  double cs = 0;
  for (int i = tid; i < N; i += nt) cs += sumsq_per_obs[i];
  scr[tid] = d2; scr[nt + tid] = x2; scr[2 * nt + tid] = xc2; scr[3 * nt + tid] = gm; scr[4 * nt + tid] = cs;
  __syncthreads();
  for (int off = nt / 2; off > 0; off >>= 1) {
    if (tid < off) {
      scr[tid] += scr[tid + off]; scr[nt + tid] += scr[nt + tid + off]; scr[2 * nt + tid] += scr[2 * nt + tid + off];
      scr[3 * nt + tid] = fmax(scr[3 * nt + tid], scr[3 * nt + tid + off]); scr[4 * nt + tid] += scr[4 * nt + tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    res[RES_COST_X] = 0.5 * scr[4 * nt]; res[RES_GMAX] = scr[3 * nt]; res[RES_XNORM2] = scr[nt];
    res[RES_CHOL_OK] = s_ok ? 1.0 : 0.0; res[RES_STEP2] = scr[0]; res[RES_XCNORM2] = scr[2 * nt]; res[RES_POINT_FAIL] = 0.0;
  }
}

// Model cost change -(J d).(r + J d / 2) and candidate cost, one workgroup, fixed order.  kLoss: J and r are the corrected ones
// (k_marker_eval<true>), the cost is 1/2 sum rho(s_c) (rho_c) and the raw sum of squares stays the RMS metric's.
template <bool kLoss>
__global__ void __launch_bounds__(256)
k_marker_candidate(int N, const MarkerObs* __restrict__ mo, const double* __restrict__ Jbuf, const double* __restrict__ rbuf,
                   const double* __restrict__ delta_act, const double* __restrict__ sumsq_c, double* __restrict__ res,
                   const double* __restrict__ rho_c = nullptr) {
  __shared__ double s[kLoss ? 3 : 2][256];
  const int tid = threadIdx.x;
  double mcc = 0, cc = 0, rc = 0;
  for (int i = tid; i < N; i += blockDim.x) {
    const MarkerObs o = mo[i];
    for (int r = 0; r < 8; ++r) {
      double mr = 0.0;
      for (int q = 0; q < 18; ++q) {
        const int b = q / 6; const int base = b == 0 ? o.act_cam : (b == 1 ? o.act_time : o.act_marker);
        if (base >= 0) mr += Jbuf[(size_t)(8 * i + r) * 18 + q] * delta_act[base + (q - 6 * b)];
      }
      mcc -= mr * (rbuf[8 * (size_t)i + r] + 0.5 * mr);
    }
    cc += sumsq_c[i];
    if constexpr (kLoss) rc += rho_c[i];
  }
  s[0][tid] = mcc; s[1][tid] = cc;
  if constexpr (kLoss) s[2][tid] = rc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) { s[0][tid] += s[0][tid + off]; s[1][tid] += s[1][tid + off]; if constexpr (kLoss) s[2][tid] += s[2][tid + off]; }
    __syncthreads();
  }
  if (tid == 0) {
    res[RES_MCC] = s[0][0];
    double c = 0.5 * s[kLoss ? 2 : 1][0];
    if (!(c == c) || !(fabs(c) <= DBL_MAX)) c = DBL_MAX;
    res[RES_COST_C] = c; res[RES_SUMSQ_C] = s[1][0];
  }
}

class KernelTimer;

// Gaussian priors on camera and marker blocks (rsba_problem_set_block_prior, ceres::NormalPrior): the residual A (x - b) of a block, no
// loss.  The tables of a solver created with K priors, in ascending parameter offset; which blocks carry one is fixed at create, the
// values (ab) can be replaced (Set).
struct PriorDevice {
  int K = 0;
  int *full = nullptr;   // [K] the block's offset in the full parameter array
  int *col = nullptr;    // [K] its first column in the path's linear system (active / reduced), -1: constant as a whole
  int *mask = nullptr;   // [K] its constant components (bit q), 0 for a constant block
  double* ab = nullptr;  // [K][42] A row-major, then b
  std::vector<int> hfull, hcol;   // (the host's copies: the setter and the Jacobian's structure)
  void Free() { for (void* q : {(void*)full, (void*)col, (void*)mask, (void*)ab}) if (q) (void)hipFree(q); full = col = mask = nullptr; ab = nullptr; K = 0; }
  // cols: per prior of the problem (the map's order = ascending offset) its first column
  int Upload(const rsba_problem& p, const std::vector<int>& cols) {
    K = (int)p.block_priors.size();
    hcol = cols;
    if (K == 0) return RSBA_OK;
    std::vector<int> hmask; std::vector<double> hab;
    hfull.clear();
    int k = 0;
    for (const auto& kv : p.block_priors) {
      hfull.push_back(6 * kv.first); hmask.push_back(cols[k] >= 0 ? p.subset_mask(kv.first) : 0);
      hab.insert(hab.end(), kv.second.begin(), kv.second.end()); ++k;
    }
    if (hipMalloc((void**)&full, K * 4) != hipSuccess || hipMalloc((void**)&col, K * 4) != hipSuccess || hipMalloc((void**)&mask, K * 4) != hipSuccess ||
        hipMalloc((void**)&ab, (size_t)K * 42 * 8) != hipSuccess) return RSBA_ERR_HIP;
    if (hipMemcpy(full, hfull.data(), K * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(col, cols.data(), K * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(mask, hmask.data(), K * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(ab, hab.data(), (size_t)K * 42 * 8, hipMemcpyHostToDevice) != hipSuccess)
      return RSBA_ERR_HIP;
    return RSBA_OK;
  }
  // new values for the prior of the block at `offset`: RSBA_ERR_UNSUPPORTED when the block had none at create
  int Set(int64_t offset, const double* A, const double* b) {
    if (offset < 0 || offset > INT32_MAX) return RSBA_ERR_UNSUPPORTED;
    const auto it = std::lower_bound(hfull.begin(), hfull.end(), (int)offset);
    if (it == hfull.end() || *it != offset) return RSBA_ERR_UNSUPPORTED;
    double v[42];
    memcpy(v, A, 36 * 8); memcpy(v + 36, b, 6 * 8);
    return hipMemcpy(ab + 42 * (size_t)(it - hfull.begin()), v, sizeof(v), hipMemcpyHostToDevice) == hipSuccess ? RSBA_OK : RSBA_ERR_HIP;
  }
};

// The priors as K pseudo residual blocks behind the N observations' (dense path): rows 0..5 of block N + k hold A in the column group
// of its block (camera: 0..5, marker: 12..17; exact zeros in the columns of constant components and everywhere else), rows 6..7 are
// zero, r = A (x - b).  rho gets |r|^2 (what k_marker_system / k_marker_candidate sum into the cost: a solver with priors runs the
// loss instances), the raw sum of squares 0.0: the reprojection metric never sees a prior.  with_rows = 0: the candidate, sums only.
// Thread per prior.
__global__ void __launch_bounds__(64) k_marker_prior_rows(int K, int N, const MarkerObs* __restrict__ mo, const int* __restrict__ mask,
                                                          const double* __restrict__ ab, const double* __restrict__ params, int with_rows,
                                                          double* __restrict__ Jbuf, double* __restrict__ rbuf, double* __restrict__ sumsq,
                                                          double* __restrict__ rho) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  const MarkerObs o = mo[N + k];
  const int g = o.full_cam >= 0 ? 0 : 12;
  const double* __restrict__ A = ab + 42 * (size_t)k;
  const double* __restrict__ x = params + (o.full_cam >= 0 ? o.full_cam : o.full_marker);
  double d[6], ss = 0.0;
  for (int q = 0; q < 6; ++q) d[q] = x[q] - A[36 + q];
  for (int i = 0; i < 8; ++i) {
    double r = 0.0;
    if (i < 6) for (int q = 0; q < 6; ++q) r += A[6 * i + q] * d[q];
    ss += r * r;
    if (with_rows) {
      rbuf[8 * (size_t)(N + k) + i] = r;
      double* __restrict__ row = Jbuf + ((size_t)(N + k) * 8 + i) * 18;
      for (int q = 0; q < 18; ++q) row[q] = 0.0;
      if (i < 6) for (int q = 0; q < 6; ++q) row[g + q] = ((mask[k] >> q) & 1) ? 0.0 : A[6 * i + q];
    }
  }
  sumsq[N + k] = 0.0;
  rho[N + k] = ss;
}

// ------------------------------------------------------------------------------------------------
// Free intrinsics (rsba_problem_set_intrinsics_free): a fourth block per residual, the detecting camera's six values
// fx fy cx cy k1 k2.  Kernels of their own: a solver without free intrinsics runs the instances above, untouched.
//   state:  the vectors params[2] / params0 continue behind the nfull pose values with six values per camera (every camera, free
//           or not), camera k at nfull + 6 k; p1 p2 k3 stay in dist [C][5] (zeros where the problem has no coefficients)
//   rows:   8 x 24 per residual block, columns camera | time | marker | intrinsics; the 18 pose columns by dual numbers as
//           k_marker_eval<., true> forms them, the six others analytic:
//             du / d (fx cx k1 k2) = xd, 1, fx x r2, fx x r2^2     dv / d (fy cy k1 k2) = yd, 1, fy y r2, fy y r2^2
//   icol:   [C] the first column of a camera's intrinsics block in the linear system, -1: the camera has none
//   pad:    bits 18..23 of MarkerObs::pad mark the held components of the block (all six where the camera has none)
// ------------------------------------------------------------------------------------------------
#define RSBA_INTR_MAX_COLUMNS 8192   // active columns of the dense system above which a solver with free intrinsics is refused

// the constant columns of the stored 8 x 24 rows as exact zeros (k_marker_subset_rows at this width).  Thread per entry.
__global__ void __launch_bounds__(256) k_marker_intr_subset_rows(int N, const MarkerObs* __restrict__ mo, double* __restrict__ Jbuf) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)N * 192) return;
  const int i = (int)(e / 192), q = (int)(e - (size_t)i * 192) % 24;
  if ((mo[i].pad >> q) & 1) Jbuf[e] = 0.0;
}

// Always with the corrector and the weights (k_marker_eval<true, true>): loss = 0 and weights of one change no bit, so a solver
// without either passes those.
__global__ void __launch_bounds__(64) k_marker_intr_eval(int N, const MarkerObs* __restrict__ mo, const double* __restrict__ obs8,
                              const double* __restrict__ params, int nfull, const double* __restrict__ dist, double half_side,
                              int with_jacobian, double* __restrict__ Jbuf, double* __restrict__ rbuf,
                              double* __restrict__ sumsq_per_obs, double loss, double* __restrict__ rho_per_obs,
                              const double* __restrict__ wts) {
  __shared__ double stage[64 * 49];   // (k_marker_eval's staging, 48 doubles per corner and the corrector's word)
  const int i0 = blockIdx.x * blockDim.x, i = i0 + threadIdx.x;
  const bool live = i < N;
  const int ii = live ? i : N - 1;
  const MarkerObs o = mo[ii];
  const double* __restrict__ sv = params + nfull + 6 * (size_t)o.camera;
  const double fx = sv[0], fy = sv[1], ppx = sv[2], ppy = sv[3];
  const double kd5[5] = {sv[4], sv[5], dist[5 * o.camera + 2], dist[5 * o.camera + 3], dist[5 * o.camera + 4]};
  const double cx[4] = {-half_side, half_side, half_side, -half_side};
  const double cy[4] = {half_side, half_side, -half_side, -half_side};
  double ss = 0.0;
  if (!with_jacobian) {
    for (int k = 0; k < 4; ++k) {
      double p[3] = {cx[k], cy[k], 0.0};
      if (o.full_marker >= 0) { const double* m = params + o.full_marker; RotateD(m, p); p[0] += m[3]; p[1] += m[4]; p[2] += m[5]; }
      { const double* t = params + o.full_time; RotateD(t, p); p[0] += t[3]; p[1] += t[4]; p[2] += t[5]; }
      if (o.full_cam >= 0) { const double* c = params + o.full_cam; RotateD(c, p); p[0] += c[3]; p[1] += c[4]; p[2] += c[5]; }
      double r0, r1;
      ProjectCornerResidual<true>(p[0], p[1], p[2], fx, fy, ppx, ppy, kd5, obs8[8 * (size_t)ii + 2 * k], obs8[8 * (size_t)ii + 2 * k + 1], &r0, &r1);
      ss += r0 * r0 + r1 * r1;
    }
  } else {
    typedef DJet<18> J;
    J cam[6], tim[6], mar[6];
    for (int q = 0; q < 6; ++q) {
      cam[q] = o.full_cam >= 0 ? JVar<18>(params[o.full_cam + q], q) : JConst<18>(0.0);
      tim[q] = JVar<18>(params[o.full_time + q], 6 + q);
      mar[q] = o.full_marker >= 0 ? JVar<18>(params[o.full_marker + q], 12 + q) : JConst<18>(0.0);
    }
    for (int k = 0; k < 4; ++k) {
      J p[3] = {JConst<18>(cx[k]), JConst<18>(cy[k]), JConst<18>(0.0)};
      if (o.full_marker >= 0) { RotateJet<18>(mar, p); p[0] = p[0] + mar[3]; p[1] = p[1] + mar[4]; p[2] = p[2] + mar[5]; }
      RotateJet<18>(tim, p); p[0] = p[0] + tim[3]; p[1] = p[1] + tim[4]; p[2] = p[2] + tim[5];
      if (o.full_cam >= 0) { RotateJet<18>(cam, p); p[0] = p[0] + cam[3]; p[1] = p[1] + cam[4]; p[2] = p[2] + cam[5]; }
      J kd[5], xd, yd;
      for (int q = 0; q < 5; ++q) kd[q] = JConst<18>(kd5[q]);
      const J xn = p[0] / p[2], yn = p[1] / p[2];
      DistortNormalised(xn, yn, kd, JConst<18>(1.0), JConst<18>(2.0), &xd, &yd);
      const J xp = JConst<18>(fx) * xd + JConst<18>(ppx);
      const J yp = JConst<18>(fy) * yd + JConst<18>(ppy);
      const double r0 = xp.a - obs8[8 * (size_t)ii + 2 * k], r1 = yp.a - obs8[8 * (size_t)ii + 2 * k + 1];
      if (live) { rbuf[8 * (size_t)i + 2 * k] = r0; rbuf[8 * (size_t)i + 2 * k + 1] = r1; }
      double* __restrict__ su = stage + threadIdx.x * 49;
      double* __restrict__ sw = su + 24;
      for (int q = 0; q < 18; ++q) { su[q] = xp.v[q]; sw[q] = yp.v[q]; }
      {
        // the intrinsics columns: the projection is linear in each of the six
        const double r2 = xn.a * xn.a + yn.a * yn.a;
        const double gx = fx * xn.a * r2, gy = fy * yn.a * r2;
        su[18] = xd.a; su[19] = 0.0; su[20] = 1.0; su[21] = 0.0; su[22] = gx; su[23] = gx * r2;
        sw[18] = 0.0; sw[19] = yd.a; sw[20] = 0.0; sw[21] = 1.0; sw[22] = gy; sw[23] = gy * r2;
      }
      __syncthreads();
      {
        const int nlive = min(64, N - i0);
        for (int e = threadIdx.x; e < nlive * 48; e += 64) { const int t = e / 48, q = e - 48 * t; Jbuf[(size_t)(i0 + t) * 192 + 48 * k + q] = stage[t * 49 + q]; }
      }
      __syncthreads();
      ss += r0 * r0 + r1 * r1;
    }
    {
      // (k_marker_eval's corrector and weight, over all 24 columns)
      double sq;
      const double a = wts[ii];
      const double rho = a * LossAndScale(loss, ss, &sq);
      sq *= sqrt(a);
      if (live) {
        rho_per_obs[i] = rho;
        for (int e = 0; e < 8; ++e) rbuf[8 * (size_t)i + e] *= sq;
      }
      stage[threadIdx.x * 49 + 48] = sq;
      __threadfence_block();
      __syncthreads();
      const int nlive = min(64, N - i0);
      for (int e = threadIdx.x; e < nlive * 192; e += 64) Jbuf[(size_t)i0 * 192 + e] *= stage[(e / 192) * 49 + 48];
    }
  }
  if (!with_jacobian && live) { double sq; rho_per_obs[i] = wts[i] * LossAndScale(loss, ss, &sq); }
  if (live) sumsq_per_obs[i] = ss;
}

// the first column of local column q (0..23) of residual block ob; blocks N.. are the priors' pseudo-blocks: no intrinsics columns
__device__ __forceinline__ int MarkerIntrColumn(const MarkerObs& o, int q, int ob, int N, const int* __restrict__ icol) {
  const int b = q / 6;
  const int base = b == 0 ? o.act_cam : (b == 1 ? o.act_time : (b == 2 ? o.act_marker : (ob < N ? icol[o.camera] : -1)));
  return base < 0 ? -1 : base + (q - 6 * b);
}

// k_marker_system<., true> over the 24 columns.  N: the observations, NK: with the priors' pseudo-blocks behind them.
template <int kThreads>
__global__ void __launch_bounds__(kThreads)
k_marker_intr_system(int N, int NK, int n, const MarkerObs* __restrict__ mo, const int* __restrict__ icol, const double* __restrict__ Jbuf,
                     const double* __restrict__ rbuf, const double* __restrict__ sumsq_per_obs, double* __restrict__ A,
                     double* __restrict__ scale, double* __restrict__ grad, const int* __restrict__ act_to_full,
                     const double* __restrict__ params_x, double* __restrict__ params_c, double* __restrict__ delta_act,
                     double* __restrict__ res, IterParams ip) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  __shared__ int s_ok;
  for (size_t e = tid; e < (size_t)n * n; e += nt) A[e] = 0.0;
  for (int i = tid; i < n; i += nt) { A[(size_t)n * n + i] = 0.0; }
  __syncthreads();
  for (int ob = 0; ob < NK; ++ob) {
    const MarkerObs o = mo[ob];
    // 24 x 24 local block, 576 entries over the threads
    for (int e = tid; e < 576; e += nt) {
      const int a = e / 24, b = e - 24 * a;
      const int ca = MarkerIntrColumn(o, a, ob, N, icol), cb = MarkerIntrColumn(o, b, ob, N, icol);
      if (ca < 0 || cb < 0) continue;
      double s = 0.0;
      for (int r = 0; r < 8; ++r) s += Jbuf[(size_t)(8 * ob + r) * 24 + a] * Jbuf[(size_t)(8 * ob + r) * 24 + b];
      A[(size_t)ca * n + cb] += s;
    }
    for (int a = tid; a < 24; a += nt) {
      const int ca = MarkerIntrColumn(o, a, ob, N, icol);
      if (ca < 0) continue;
      double s = 0.0;
      for (int r = 0; r < 8; ++r) s += Jbuf[(size_t)(8 * ob + r) * 24 + a] * rbuf[8 * (size_t)ob + r];
      A[(size_t)n * n + ca] += s;
    }
    __threadfence_block();
    __syncthreads();
  }
  for (int i = tid; i < n; i += nt) if (act_to_full[i] & RSBA_SUBSET_BIT) A[(size_t)i * n + i] = 1.0;
  __threadfence_block();
  __syncthreads();
  for (int i = tid; i < n; i += nt) {
    grad[i] = A[(size_t)n * n + i];
    if (ip.first) scale[i] = ip.jacobi_scaling ? 1.0 / (1.0 + sqrt(A[(size_t)i * n + i])) : 1.0;
  }
  __threadfence_block();
  __syncthreads();
  for (size_t e = tid; e < (size_t)n * n; e += nt) {
    const int i = (int)(e / n), j = (int)(e - (size_t)i * n);
    double v = A[e] * (scale[i] * scale[j]);
    if (i == j) v += fmin(fmax(v, ip.min_lm_diagonal), ip.max_lm_diagonal) / ip.radius;
    A[e] = v;
  }
  for (int i = tid; i < n; i += nt) A[(size_t)n * n + i] *= scale[i];
  __threadfence_block();
  __syncthreads();
  double* ysol = A + (size_t)n * n;
  if (kThreads == 512) CholeskySolvePanelLDS(n, A, ysol, &s_ok, lds, PanelSource{nullptr, nullptr, nullptr, 0.0, 0.0, 0.0, nullptr, nullptr, 0});
  else CholeskySolveBlocked<2>(n, A, ysol, &s_ok, lds);   // (a copy of its own: see CholeskySolveBlocked)
  __syncthreads();
  double* scr = lds;
  double d2 = 0, x2 = 0, xc2 = 0, gm = 0;
  for (int i = tid; i < n; i += nt) {
    const double d = -scale[i] * ysol[i];
    delta_act[i] = d;
    const int fi = act_to_full[i] & ~RSBA_SUBSET_BIT;
    const double x = params_x[fi], xc = x + d;
    params_c[fi] = xc;
    d2 += d * d; x2 += x * x; xc2 += xc * xc; gm = fmax(gm, fabs(grad[i]));
  }
  double cs = 0;
  for (int i = tid; i < NK; i += nt) cs += sumsq_per_obs[i];
  scr[tid] = d2; scr[nt + tid] = x2; scr[2 * nt + tid] = xc2; scr[3 * nt + tid] = gm; scr[4 * nt + tid] = cs;
  __syncthreads();
  for (int off = nt / 2; off > 0; off >>= 1) {
    if (tid < off) {
      scr[tid] += scr[tid + off]; scr[nt + tid] += scr[nt + tid + off]; scr[2 * nt + tid] += scr[2 * nt + tid + off];
      scr[3 * nt + tid] = fmax(scr[3 * nt + tid], scr[3 * nt + tid + off]); scr[4 * nt + tid] += scr[4 * nt + tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    res[RES_COST_X] = 0.5 * scr[4 * nt]; res[RES_GMAX] = scr[3 * nt]; res[RES_XNORM2] = scr[nt];
    res[RES_CHOL_OK] = s_ok ? 1.0 : 0.0; res[RES_STEP2] = scr[0]; res[RES_XCNORM2] = scr[2 * nt]; res[RES_POINT_FAIL] = 0.0;
  }
}

// k_marker_candidate<true> over the 24 columns
__global__ void __launch_bounds__(256)
k_marker_intr_candidate(int N, int NK, const MarkerObs* __restrict__ mo, const int* __restrict__ icol, const double* __restrict__ Jbuf,
                        const double* __restrict__ rbuf, const double* __restrict__ delta_act, const double* __restrict__ sumsq_c,
                        double* __restrict__ res, const double* __restrict__ rho_c) {
  __shared__ double s[3][256];
  const int tid = threadIdx.x;
  double mcc = 0, cc = 0, rc = 0;
  for (int i = tid; i < NK; i += blockDim.x) {
    const MarkerObs o = mo[i];
    int col[24];
    for (int q = 0; q < 24; ++q) col[q] = MarkerIntrColumn(o, q, i, N, icol);
    for (int r = 0; r < 8; ++r) {
      double mr = 0.0;
      for (int q = 0; q < 24; ++q) if (col[q] >= 0) mr += Jbuf[(size_t)(8 * i + r) * 24 + q] * delta_act[col[q]];
      mcc -= mr * (rbuf[8 * (size_t)i + r] + 0.5 * mr);
    }
    cc += sumsq_c[i];
    rc += rho_c[i];
  }
  s[0][tid] = mcc; s[1][tid] = cc;
  s[2][tid] = rc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) { s[0][tid] += s[0][tid + off]; s[1][tid] += s[1][tid + off]; s[2][tid] += s[2][tid + off]; }
    __syncthreads();
  }
  if (tid == 0) {
    res[RES_MCC] = s[0][0];
    double c = 0.5 * s[2][0];
    if (!(c == c) || !(fabs(c) <= DBL_MAX)) c = DBL_MAX;
    res[RES_COST_C] = c; res[RES_SUMSQ_C] = s[1][0];
  }
}

// k_marker_prior_rows at 24 columns: the six intrinsics columns of a prior's pseudo-block are zeros
__global__ void __launch_bounds__(64) k_marker_intr_prior_rows(int K, int N, const MarkerObs* __restrict__ mo, const int* __restrict__ mask,
                                                               const double* __restrict__ ab, const double* __restrict__ params, int with_rows,
                                                               double* __restrict__ Jbuf, double* __restrict__ rbuf, double* __restrict__ sumsq,
                                                               double* __restrict__ rho) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  const MarkerObs o = mo[N + k];
  const int g = o.full_cam >= 0 ? 0 : 12;
  const double* __restrict__ A = ab + 42 * (size_t)k;
  const double* __restrict__ x = params + (o.full_cam >= 0 ? o.full_cam : o.full_marker);
  double d[6], ss = 0.0;
  for (int q = 0; q < 6; ++q) d[q] = x[q] - A[36 + q];
  for (int i = 0; i < 8; ++i) {
    double r = 0.0;
    if (i < 6) for (int q = 0; q < 6; ++q) r += A[6 * i + q] * d[q];
    ss += r * r;
    if (with_rows) {
      rbuf[8 * (size_t)(N + k) + i] = r;
      double* __restrict__ row = Jbuf + ((size_t)(N + k) * 8 + i) * 24;
      for (int q = 0; q < 24; ++q) row[q] = 0.0;
      if (i < 6) for (int q = 0; q < 6; ++q) row[g + q] = ((mask[k] >> q) & 1) ? 0.0 : A[6 * i + q];
    }
  }
  sumsq[N + k] = 0.0;
  rho[N + k] = ss;
}


struct MarkerDevice {
  int N = 0, n = 0, nfull = 0;
  double half_side = 0;
  MarkerObs* mo = nullptr;
  double *obs8 = nullptr, *intr = nullptr, *params[2] = {nullptr, nullptr}, *params0 = nullptr;
  double *Jbuf = nullptr, *rbuf = nullptr, *ss_x = nullptr, *ss_c = nullptr, *A = nullptr, *scale = nullptr, *grad = nullptr,
         *delta = nullptr, *res = nullptr;
  double *rho_x = nullptr, *rho_c = nullptr;   // rho(s) per residual block at x / at the candidate (a robust loss only)
  bool with_loss = false;   // the kLoss instances (Upload): a robust loss, or the problem carried observation weights
  double* wts = nullptr;    // [N] the blocks' weights, the problem's order (with_loss only; all ones when the problem had none)
  int* act_to_full = nullptr;
  int cur = 0;
  bool with_subset = false; // some block in the program has constant components (Upload): k_marker_subset_rows and k_marker_system<., true>
  bool with_dist = false;   // the kDist instances (Upload): some distortion coefficient of the problem is not zero
  double* dist = nullptr;   // [C][5], indexed as intr
  PriorDevice prior;        // K priors: K pseudo residual blocks behind the N observations' (k_marker_prior_rows); with_loss then
  // free intrinsics (rsba_problem_set_intrinsics_free): the k_marker_intr_* kernels, rows of 24 columns, with_loss always (ones for the
  // weights, loss 0 where the solver has neither) and dist always there (zeros where the problem has no coefficients)
  bool with_intr = false;
  int nstate = 0;           // doubles of params[2] / params0: nfull, with_intr: + 6 per camera (fx fy cx cy k1 k2)
  int* icol = nullptr;      // [C] first column of the camera's intrinsics block, -1: none (with_intr only)
  std::vector<int> intr_mask;   // [C] the masks this solver was created with (with_intr only)

  void Free() {
    prior.Free();
    void* ptrs[] = {mo, obs8, intr, params[0], params[1], params0, Jbuf, rbuf, ss_x, ss_c, A, scale, grad, delta, res, act_to_full, rho_x, rho_c, wts, dist, icol};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    mo = nullptr;
  }
  int Upload(const rsba_problem& p, bool loss = false) {
    with_loss = loss;
    N = (int)p.num_observations; nfull = (int)p.parameters.size(); half_side = p.marker_side / 2;
    const int nblocks = p.num_cameras + p.num_times + p.num_markers;
    std::vector<char> used(nblocks, 0);
    for (int i = 0; i < N; ++i) { if (p.uses_camera(i)) used[p.camera_block(i)] = 1; used[p.time_block(i)] = 1; if (p.uses_marker(i)) used[p.marker_block(i)] = 1; }
    // a constant block (rsba_problem_set_parameter_block_constant) keeps its transform in every residual that names it (full_*) and has no
    // columns (act_* = -1): it is not in the program, as Ceres has it
    for (int b = 0; b < nblocks && b < (int)p.block_constant.size(); ++b) if (p.block_constant[b]) used[b] = 0;
    std::vector<int> act(nblocks, -1), a2f;
    int na = 0;
    // constant components (block_subset) of a block in the program: the column stays, marked; a constant or unused block's mask is ignored
    with_subset = false;
    for (int b = 0; b < nblocks; ++b) if (used[b]) {
      act[b] = 6 * na++;
      const int mask = p.subset_mask(b);
      with_subset = with_subset || mask != 0;
      for (int q = 0; q < 6; ++q) a2f.push_back((6 * b + q) | (((mask >> q) & 1) ? RSBA_SUBSET_BIT : 0));
    }
    n = 6 * na;
    // free intrinsics: the blocks behind the pose columns, ascending camera index; a held component is a marked column, as a pose block's.
    // Refusals come before anything is allocated.
    const int C = p.num_cameras;
    with_intr = p.has_free_intrinsics();
    std::vector<int> hicol(C, -1);
    intr_mask.assign(with_intr ? C : 0, 0);
    if (with_intr) {
      std::vector<char> named(C, 0);
      for (int i = 0; i < N; ++i) named[p.camera_index[i]] = 1;
      for (int k = 0; k < C; ++k) {
        const int mask = p.intrinsics_free_mask(k);
        if (mask == 0) continue;
        if (!named[k]) return RSBA_ERR_UNSUPPORTED;   // (like a prior on a block no observation names)
        if (n + 6 > RSBA_INTR_MAX_COLUMNS) return RSBA_ERR_UNSUPPORTED;   // one workgroup factors the dense system
        intr_mask[k] = mask; hicol[k] = n; n += 6;
        for (int q = 0; q < 6; ++q) a2f.push_back((nfull + 6 * k + q) | (((mask >> q) & 1) ? 0 : RSBA_SUBSET_BIT));
      }
      if (n > RSBA_INTR_MAX_COLUMNS) return RSBA_ERR_UNSUPPORTED;
      with_loss = true;
    }
    nstate = nfull + (with_intr ? 6 * C : 0);
    const int ncols = with_intr ? 24 : 18;   // columns of a stored row
    const int K = (int)p.block_priors.size();
    std::vector<int> pcols;
    std::vector<MarkerObs> h(N + K);
    {
      int k = 0;
      for (const auto& kv : p.block_priors) {
        const int b = kv.first;
        MarkerObs& o = h[N + k++];
        o.full_cam = b < p.num_cameras ? 6 * b : -1; o.full_time = -1; o.full_marker = b < p.num_cameras ? -1 : 6 * b;
        o.act_cam = b < p.num_cameras ? act[b] : -1; o.act_time = -1; o.act_marker = b < p.num_cameras ? -1 : act[b];
        o.camera = 0; o.pad = 0;
        pcols.push_back(act[b]);
      }
    }
    const int NK = N + K;
    for (int i = 0; i < N; ++i) {
      MarkerObs& o = h[i];
      o.full_cam = p.uses_camera(i) ? 6 * p.camera_block(i) : -1; o.full_time = 6 * p.time_block(i);
      o.full_marker = p.uses_marker(i) ? 6 * p.marker_block(i) : -1;
      o.act_cam = p.uses_camera(i) ? act[p.camera_block(i)] : -1; o.act_time = act[p.time_block(i)];
      o.act_marker = p.uses_marker(i) ? act[p.marker_block(i)] : -1;
      o.camera = p.camera_index[i]; o.pad = 0;
      if (o.act_cam >= 0) o.pad |= p.subset_mask(p.camera_block(i));
      if (o.act_time >= 0) o.pad |= p.subset_mask(p.time_block(i)) << 6;
      if (o.act_marker >= 0) o.pad |= p.subset_mask(p.marker_block(i)) << 12;
      if (with_intr) o.pad |= (hicol[o.camera] >= 0 ? (~intr_mask[o.camera] & 63) : 63) << 18;
    }
    auto al = [](void** q, size_t bytes) { return hipMalloc(q, std::max<size_t>(bytes, 8)) == hipSuccess; };
    if (!al((void**)&mo, NK * sizeof(MarkerObs)) || !al((void**)&obs8, 8 * (size_t)N * 8) || !al((void**)&intr, p.intrinsics.size() * 8) ||
        !al((void**)&params[0], (size_t)nstate * 8) || !al((void**)&params[1], (size_t)nstate * 8) || !al((void**)&params0, (size_t)nstate * 8) ||
        !al((void**)&Jbuf, (size_t)NK * 8 * ncols * 8) || !al((void**)&rbuf, (size_t)NK * 8 * 8) || !al((void**)&ss_x, NK * 8) || !al((void**)&ss_c, NK * 8) ||
        !al((void**)&A, (size_t)(n + 2) * n * 8) || !al((void**)&scale, n * 8) || !al((void**)&grad, n * 8) || !al((void**)&delta, n * 8) ||
        !al((void**)&res, RES_SIZE * 8) || !al((void**)&act_to_full, n * sizeof(int)) || !al((void**)&rho_x, NK * 8) || !al((void**)&rho_c, NK * 8))
      return RSBA_ERR_HIP;
    if (hipMemcpy(mo, h.data(), NK * sizeof(MarkerObs), hipMemcpyHostToDevice) != hipSuccess) return RSBA_ERR_HIP;
    if (prior.Upload(p, pcols) != RSBA_OK) return RSBA_ERR_HIP;
    if (hipMemcpy(obs8, p.observations.data(), 8 * (size_t)N * 8, hipMemcpyHostToDevice) != hipSuccess) return RSBA_ERR_HIP;
    if (hipMemcpy(intr, p.intrinsics.data(), p.intrinsics.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return RSBA_ERR_HIP;
    if (hipMemcpy(params0, p.parameters.data(), nfull * 8, hipMemcpyHostToDevice) != hipSuccess) return RSBA_ERR_HIP;
    if (hipMemcpy(act_to_full, a2f.data(), n * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return RSBA_ERR_HIP;
    with_dist = p.has_distortion();
    if (with_intr) {
      // the state behind the poses, and the coefficients as an array that is always there
      std::vector<double> hs(6 * (size_t)C), hd(5 * (size_t)C, 0.0);
      if (!p.distortion.empty()) hd = p.distortion;
      for (int k = 0; k < C; ++k) {
        for (int q = 0; q < 4; ++q) hs[6 * (size_t)k + q] = p.intrinsics[4 * (size_t)k + q];
        hs[6 * (size_t)k + 4] = hd[5 * (size_t)k]; hs[6 * (size_t)k + 5] = hd[5 * (size_t)k + 1];
      }
      if (!al((void**)&icol, C * sizeof(int)) || !al((void**)&dist, hd.size() * 8) ||
          hipMemcpy(icol, hicol.data(), C * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(dist, hd.data(), hd.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(params0 + nfull, hs.data(), hs.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return RSBA_ERR_HIP;
    } else
    if (with_dist && (!al((void**)&dist, p.distortion.size() * 8) ||
                      hipMemcpy(dist, p.distortion.data(), p.distortion.size() * 8, hipMemcpyHostToDevice) != hipSuccess)) return RSBA_ERR_HIP;
    if (with_loss) {
      if (!al((void**)&wts, (size_t)N * 8)) return RSBA_ERR_HIP;
      const std::vector<double> ones(p.observation_weights.empty() ? (size_t)N : 0, 1.0);
      return SetWeights(p.observation_weights.empty() ? ones.data() : p.observation_weights.data());
    }
    return RSBA_OK;
  }
  // the blocks' weights, the problem's order (a solver that runs the kLoss instances)
  int SetWeights(const double* w) {
    return N == 0 || hipMemcpy(wts, w, (size_t)N * 8, hipMemcpyHostToDevice) == hipSuccess ? RSBA_OK : RSBA_ERR_HIP;
  }
  int Reset(hipStream_t st) {
    if (hipMemcpyAsync(params[0], params0, (size_t)nstate * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return RSBA_ERR_HIP;
    if (hipMemcpyAsync(params[1], params0, (size_t)nstate * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return RSBA_ERR_HIP;
    cur = 0;
    return RSBA_OK;
  }
  void Accept() { cur = 1 - cur; }
  template <typename Timer>
  int Step(hipStream_t st, const rsba_options& o, double radius, bool first, double* res_host, Timer& T) {
    IterParams ip;
    ip.radius = radius; ip.min_lm_diagonal = o.min_lm_diagonal; ip.max_lm_diagonal = o.max_lm_diagonal; ip.huber_delta = 0.0;
    ip.first = first ? 1 : 0; ip.jacobi_scaling = o.jacobi_scaling;
    // the robust loss, read as the point model reads it (signed: see LossAndScale); the instances without one are untouched
    // (Upload was told whether the kLoss instances run: a loss, or weights alone with loss = 0, rho(s) = s)
    const double loss = o.huber_delta > 0.0 ? (o.loss_type == RSBA_LOSS_CAUCHY ? -o.huber_delta : o.huber_delta) : 0.0;
    const int x = cur, c = 1 - cur;
    // the candidate array must carry the untouched blocks too
    if (hipMemcpyAsync(params[c], params[x], (size_t)nstate * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return RSBA_ERR_HIP;
    auto chk = [&](const char* what) {
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) { fprintf(stderr, "rsba: %s launch failed: %s\n", what, hipGetErrorString(e)); return false; }
      return true;
    };
    if (!chk("(before marker step)")) return RSBA_ERR_HIP;
    if (with_intr) return StepIntr(st, ip, loss, res_host, T);
    T.Begin("k_marker_eval", st);
    if (with_dist) {
      if (with_loss) k_marker_eval<true, true><<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[x], IntrDist{intr, dist}, half_side, 1, Jbuf, rbuf, ss_x, loss, rho_x, wts);
      else k_marker_eval<false, true><<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[x], IntrDist{intr, dist}, half_side, 1, Jbuf, rbuf, ss_x);
    } else if (with_loss) k_marker_eval<true><<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[x], intr, half_side, 1, Jbuf, rbuf, ss_x, loss, rho_x, wts);
    else k_marker_eval<false><<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[x], intr, half_side, 1, Jbuf, rbuf, ss_x);
    T.End(st);
    if (!chk("k_marker_eval")) return RSBA_ERR_HIP;
    if (with_subset) {
      T.Begin("k_marker_subset_rows", st);
      k_marker_subset_rows<<<(unsigned)(((size_t)N * 144 + 255) / 256), 256, 0, st>>>(N, mo, Jbuf);
      T.End(st);
    }
    const int NK = N + prior.K;   // the residual blocks k_marker_system and k_marker_candidate walk
    if (prior.K > 0) {
      T.Begin("k_marker_prior_rows", st);
      k_marker_prior_rows<<<(prior.K + 63) / 64, 64, 0, st>>>(prior.K, N, mo, prior.mask, prior.ab, params[x], 1, Jbuf, rbuf, ss_x, rho_x);
      T.End(st);
    }
    size_t lds = (size_t)std::max(2 * RSBA_TB * (RSBA_NB + 1) + RSBA_NB * (RSBA_NB + 1), 5 * 1024) * sizeof(double);
    if (n <= RSBA_CHOL_MAXN) lds = std::max(lds, CholeskyLdsDoubles(n) * sizeof(double));
    const double* cost_x = with_loss ? rho_x : ss_x;   // what k_marker_system sums into the cost at x
    T.Begin("k_marker_system", st);
    if (with_subset) {
      if (n <= RSBA_CHOL_MAXN) {
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k_marker_system<512, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        k_marker_system<512, true><<<1, 512, lds, st>>>(NK, n, mo, Jbuf, rbuf, cost_x, A, scale, grad, act_to_full, params[x], params[c], delta, res, ip);
      } else {
        k_marker_system<1024, true><<<1, 1024, lds, st>>>(NK, n, mo, Jbuf, rbuf, cost_x, A, scale, grad, act_to_full, params[x], params[c], delta, res, ip);
      }
    } else if (n <= RSBA_CHOL_MAXN) {
      if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k_marker_system<512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      k_marker_system<512><<<1, 512, lds, st>>>(NK, n, mo, Jbuf, rbuf, cost_x, A, scale, grad, act_to_full, params[x], params[c], delta, res, ip);
    } else {
      k_marker_system<1024><<<1, 1024, lds, st>>>(NK, n, mo, Jbuf, rbuf, cost_x, A, scale, grad, act_to_full, params[x], params[c], delta, res, ip);
    }
    T.End(st);
    if (!chk("k_marker_system")) return RSBA_ERR_HIP;
    T.Begin("k_marker_eval", st);
    if (with_dist) {
      if (with_loss) k_marker_eval<true, true><<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[c], IntrDist{intr, dist}, half_side, 0, nullptr, nullptr, ss_c, loss, rho_c, wts);
      else k_marker_eval<false, true><<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[c], IntrDist{intr, dist}, half_side, 0, nullptr, nullptr, ss_c);
    } else if (with_loss) k_marker_eval<true><<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[c], intr, half_side, 0, nullptr, nullptr, ss_c, loss, rho_c, wts);
    else k_marker_eval<false><<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[c], intr, half_side, 0, nullptr, nullptr, ss_c);
    T.End(st);
    if (prior.K > 0) {
      T.Begin("k_marker_prior_rows", st);
      k_marker_prior_rows<<<(prior.K + 63) / 64, 64, 0, st>>>(prior.K, N, mo, prior.mask, prior.ab, params[c], 0, nullptr, nullptr, ss_c, rho_c);
      T.End(st);
    }
    T.Begin("k_marker_candidate", st);
    if (with_loss) k_marker_candidate<true><<<1, 256, 0, st>>>(NK, mo, Jbuf, rbuf, delta, ss_c, res, rho_c);
    else k_marker_candidate<false><<<1, 256, 0, st>>>(NK, mo, Jbuf, rbuf, delta, ss_c, res);
    T.End(st);
    if (!chk("k_marker_candidate")) return RSBA_ERR_HIP;
    if (hipMemcpyAsync(res_host, res, RES_SIZE * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) return RSBA_ERR_HIP;
    { hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) { fprintf(stderr, "rsba: marker-chain step failed: %s\n", hipGetErrorString(e)); return RSBA_ERR_HIP; } }
    return RSBA_OK;
  }
  // The step of a solver with free intrinsics: the same five stages on rows of 24 columns, every one reading the state's intrinsics.
  template <typename Timer>
  int StepIntr(hipStream_t st, const IterParams& ip, double loss, double* res_host, Timer& T) {
    const int x = cur, c = 1 - cur, NK = N + prior.K;
    auto chk = [&](const char* what) {
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) { fprintf(stderr, "rsba: %s launch failed: %s\n", what, hipGetErrorString(e)); return false; }
      return true;
    };
    T.Begin("k_marker_intr_eval", st);
    k_marker_intr_eval<<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[x], nfull, dist, half_side, 1, Jbuf, rbuf, ss_x, loss, rho_x, wts);
    T.End(st);
    if (!chk("k_marker_intr_eval")) return RSBA_ERR_HIP;
    T.Begin("k_marker_intr_subset_rows", st);
    k_marker_intr_subset_rows<<<(unsigned)(((size_t)N * 192 + 255) / 256), 256, 0, st>>>(N, mo, Jbuf);
    T.End(st);
    if (prior.K > 0) {
      T.Begin("k_marker_intr_prior_rows", st);
      k_marker_intr_prior_rows<<<(prior.K + 63) / 64, 64, 0, st>>>(prior.K, N, mo, prior.mask, prior.ab, params[x], 1, Jbuf, rbuf, ss_x, rho_x);
      T.End(st);
    }
    size_t lds = (size_t)std::max(2 * RSBA_TB * (RSBA_NB + 1) + RSBA_NB * (RSBA_NB + 1), 5 * 1024) * sizeof(double);
    if (n <= RSBA_CHOL_MAXN) lds = std::max(lds, CholeskyLdsDoubles(n) * sizeof(double));
    T.Begin("k_marker_intr_system", st);
    if (n <= RSBA_CHOL_MAXN) {
      if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k_marker_intr_system<512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      k_marker_intr_system<512><<<1, 512, lds, st>>>(N, NK, n, mo, icol, Jbuf, rbuf, rho_x, A, scale, grad, act_to_full, params[x], params[c], delta, res, ip);
    } else {
      k_marker_intr_system<1024><<<1, 1024, lds, st>>>(N, NK, n, mo, icol, Jbuf, rbuf, rho_x, A, scale, grad, act_to_full, params[x], params[c], delta, res, ip);
    }
    T.End(st);
    if (!chk("k_marker_intr_system")) return RSBA_ERR_HIP;
    T.Begin("k_marker_intr_eval", st);
    k_marker_intr_eval<<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[c], nfull, dist, half_side, 0, nullptr, nullptr, ss_c, loss, rho_c, wts);
    T.End(st);
    if (prior.K > 0) {
      T.Begin("k_marker_intr_prior_rows", st);
      k_marker_intr_prior_rows<<<(prior.K + 63) / 64, 64, 0, st>>>(prior.K, N, mo, prior.mask, prior.ab, params[c], 0, nullptr, nullptr, ss_c, rho_c);
      T.End(st);
    }
    T.Begin("k_marker_intr_candidate", st);
    k_marker_intr_candidate<<<1, 256, 0, st>>>(N, NK, mo, icol, Jbuf, rbuf, delta, ss_c, res, rho_c);
    T.End(st);
    if (!chk("k_marker_intr_candidate")) return RSBA_ERR_HIP;
    if (hipMemcpyAsync(res_host, res, RES_SIZE * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) return RSBA_ERR_HIP;
    { hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) { fprintf(stderr, "rsba: marker-chain step failed: %s\n", hipGetErrorString(e)); return RSBA_ERR_HIP; } }
    return RSBA_OK;
  }
  int SumSquares(hipStream_t st, double* out) {
    if (Reset(st) != RSBA_OK) return RSBA_ERR_HIP;
    if (with_dist) k_marker_eval<false, true><<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[0], IntrDist{intr, dist}, half_side, 0, nullptr, nullptr, ss_x);
    else k_marker_eval<false><<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[0], intr, half_side, 0, nullptr, nullptr, ss_x);
    std::vector<double> h(N);
    if (hipMemcpyAsync(h.data(), ss_x, N * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return RSBA_ERR_HIP;
    double s = 0; for (double v : h) s += v;
    *out = s;
    return RSBA_OK;
  }
  int Download(rsba_problem* p) {
    if (hipMemcpy(p->parameters.data(), params[cur], nfull * 8, hipMemcpyDeviceToHost) != hipSuccess) return RSBA_ERR_HIP;
    if (with_intr) {
      // the state's six values of EVERY camera into the problem's own arrays: the refined ones, and those rsba_solver_set_parameters
      // changed under the extended layout (a held component, a camera without a block).  Without such a call these keep their bits: the
      // state started from them.  A distortion array appears when the problem had none and k1 or k2 was free, or was set to non-zero
      const int C = (int)intr_mask.size();
      std::vector<double> hs(6 * (size_t)C);
      if (hipMemcpy(hs.data(), params[cur] + nfull, hs.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return RSBA_ERR_HIP;
      bool want_dist = !p->distortion.empty();
      for (int k = 0; k < C; ++k) want_dist = want_dist || (intr_mask[k] & 0x30) || hs[6 * (size_t)k + 4] != 0.0 || hs[6 * (size_t)k + 5] != 0.0;
      if (want_dist && p->distortion.empty()) p->distortion.assign(5 * (size_t)C, 0.0);
      for (int k = 0; k < C; ++k) {
        for (int q = 0; q < 4; ++q) p->intrinsics[4 * (size_t)k + q] = hs[6 * (size_t)k + q];
        if (want_dist) { p->distortion[5 * (size_t)k] = hs[6 * (size_t)k + 4]; p->distortion[5 * (size_t)k + 1] = hs[6 * (size_t)k + 5]; }
      }
    }
    return RSBA_OK;
  }
};

}  // namespace rsba
