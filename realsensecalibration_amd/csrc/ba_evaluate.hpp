// ceres::Problem::Evaluate (without the Jacobian) on a resident solver: cost, residuals in the problem's observation order and the
// gradient in the problem's parameter layout, at the solver's current device parameters (rsba_solver_evaluate, include/rsba.h).
//
// The kernels are this file's own and write only into the arena the host hands them: the LM state — parameters, scales, kept
// linearisations, stage flags — is read, never written, so run -> evaluate -> run gives the bits of run -> run.
//
// Every sum is taken in an order that depends on the problem's index arrays alone (no floating-point atomics), so two calls return
// the same bits:
//   cost              per-workgroup partials on a fixed grid, summed by k_eval_cost in index order
//   point gradient    a wavefront owns a point: its lanes walk the point's observations in chunks of 64, then a butterfly
//   camera gradient   the camera-major index of ba_evaluate_plan.hpp: a camera's observations in RSBA_EVAL_CAM_SEGS contiguous
//                     segments, one workgroup each (k_eval_cam_grad), the segments' sums added in order (k_eval_cam_sum)
//   marker chain      J'r of every observation (18 values, camera | time | marker) from one thread, then one workgroup per block
//                     of [C | T | M] over the block's (observation, slot) list (k_eval_marker_block_sum)
//                     (free intrinsics under the extended layout: 24 values and C more blocks, k_eval_marker_intr)
// A workgroup's sum is: a thread's own terms in ascending order with stride 256, the wavefront's butterfly, the four wavefronts
// left to right (EvalBlockSum).
//
// Residuals and Jacobian rows come from ba_math.hpp — Residual / ResidualPointJacobian / ResidualJacobian for the point model,
// MarkerCornerResidualJacobian for the marker chain on BOTH of its paths, so a dense-path solver and a time-eliminating one return
// the same bits at the same parameters.  With a loss, a block's residuals leave scaled by sqrt(rho'(s)) and its gradient terms by
// rho'(s) (LossAndScale: the corrector the solve applies).  The residual-only instances (kGrad = false) form no Jacobian row: the
// point model's calls Residual, the marker chain's leaves the rows of MarkerCornerResidualJacobian unread (see k_eval_marker).
#pragma once
#include <hip/hip_runtime.h>

#include "ba_covariance.hpp"
#include "ba_evaluate_plan.hpp"
#include "ba_math.hpp"
#include "ba_point_kernels.hpp"

namespace rsba {

#define RSBA_EVAL_CAM_SEGS 8   // workgroups per camera of k_eval_cam_grad: 512 at 64 cameras, two per CU

// Sum of kN values per thread over a 256-thread workgroup, in every thread: butterfly inside the wavefront, then the four
// wavefronts left to right.  lds: 4 * kN doubles.
template <int kN>
__device__ __forceinline__ void EvalBlockSum(double (&v)[kN], double* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kN; ++i) v[i] = WaveSum(v[i]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kN; ++i) lds[wave * kN + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kN; ++i) v[i] = ((lds[i] + lds[kN + i]) + lds[2 * kN + i]) + lds[3 * kN + i];
}

// Point model: residuals (scattered to the problem's order through `order`), the cost's partials and — kGrad — every point's
// gradient (through pt_perm to the problem's point order).  One wavefront per point, the arrays of the solver's point-major order;
// any number of views per point.  live[C + j] == 0: point j of the problem is constant or unreferenced, its slots are 0.0.
template <bool kGrad>
__global__ void __launch_bounds__(256)
k_eval_points(int P, int C, const double* __restrict__ obs_u, const double* __restrict__ obs_v, const int* __restrict__ obs_cam,
              const int* __restrict__ pt_ptr, const double* __restrict__ camc, const double* __restrict__ pts, const int* __restrict__ order,
              const int* __restrict__ pt_perm, const unsigned char* __restrict__ live, double loss, double* __restrict__ residuals,
              double* __restrict__ gradient, double* __restrict__ cost_parts) {
  __shared__ double part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double cost = 0.0;
  for (int j = blockIdx.x * 4 + wave; j < P; j += gridDim.x * 4) {
    const int b = pt_ptr[j], k = pt_ptr[j + 1] - b;
    const double X[3] = {pts[3 * (size_t)j], pts[3 * (size_t)j + 1], pts[3 * (size_t)j + 2]};
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int q = lane; q < k; q += 64) {
      const double* cc = camc + (size_t)obs_cam[b + q] * CC_STRIDE;
      double r[2], jp[6];
      if constexpr (kGrad) ResidualPointJacobian(cc, X, obs_u[b + q], obs_v[b + q], r, jp);
      else Residual(cc, X, obs_u[b + q], obs_v[b + q], r);
      double sq;
      cost += LossAndScale(loss, r[0] * r[0] + r[1] * r[1], &sq);
      const double rt0 = sq * r[0], rt1 = sq * r[1];
      if (residuals != nullptr) {
        const size_t o = 2 * (size_t)order[b + q];
        residuals[o] = rt0; residuals[o + 1] = rt1;
      }
      if constexpr (kGrad) {
        g0 += (sq * jp[0]) * rt0 + (sq * jp[3]) * rt1;
        g1 += (sq * jp[1]) * rt0 + (sq * jp[4]) * rt1;
        g2 += (sq * jp[2]) * rt0 + (sq * jp[5]) * rt1;
      }
    }
    if constexpr (kGrad) {
      g0 = WaveSum(g0); g1 = WaveSum(g1); g2 = WaveSum(g2);
      const int jo = pt_perm != nullptr ? pt_perm[j] : j;
      const bool on = live[(size_t)C + jo] != 0;
      if (lane < 3) gradient[6 * (size_t)C + 3 * (size_t)jo + lane] = on ? (lane == 0 ? g0 : (lane == 1 ? g1 : g2)) : 0.0;
    }
  }
  cost = WaveSum(cost);
  if (lane == 0) part[wave] = cost;
  __syncthreads();
  if (threadIdx.x == 0) cost_parts[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// Point model, camera gradient, first stage: workgroup (camera c, segment g) sums Jc'r over its contiguous part of the camera's
// list (cam_slot: the solver's observation slots, ascending; cam_point: the device position of each slot's point).
__global__ void __launch_bounds__(256)
k_eval_cam_grad(const int* __restrict__ cam_ptr, const int* __restrict__ cam_slot, const int* __restrict__ cam_point,
                const double* __restrict__ obs_u, const double* __restrict__ obs_v, const double* __restrict__ camc,
                const double* __restrict__ pts, double loss, double* __restrict__ parts) {
  __shared__ double lds[4 * 6];
  const int c = blockIdx.x / RSBA_EVAL_CAM_SEGS, seg = blockIdx.x - c * RSBA_EVAL_CAM_SEGS;
  const int b = cam_ptr[c], n = cam_ptr[c + 1] - b;
  const int per = (n + RSBA_EVAL_CAM_SEGS - 1) / RSBA_EVAL_CAM_SEGS;
  const int lo = min(n, seg * per), hi = min(n, lo + per);
  const double* cc = camc + (size_t)c * CC_STRIDE;
  double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = lo + (int)threadIdx.x; q < hi; q += 256) {
    const int s = cam_slot[b + q];
    const size_t j = (size_t)cam_point[b + q];
    const double X[3] = {pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]};
    double r[2], jc[12], jp[6];
    ResidualJacobian(cc, X, obs_u[s], obs_v[s], r, jc, jp);
    double sq;
    (void)LossAndScale(loss, r[0] * r[0] + r[1] * r[1], &sq);
    const double rt0 = sq * r[0], rt1 = sq * r[1];
#pragma unroll
    for (int a = 0; a < 6; ++a) g[a] += (sq * jc[a]) * rt0 + (sq * jc[6 + a]) * rt1;
  }
  EvalBlockSum<6>(g, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) parts[(size_t)blockIdx.x * 6 + a] = g[a];
  }
}

// ... second stage: the segments' sums in order; 0.0 for a constant or unreferenced camera (live[c] == 0).
__global__ void __launch_bounds__(256)
k_eval_cam_sum(int C, const double* __restrict__ parts, const unsigned char* __restrict__ live, double* __restrict__ gradient) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 6 * C) return;
  const int c = i / 6, a = i - 6 * c;
  double v = 0.0;
#pragma unroll
  for (int seg = 0; seg < RSBA_EVAL_CAM_SEGS; ++seg) v += parts[((size_t)c * RSBA_EVAL_CAM_SEGS + seg) * 6 + a];
  gradient[i] = live[c] != 0 ? v : 0.0;
}

// Marker-chain models, both paths: one thread per observation of the problem's order.  rows / obs8 in that order, pc the pose
// constants of every block of [C | T | M] at the current parameters (k_cov_pose_constants).  kGrad: J'r of the observation, scaled
// by rho'(s), into obs_grad[18 i ..] — camera | time | marker, zeros for a block the functor does not have.  The corners are walked
// one after the other (the loop is kept rolled): one corner's 2 x 18 rows are live at a time and J'r is added up corner by corner;
// the 8 x 18 block is never stored.  A corner's raw residuals are written as they are formed and — s is known only after the
// fourth corner — scaled in place by the same thread when a loss applies.  kGrad = false calls the same function and never reads
// its J: the rows are not computed because the compiler drops the dead stores after inlining (82 registers against 208; the code
// object is the check, tools/kernel_resources.py).  wts (nullptr: none): the observations' weights a_i (ceres::ScaledLoss), passed
// when the loss applies: the cost a_i rho(s), residuals scaled by sqrt(a_i) sqrt(rho'), J'r by its square.
// kDist: dist = the cameras' five distortion coefficients [C][5], indexed as intr (ProjectCorner, ba_math.hpp).
template <bool kGrad, bool kDist = false>
__global__ void __launch_bounds__(64)
k_eval_marker(int N, const EvalMarkerRow* __restrict__ rows, const double* __restrict__ obs8, typename IntrArg<kDist>::type intr,
              const double* __restrict__ pc, double half_side, double loss, double* __restrict__ residuals,
              double* __restrict__ obs_grad, double* __restrict__ cost_parts, const double* __restrict__ wts = nullptr) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  double rho = 0.0;
  if (i < N) {
    const EvalMarkerRow rw = rows[i];
    const double* o8 = obs8 + 8 * (size_t)i;
    const double* pcc = rw.cam_block >= 0 ? pc + (size_t)rw.cam_block * CC_STRIDE : nullptr;
    const double* pct = pc + (size_t)rw.time_block * CC_STRIDE;
    const double* pcm = rw.marker_block >= 0 ? pc + (size_t)rw.marker_block * CC_STRIDE : nullptr;
    double g[18], ss = 0.0;
#pragma unroll
    for (int q = 0; q < 18; ++q) g[q] = 0.0;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      // top-left, top-right, bottom-right, bottom-left (bundle_adjustment.h:92-101)
      const double cx = (k == 0 || k == 3) ? -half_side : half_side, cy = k < 2 ? half_side : -half_side;
      double rk[2], J[36];
      MarkerCornerResidualJacobian<kDist>(pcc, pct, pcm, IntrOf(intr) + 4 * rw.camera, cx, cy, o8[2 * k], o8[2 * k + 1], rk, J, DistOf(intr, rw.camera));
      ss += rk[0] * rk[0] + rk[1] * rk[1];
      if (residuals != nullptr) { residuals[8 * (size_t)i + 2 * k] = rk[0]; residuals[8 * (size_t)i + 2 * k + 1] = rk[1]; }
      if constexpr (kGrad) {
#pragma unroll
        for (int q = 0; q < 18; ++q) g[q] += J[q] * rk[0] + J[18 + q] * rk[1];
      }
    }
    double sq;
    rho = LossAndScale(loss, ss, &sq);
    if (wts != nullptr) { const double a = wts[i]; rho *= a; sq *= sqrt(a); }
    if (residuals != nullptr && sq != 1.0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) residuals[8 * (size_t)i + e] *= sq;
    }
    if constexpr (kGrad) {
      const double w = sq * sq;
#pragma unroll
      for (int q = 0; q < 18; ++q) obs_grad[18 * (size_t)i + q] = w * g[q];
    }
  }
  rho = WaveSum(rho);
  if (threadIdx.x == 0) cost_parts[blockIdx.x] = rho;
}

// A solver with free intrinsics under the extended layout (rsba_solver_set_extended_layout), both paths: k_eval_marker's walk with the
// camera values of the STATE — params continues behind the nfull pose values with fx fy cx cy k1 k2 of every camera; p1 p2 k3 stay
// dist's [C][5] — and, kGrad, six more J'r values per observation: the analytic columns of k_marker_intr_eval,
//   du / d (fx cx k1 k2) = xd, 1, fx x r2, fx x r2^2     dv / d (fy cy k1 k2) = yd, 1, fy y r2, fy y r2^2
// at the normalised point (x, y) the corner's chain gives (MarkerCornerIntrinsicsTerms, ba_math.hpp).  The 18 pose values go to obs_grad[18 i ..], the six to
// obs_grad[18 N + 6 i ..] (EvalMarkerIntrPlan: k_eval_marker_block_sum reads both through its lists).  Always the distortion form and
// always the weights' pointer test, as k_eval_marker<., true>.
template <bool kGrad>
__global__ void __launch_bounds__(64)
k_eval_marker_intr(int N, const EvalMarkerRow* __restrict__ rows, const double* __restrict__ obs8, const double* __restrict__ params, int nfull,
                   const double* __restrict__ dist, const double* __restrict__ pc, double half_side, double loss, double* __restrict__ residuals,
                   double* __restrict__ obs_grad, double* __restrict__ cost_parts, const double* __restrict__ wts) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  double rho = 0.0;
  if (i < N) {
    const EvalMarkerRow rw = rows[i];
    const double* o8 = obs8 + 8 * (size_t)i;
    const double* pcc = rw.cam_block >= 0 ? pc + (size_t)rw.cam_block * CC_STRIDE : nullptr;
    const double* pct = pc + (size_t)rw.time_block * CC_STRIDE;
    const double* pcm = rw.marker_block >= 0 ? pc + (size_t)rw.marker_block * CC_STRIDE : nullptr;
    const double* sv = params + (size_t)nfull + 6 * (size_t)rw.camera;
    const double intr4[4] = {sv[0], sv[1], sv[2], sv[3]};
    const double kd5[5] = {sv[4], sv[5], dist[5 * (size_t)rw.camera + 2], dist[5 * (size_t)rw.camera + 3], dist[5 * (size_t)rw.camera + 4]};
    double g[24], ss = 0.0;
#pragma unroll
    for (int q = 0; q < 24; ++q) g[q] = 0.0;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      const double cx = (k == 0 || k == 3) ? -half_side : half_side, cy = k < 2 ? half_side : -half_side;
      double rk[2], J[36];
      MarkerCornerResidualJacobian<true>(pcc, pct, pcm, intr4, cx, cy, o8[2 * k], o8[2 * k + 1], rk, J, kd5);
      ss += rk[0] * rk[0] + rk[1] * rk[1];
      if (residuals != nullptr) { residuals[8 * (size_t)i + 2 * k] = rk[0]; residuals[8 * (size_t)i + 2 * k + 1] = rk[1]; }
      if constexpr (kGrad) {
#pragma unroll
        for (int q = 0; q < 18; ++q) g[q] += J[q] * rk[0] + J[18 + q] * rk[1];
        double it[5];
        MarkerCornerIntrinsicsTerms(pcc, pct, pcm, intr4, kd5, cx, cy, it);
        const double xd = it[0], yd = it[1], gx = it[2], gy = it[3], r2 = it[4];
        g[18] += xd * rk[0]; g[19] += yd * rk[1]; g[20] += rk[0]; g[21] += rk[1];
        g[22] += gx * rk[0] + gy * rk[1];
        g[23] += (gx * r2) * rk[0] + (gy * r2) * rk[1];
      }
    }
    double sq;
    rho = LossAndScale(loss, ss, &sq);
    if (wts != nullptr) { const double a = wts[i]; rho *= a; sq *= sqrt(a); }
    if (residuals != nullptr && sq != 1.0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) residuals[8 * (size_t)i + e] *= sq;
    }
    if constexpr (kGrad) {
      const double w = sq * sq;
#pragma unroll
      for (int q = 0; q < 18; ++q) obs_grad[18 * (size_t)i + q] = w * g[q];
#pragma unroll
      for (int q = 0; q < 6; ++q) obs_grad[18 * (size_t)N + 6 * (size_t)i + q] = w * g[18 + q];
    }
  }
  rho = WaveSum(rho);
  if (threadIdx.x == 0) cost_parts[blockIdx.x] = rho;
}

// ... the gradient of block b of [C | T | M]: its list's six-value pieces of obs_grad, ascending observations; 0.0 for a constant
// block and for one no residual references as a parameter (the fixed base blocks among them).
__global__ void __launch_bounds__(256)
k_eval_marker_block_sum(const int* __restrict__ list_ptr, const int* __restrict__ list_obs, const unsigned char* __restrict__ list_slot,
                        const double* __restrict__ obs_grad, const unsigned char* __restrict__ live, double* __restrict__ gradient) {
  __shared__ double lds[4 * 6];
  const int b = blockIdx.x;
  const bool on = live[b] != 0;
  double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (on) {
    const int lo = list_ptr[b], hi = list_ptr[b + 1];
    for (int q = lo + (int)threadIdx.x; q < hi; q += 256) {
      const double* og = obs_grad + 18 * (size_t)list_obs[q] + 6 * list_slot[q];
#pragma unroll
      for (int a = 0; a < 6; ++a) g[a] += og[a];
    }
  }
  EvalBlockSum<6>(g, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) gradient[6 * (size_t)b + a] = on ? g[a] : 0.0;
  }
}

// Constant components of partly constant blocks (rsba_problem_set_parameter_subset_constant): 0.0 in their gradient slots, after
// k_eval_marker_block_sum wrote the blocks' sums (Ceres' gradient has the block's local size; here the slots stay and hold zeros).
// bsub[b]: block b's mask.
__global__ void __launch_bounds__(256) k_eval_subset_gradient(int nb, const unsigned char* __restrict__ bsub, double* __restrict__ gradient) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 6 * nb) return;
  if ((bsub[i / 6] >> (i % 6)) & 1) gradient[i] = 0.0;
}

// cost = 1/2 x the n partials, summed in index order by one workgroup
__global__ void __launch_bounds__(256) k_eval_cost(int n, const double* __restrict__ parts, double* __restrict__ cost) {
  __shared__ double lds[4];
  double v[1] = {0.0};
  for (int i = threadIdx.x; i < n; i += 256) v[0] += parts[i];
  EvalBlockSum<1>(v, lds);
  if (threadIdx.x == 0) *cost = 0.5 * v[0];
}

// The priors of a marker-chain solver (PriorDevice, ba_marker_kernels.hpp) behind the observations' work: residuals A (x - b) (six per
// prior, ascending parameter offset; res: where the first goes, or nullptr), A~'A (x - b) added to the gradient slots of a block with
// columns (col >= 0; A~: without the columns of its constant components, whose slots stay 0.0) and sum |A (x - b)|^2 as one more of
// the cost's partials, summed over the priors in order by thread 0.  No loss applies to a prior.  One workgroup, thread per prior.
__global__ void __launch_bounds__(256) k_eval_prior(int K, const int* __restrict__ full, const int* __restrict__ col, const int* __restrict__ mask,
                                                    const double* __restrict__ ab, const double* __restrict__ params, double* __restrict__ res,
                                                    double* __restrict__ gradient, double* __restrict__ pe, double* __restrict__ cost_part) {
  for (int k = threadIdx.x; k < K; k += 256) {
    const double* __restrict__ A = ab + 42 * (size_t)k;
    const double* __restrict__ x = params + full[k];
    double d[6], r[6], ss = 0.0;
    for (int q = 0; q < 6; ++q) d[q] = x[q] - A[36 + q];
    for (int i = 0; i < 6; ++i) { double t = 0.0; for (int q = 0; q < 6; ++q) t += A[6 * i + q] * d[q]; r[i] = t; ss += t * t; }
    pe[k] = ss;
    if (res) for (int i = 0; i < 6; ++i) res[6 * (size_t)k + i] = r[i];
    if (gradient && col[k] >= 0) {
      for (int q = 0; q < 6; ++q) {
        if ((mask[k] >> q) & 1) continue;
        double g = 0.0;
        for (int i = 0; i < 6; ++i) g += A[6 * i + q] * r[i];
        gradient[full[k] + q] += g;
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) { double t = 0.0; for (int k = 0; k < K; ++k) t += pe[k]; *cost_part = t; }
}

// Point model on a sharded solver: what the ranks add up, [cost | 6C camera gradient | C "some observation of mine references
// camera c" flags], from this rank's cost and k_eval_cam_sum's output (the shard's own sums; 0.0 where the shard has nothing).
// grad false: the cost alone.
__global__ void __launch_bounds__(256)
k_eval_shard_pack(int C, bool grad, const double* __restrict__ cost, const double* __restrict__ gradient, const int* __restrict__ cam_ptr,
                  double* __restrict__ pay) {
  const int n = grad ? 7 * C + 1 : 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (i == 0) pay[0] = *cost;
    else if (i <= 6 * C) pay[i] = gradient[i - 1];
    else { const int c = i - 1 - 6 * C; pay[i] = cam_ptr[c + 1] > cam_ptr[c] ? 1.0 : 0.0; }
  }
}

// ... and back from the all-ranks sums: the cost, and the camera slots under the GROUP's zero mask — 0.0 for a constant camera and
// for one no rank references; a camera this shard never observes but another does carries the other ranks' sum.
__global__ void __launch_bounds__(256)
k_eval_shard_unpack(int C, bool grad, const double* __restrict__ pay, const unsigned char* __restrict__ cam_const, double* __restrict__ cost,
                    double* __restrict__ gradient) {
  const int n = grad ? 6 * C + 1 : 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (i == 0) { *cost = pay[0]; continue; }
    const int c = (i - 1) / 6;
    gradient[i - 1] = cam_const[c] != 0 || pay[1 + 6 * C + c] == 0.0 ? 0.0 : pay[i];
  }
}

// What a solver keeps for rsba_solver_evaluate: the index tables (built on the first call, from the problem's index arrays alone)
// and the scratch arena (grows only: a repeated call neither allocates nor frees).
struct EvalDevice {
  bool built = false;
  // point model: the camera-major index, `order` and pt_perm (nullptr: identity) as the kernels read them
  int *cam_ptr = nullptr, *cam_slot = nullptr, *cam_point = nullptr, *order = nullptr, *pt_perm = nullptr;
  // marker chain: rows and observations in the problem's order, the block-major lists
  EvalMarkerRow* rows = nullptr;
  double *obs8 = nullptr, *intr = nullptr;
  int *list_ptr = nullptr, *list_obs = nullptr;
  unsigned char* list_slot = nullptr;
  unsigned char* live = nullptr;   // per block of the gradient: != 0 computed, 0 written as 0.0 (EvalPointLive / EvalMarkerLive)
  unsigned char* cam_const = nullptr;   // point model with a communicator: per camera, != 0 constant (k_eval_shard_unpack)
  unsigned char* bsub = nullptr;        // marker chain, a solver with constant components: per block its mask (nullptr: none)
  char* arena = nullptr;
  size_t arena_cap = 0;

  void Free() {
    void* ptrs[] = {cam_ptr, cam_slot, cam_point, order, pt_perm, rows, obs8, intr, list_ptr, list_obs, list_slot, live, cam_const, bsub, arena};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    *this = EvalDevice();
  }
};

}  // namespace rsba
