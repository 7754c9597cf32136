// The Jacobian of ceres::Problem::Evaluate on a resident solver (rsba_solver_evaluate_jacobian, include/rsba.h): the values of the
// compressed-row matrix whose structure ba_evaluate_plan.hpp lays out, at the solver's current device parameters.  Rows in the
// problem's observation order, columns = parameter offsets; observation i's rows are one contiguous piece of `values` starting at
// off[i], row after row, each row its free blocks' columns compacted (camera | point, camera | time | marker).  With a loss a block's
// rows leave multiplied by sqrt(rho'(s)) (LossAndScale), one rounding of sq * J.
//
// Like ba_evaluate.hpp's, these kernels write only into the arena the host hands them, and they add nothing up: every value is
// written once by one thread, so two calls return the same bits.  The rows are ba_math.hpp's — ResidualJacobian on
// k_camera_constants' output, MarkerCornerResidualJacobian on k_cov_pose_constants' — as the gradient's are.
//
// Which blocks of an observation are present is read from the row width (off[i + 1] - off[i]) / rows — on the point model it says
// it all: 3 point, 6 camera, 9 both — and on the marker chain from what evaluate already keeps on the device: live[b] of the blocks
// the observation names (a named block is referenced, so live means "not constant").
#pragma once
#include <hip/hip_runtime.h>

#include "ba_evaluate.hpp"

namespace rsba {

#define RSBA_JAC_OBS 256   // observations per workgroup of k_eval_jacobian_points: 256 x 18 doubles of LDS

// Point model.  The output is a pure store stream (18 doubles per observation with both blocks free), so the work is laid out for
// the stores: thread t of a workgroup takes observation 256 b + t of the PROBLEM's order, gathers its camera's constants and its
// point through `rows` (camera, device position of the point) and puts its 2 x width values where they belong in the workgroup's
// piece — contiguous, because off ascends with the observation — in LDS; the workgroup then streams the piece out, 16 bytes per
// lane, neighbouring lanes neighbouring addresses.  (A piece starts at a multiple of 6 doubles, so it is 16-byte aligned and of even
// length.)  The solver's point-major slots, `order` and the Schur variant do not enter: the matrix is the same under all of them.
__global__ void __launch_bounds__(RSBA_JAC_OBS)
k_eval_jacobian_points(int N, const EvalJacobianPointRow* __restrict__ rows, const double2* __restrict__ obs, const int64_t* __restrict__ off,
                       const double* __restrict__ camc, const double* __restrict__ pts, double loss,
                       double* __restrict__ values) {
  __shared__ double2 stage2[RSBA_JAC_OBS * 9];
  double* stage = reinterpret_cast<double*>(stage2);
  const int i0 = blockIdx.x * RSBA_JAC_OBS, i = i0 + (int)threadIdx.x;
  const int64_t base = off[i0], end = off[min(i0 + RSBA_JAC_OBS, N)];
  if (i < N) {
    const int64_t o = off[i];
    const int w = (int)(off[i + 1] - o) >> 1;
    if (w > 0) {
      const EvalJacobianPointRow rw = rows[i];
      const bool cam_on = w != 3, pt_on = w != 6;   // widths: 3 point, 6 camera, 9 both
      const double X[3] = {pts[3 * (size_t)rw.point], pts[3 * (size_t)rw.point + 1], pts[3 * (size_t)rw.point + 2]};
      const double2 uv = obs[i];
      double r[2], jc[12], jp[6], sq;
      ResidualJacobian(camc + (size_t)rw.camera * CC_STRIDE, X, uv.x, uv.y, r, jc, jp);
      (void)LossAndScale(loss, r[0] * r[0] + r[1] * r[1], &sq);
      double* d = stage + (o - base);
      if (cam_on) {
#pragma unroll
        for (int a = 0; a < 6; ++a) { d[a] = sq * jc[a]; d[w + a] = sq * jc[6 + a]; }
        d += 6;
      }
      if (pt_on) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { d[a] = sq * jp[a]; d[w + a] = sq * jp[3 + a]; }
      }
    }
  }
  __syncthreads();
  const int n2 = (int)(end - base) >> 1;
  double2* out = reinterpret_cast<double2*>(values + base);
  for (int e = threadIdx.x; e < n2; e += RSBA_JAC_OBS) out[e] = stage2[e];
}

// Marker-chain models, both paths: one thread per observation of the problem's order, the corners one after the other with the loop
// kept rolled, as in k_eval_marker — one corner's 2 x 18 rows are live at a time.  A corner's two rows are stored as they are formed,
// the columns of absent blocks (base, constant) skipped; s is known only after the fourth corner, so with a loss the thread then
// scales its own 8 x width values in place, as the residual output does: every value is the single rounding of sq * J.
// wts (nullptr: none): the observations' weights, passed when the loss applies: sq = sqrt(a_i) sqrt(rho').
// kDist: dist = the cameras' five distortion coefficients [C][5], indexed as intr.
template <bool kDist = false>
__global__ void __launch_bounds__(64)
k_eval_jacobian_marker(int N, const EvalMarkerRow* __restrict__ rows, const double* __restrict__ obs8, typename IntrArg<kDist>::type intr,
                       const double* __restrict__ pc, const int64_t* __restrict__ off, const unsigned char* __restrict__ live,
                       double half_side, double loss, double* __restrict__ values, const double* __restrict__ wts = nullptr) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= N) return;
  const int64_t o = off[i];
  const int w = (int)(off[i + 1] - o) >> 3;
  if (w == 0) return;
  const EvalMarkerRow rw = rows[i];
  const double* o8 = obs8 + 8 * (size_t)i;
  const double* pcc = rw.cam_block >= 0 ? pc + (size_t)rw.cam_block * CC_STRIDE : nullptr;
  const double* pct = pc + (size_t)rw.time_block * CC_STRIDE;
  const double* pcm = rw.marker_block >= 0 ? pc + (size_t)rw.marker_block * CC_STRIDE : nullptr;
  const bool on[3] = {rw.cam_block >= 0 && live[rw.cam_block] != 0, live[rw.time_block] != 0, rw.marker_block >= 0 && live[rw.marker_block] != 0};
  double* v = values + o;
  double ss = 0.0;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    // top-left, top-right, bottom-right, bottom-left (bundle_adjustment.h:92-101)
    const double cx = (k == 0 || k == 3) ? -half_side : half_side, cy = k < 2 ? half_side : -half_side;
    double rk[2], J[36];
    MarkerCornerResidualJacobian<kDist>(pcc, pct, pcm, IntrOf(intr) + 4 * rw.camera, cx, cy, o8[2 * k], o8[2 * k + 1], rk, J, DistOf(intr, rw.camera));
    ss += rk[0] * rk[0] + rk[1] * rk[1];
    double* d = v + 2 * k * w;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (!on[b]) continue;
#pragma unroll
      for (int a = 0; a < 6; ++a) { d[a] = J[6 * b + a]; d[w + a] = J[18 + 6 * b + a]; }
      d += 6;
    }
  }
  double sq;
  (void)LossAndScale(loss, ss, &sq);
  if (wts != nullptr) sq *= sqrt(wts[i]);
  if (sq != 1.0) {
    for (int e = 0; e < 8 * w; ++e) v[e] *= sq;
  }
}

// Constant components of partly constant blocks (rsba_problem_set_parameter_subset_constant): exact 0.0 in their columns of the
// values k_eval_jacobian_marker wrote — the structure keeps the block's six columns, so J'r equals the gradient slot for slot.
// One thread per observation, the layout k_eval_jacobian_marker walks.  bsub[b]: block b's mask.
__global__ void __launch_bounds__(64)
k_eval_jacobian_subset(int N, const EvalMarkerRow* __restrict__ rows, const int64_t* __restrict__ off, const unsigned char* __restrict__ live,
                       const unsigned char* __restrict__ bsub, double* __restrict__ values) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= N) return;
  const int64_t o = off[i];
  const int w = (int)(off[i + 1] - o) >> 3;
  if (w == 0) return;
  const EvalMarkerRow rw = rows[i];
  const int blk[3] = {rw.cam_block, rw.time_block, rw.marker_block};
  double* v = values + o;
  int col = 0;
  for (int b = 0; b < 3; ++b) {
    if (blk[b] < 0 || live[blk[b]] == 0) continue;
    const int sub = bsub[blk[b]];
    for (int a = 0; a < 6; ++a)
      if ((sub >> a) & 1)
        for (int r = 0; r < 8; ++r) v[r * w + col + a] = 0.0;
    col += 6;
  }
}

// What a solver keeps for rsba_solver_evaluate_jacobian beyond EvalDevice: the layout on the host (rsba_solver_jacobian_structure
// answers from it and launches nothing) and, from the first call that wants values, the observations' offsets and the point
// model's problem-order tables on the device.  The values are carved from EvalDevice's arena.
struct EvalJacobianDevice {
  bool planned = false, built = false;
  EvalJacobianLayout layout;
  int64_t* off = nullptr;
  EvalJacobianPointRow* rows = nullptr;   // point model
  double2* obs = nullptr;                 // point model: (u, v) in the problem's order

  void Free() {
    void* ptrs[] = {off, rows, obs};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    *this = EvalJacobianDevice();
  }
};

// The priors' rows of the CRS Jacobian, behind the observations' values (base: their count): six rows of six values A[i][q] per prior
// whose block has columns (col >= 0), in the priors' order; exact 0.0 in the columns of constant components; none for a prior on a
// constant block (its rows are empty).  Thread per value.
__global__ void __launch_bounds__(256) k_eval_jacobian_prior(int K, const int* __restrict__ col, const int* __restrict__ mask, const double* __restrict__ ab,
                                                             int64_t base, double* __restrict__ values) {
  const int e = blockIdx.x * 256 + threadIdx.x, k = e / 36, iq = e - 36 * k;
  if (k >= K || col[k] < 0) return;
  int before = 0;
  for (int j = 0; j < k; ++j) before += col[j] >= 0 ? 1 : 0;
  values[base + 36 * (int64_t)before + iq] = ((mask[k] >> (iq % 6)) & 1) ? 0.0 : ab[42 * (size_t)k + iq];
}

}  // namespace rsba
