// Free intrinsics (rsba_problem_set_intrinsics_free) on the marker chain's time-eliminating path: what the THIRD block of a residual
// block — the six values fx fy cx cy k1 k2 of its detecting camera — adds to the split elimination (ba_marker_split.hpp).  No kernel
// of that file changes: the device keeps a current and a candidate copy of intr [C][4] and dist [C][5], scattered from the state
// (k_mc_intr_state), and the kDist instances of the product kernels, k_mc_block_weight and k_mc_candidate<1> run on them.  An
// intrinsics block is one more slot of a time (the last ones: its columns are the highest) with a record in the format the
// accumulations read, and one more row block of pair items; the accumulations, the subset kernels, the reduced solves and
// k_mc_time_step are generic in both.  New here:
//
//   k_mc_intr_state           thread per camera: the state's six values into the two arrays (p1 p2 k3 stay what they were)
//   k_mc_intr_slot_products   thread per (time, intrinsics slot), over the camera's residual blocks at that time (block order):
//                             W = J_t' J_i, g_i = J_i' r, U_ii = J_i' J_i -> the slot's 64-double record, and J_i' J_c -> a source record
//   k_mc_intr_marker_cross    thread per residual block of a camera with a block: J_i' J_m -> a source record
//   k_mc_intr_cross_sum       thread per entry of a (chunk, intrinsics block, camera or marker block) item: its source records in
//                             time order -> xout (rows: intrinsics, columns: camera or marker — the lower triangle)
//   k_mc_intr_candidate       k_mc_candidate<0> with J_i delta_i inside J d
//
// The six columns are analytic, as k_marker_intr_eval forms them: du = (x_d, 0, 1, 0, fx x r2, fx x r2^2), dv = (0, y_d, 0, 1, fy y r2,
// fy y r2^2) at the state's values; the corrector's sqrt(rho') and the weight scale them like the other columns (wsq; null: neither).
// Every sum has a fixed order, no atomics.  Reference: the functors of Main_Calibration/bundle_adjustment.h with the intrinsics as a
// parameter block (tests/marker_intrinsics_ref.py).
#pragma once

namespace rsba {

// the two rows of the intrinsics block of one corner: the corner through the chain as CornerRows carries it, then ProjectCorner<true>'s
// normalised point
__device__ __forceinline__ void IntrColumns(const PoseC& cam, const PoseC& tim, const PoseC& mar, double fx, double fy, const double* ds,
                                            double cx, double cy, double Ji[2][6]) {
  double p[3] = {cx, cy, 0.0};
  auto apply = [&](const PoseC& t) {
    const double q0 = t.R[0] * p[0] + t.R[1] * p[1] + t.R[2] * p[2];
    const double q1 = t.R[3] * p[0] + t.R[4] * p[1] + t.R[5] * p[2];
    const double q2 = t.R[6] * p[0] + t.R[7] * p[1] + t.R[8] * p[2];
    p[0] = q0 + t.T[0]; p[1] = q1 + t.T[1]; p[2] = q2 + t.T[2];
  };
  if (mar.on) apply(mar);
  apply(tim);
  if (cam.on) apply(cam);
  const double k1 = ds[0], k2 = ds[1], p1 = ds[2], p2 = ds[3], k3 = ds[4];
  const double iz = 1.0 / p[2];
  const double x = p[0] * iz, y = p[1] * iz;
  const double xx = x * x, yy = y * y, xy = x * y;
  const double r2 = xx + yy;
  const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
  const double xd = x * rad + (2.0 * p1 * xy + p2 * (r2 + 2.0 * xx));
  const double yd = y * rad + (p1 * (r2 + 2.0 * yy) + 2.0 * p2 * xy);
  const double gx = fx * x * r2, gy = fy * y * r2;
  Ji[0][0] = xd; Ji[0][1] = 0.0; Ji[0][2] = 1.0; Ji[0][3] = 0.0; Ji[0][4] = gx; Ji[0][5] = gx * r2;
  Ji[1][0] = 0.0; Ji[1][1] = yd; Ji[1][2] = 0.0; Ji[1][3] = 1.0; Ji[1][4] = gy; Ji[1][5] = gy * r2;
}

// state: [nfull + 6 C]; camera k's values at nfull + 6 k
__global__ void __launch_bounds__(64) k_mc_intr_state(int C, int nfull, const double* __restrict__ state, double* __restrict__ intr, double* __restrict__ dist) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= C) return;
  const double* s = state + nfull + 6 * (size_t)k;
#pragma unroll
  for (int q = 0; q < 4; ++q) intr[4 * (size_t)k + q] = s[q];
  dist[5 * (size_t)k] = s[4]; dist[5 * (size_t)k + 1] = s[5];
}

struct IntrSplitArgs {
  int nislots, nib;
  const int* __restrict__ is_slot;     // [nislots] the slot S of intrinsics slot j (its record: sp + S RSBA_SP_STRIDE)
  const int* __restrict__ is_cam;      // [nislots] its camera
  const int* __restrict__ ib_ptr;      // [nislots + 1] its residual blocks ...
  const int* __restrict__ ib_blk;      // [nib] ... in block order
  const int* __restrict__ slot_time;   // [nslots]
  const int* __restrict__ time_full;   // [T]
  const MarkerObs* __restrict__ mo;
  const double* __restrict__ obs8;
  const double* __restrict__ intr;     // the CURRENT copies
  const double* __restrict__ dist;
  const double* __restrict__ posec;
  double half_side;
  const double* __restrict__ wsq;      // [N] sqrt(a rho') at x (k_mc_block_weight), or null
  double* __restrict__ sp;
  double* __restrict__ xsrc;           // [nislots + nib][36]: J_i' J_c per intrinsics slot, then J_i' J_m per entry of ib_blk; row q_i, column q at 6 q_i + q
};

__global__ void __launch_bounds__(256) k_mc_intr_slot_products(IntrSplitArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nislots) return;
  const int S = a.is_slot[j], camera = a.is_cam[j];
  const PoseC tim = LoadPose<true>(a.posec, a.time_full[a.slot_time[S]] / 6);
  const double* in = a.intr + 4 * (size_t)camera;
  const double fx = in[0], fy = in[1], ppx = in[2], ppy = in[3];
  double ds[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) ds[i] = a.dist[5 * (size_t)camera + i];
  double W[36], gs[6], U[21], X[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) { W[i] = 0.0; X[i] = 0.0; }
#pragma unroll
  for (int i = 0; i < 6; ++i) gs[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 21; ++i) U[i] = 0.0;
  const double hs = a.half_side;
  for (int e = a.ib_ptr[j]; e < a.ib_ptr[j + 1]; ++e) {
    const int k = a.ib_blk[e];
    const MarkerObs o = a.mo[k];
    const PoseC cam = LoadPose<true>(a.posec, o.full_cam >= 0 ? o.full_cam / 6 : -1);
    const PoseC mar = LoadPose<false>(a.posec, o.full_marker >= 0 ? o.full_marker / 6 : -1);
    const double w = a.wsq ? a.wsq[k] : 1.0;
    const double* ob = a.obs8 + 8 * (size_t)k;
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
      const double cx = CornerX(c, hs), cy = CornerY(c, hs);
      double r[2], Jc[2][6], Jt[2][6], Ji[2][6];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 6; ++q) Jc[i][q] = 0.0;   // (an absent camera transform: CornerRows leaves the block alone)
      CornerRows<true, true, false, true>(cam, tim, mar, fx, fy, ppx, ppy, cx, cy, ob[2 * c], ob[2 * c + 1], r, Jc, Jt, nullptr, ds);
      IntrColumns(cam, tim, mar, fx, fy, ds, cx, cy, Ji);
      ScaleCorner(w, r, Jc, Jt);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int q = 0; q < 6; ++q) Ji[i][q] *= w;
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
          for (int q = 0; q < 6; ++q) W[6 * x + q] = fma(Jt[i][x], Ji[i][q], W[6 * x + q]);
#pragma unroll
        for (int q = 0; q < 6; ++q) gs[q] = fma(Ji[i][q], r[i], gs[q]);
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
          for (int p = 0; p <= q; ++p) U[q * (q + 1) / 2 + p] = fma(Ji[i][q], Ji[i][p], U[q * (q + 1) / 2 + p]);
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
          for (int x = 0; x < 6; ++x) X[6 * q + x] = fma(Ji[i][q], Jc[i][x], X[6 * q + x]);
      }
    }
  }
  double* out = a.sp + (size_t)S * RSBA_SP_STRIDE;
#pragma unroll
  for (int i = 0; i < 36; ++i) out[i] = W[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) out[36 + i] = gs[i];
#pragma unroll
  for (int i = 0; i < 21; ++i) out[42 + i] = U[i];
  out[63] = 0.0;
  double* xo = a.xsrc + (size_t)j * 36;
#pragma unroll
  for (int i = 0; i < 36; ++i) xo[i] = X[i];
}

__global__ void __launch_bounds__(256) k_mc_intr_marker_cross(IntrSplitArgs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.nib) return;
  const int k = a.ib_blk[e];
  const MarkerObs o = a.mo[k];
  const PoseC cam = LoadPose<false>(a.posec, o.full_cam >= 0 ? o.full_cam / 6 : -1);
  const PoseC tim = LoadPose<false>(a.posec, o.full_time / 6);
  const PoseC mar = LoadPose<true>(a.posec, o.full_marker >= 0 ? o.full_marker / 6 : -1);   // (absent: a stand-in's block, which no item names)
  const double* in = a.intr + 4 * (size_t)o.camera;
  const double fx = in[0], fy = in[1], ppx = in[2], ppy = in[3];
  double ds[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) ds[i] = a.dist[5 * (size_t)o.camera + i];
  const double w = a.wsq ? a.wsq[k] : 1.0;
  const double* ob = a.obs8 + 8 * (size_t)k;
  const double hs = a.half_side;
  double X[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) X[i] = 0.0;
#pragma unroll 1
  for (int c = 0; c < 4; ++c) {
    const double cx = CornerX(c, hs), cy = CornerY(c, hs);
    double r[2], Jm[2][6], Ji[2][6];
    CornerRows<false, false, true, true>(cam, tim, mar, fx, fy, ppx, ppy, cx, cy, ob[2 * c], ob[2 * c + 1], r, nullptr, nullptr, Jm, ds);
    IntrColumns(cam, tim, mar, fx, fy, ds, cx, cy, Ji);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int q = 0; q < 6; ++q) { Ji[i][q] *= w; Jm[i][q] *= w; }
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int x = 0; x < 6; ++x) X[6 * q + x] = fma(Ji[i][q], Jm[i][x], X[6 * q + x]);
    }
  }
  double* xo = a.xsrc + ((size_t)a.nislots + e) * 36;
#pragma unroll
  for (int i = 0; i < 36; ++i) xo[i] = X[i];
}

__global__ void __launch_bounds__(256) k_mc_intr_cross_sum(int nxs, const int* __restrict__ xs_item, const int* __restrict__ xs_ptr, const int* __restrict__ xs_src,
                                                           const double* __restrict__ xsrc, double* __restrict__ xout) {
  const int g = blockIdx.x * 256 + threadIdx.x, i = g / 36, q = g - 36 * i;
  if (i >= nxs) return;
  double sum = 0.0;
  for (int e = xs_ptr[i]; e < xs_ptr[i + 1]; ++e) sum += xsrc[(size_t)xs_src[e] * 36 + q];
  xout[(size_t)xs_item[i] * 36 + q] = sum;
}

// k_mc_candidate<0, ., true> with the third block: -(J d).(r + J d / 2) over the rows of camera | time | marker | intrinsics at x.
// ti: the blocks' third columns; intr / dist: the CURRENT copies; wsq: as above.  The workgroup's sum in k_mc_candidate's order.
__global__ void __launch_bounds__(256) k_mc_intr_candidate(int N, int T, const TimeSlots* __restrict__ ts, const IntrSlots* __restrict__ ti, const MarkerObs* __restrict__ mo,
                                                           const double* __restrict__ obs8, const double* __restrict__ intr, const double* __restrict__ dist,
                                                           double half_side, const double* __restrict__ posec, const double* __restrict__ delta_r,
                                                           const double* __restrict__ delta_t, const int* __restrict__ blk_time, double* __restrict__ bp_time,
                                                           const double* __restrict__ wsq) {
  __shared__ double s_w[4];
  const int k = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double sum = 0.0;
  if (k < N) {
    const TimeSlots s = ts[k];
    const MarkerObs o = mo[k];
    const int ci = ti[k].col_intr;
    const double* in = intr + 4 * (size_t)s.camera;
    const double fx = in[0], fy = in[1], ppx = in[2], ppy = in[3];
    double ds[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) ds[i] = dist[5 * (size_t)s.camera + i];
    const double* ob = obs8 + 8 * (size_t)k;
    const PoseC cam = LoadPose<true>(posec, o.full_cam >= 0 ? o.full_cam / 6 : -1);
    const PoseC tim = LoadPose<true>(posec, o.full_time / 6);
    const PoseC mar = LoadPose<true>(posec, o.full_marker >= 0 ? o.full_marker / 6 : -1);
    double dl[24];
    const int t = blk_time[k];
    const double w = wsq ? wsq[k] : 1.0;
#pragma unroll
    for (int x = 0; x < 6; ++x) {
      dl[x] = s.col_cam >= 0 ? delta_r[s.col_cam + x] : 0.0;
      dl[6 + x] = delta_t[6 * t + x];
      dl[12 + x] = s.col_marker >= 0 ? delta_r[s.col_marker + x] : 0.0;
      dl[18 + x] = ci >= 0 ? delta_r[ci + x] : 0.0;
    }
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
      const double cx = CornerX(c, half_side), cy = CornerY(c, half_side);
      double r[2], Jc[2][6], Jt[2][6], Jm[2][6], Ji[2][6];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 6; ++q) Jc[i][q] = 0.0;
      CornerRows<true, true, true, true>(cam, tim, mar, fx, fy, ppx, ppy, cx, cy, ob[2 * c], ob[2 * c + 1], r, Jc, Jt, Jm, ds);
      IntrColumns(cam, tim, mar, fx, fy, ds, cx, cy, Ji);
      ScaleCorner(w, r, Jc, Jt);
      // (an absent marker transform: its block is formed from the stand-in pose's constants and meets dl[12..17] = 0)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        double m = 0.0;
#pragma unroll
        for (int x = 0; x < 6; ++x) m += Jc[i][x] * dl[x];
#pragma unroll
        for (int x = 0; x < 6; ++x) m += Jt[i][x] * dl[6 + x];
#pragma unroll
        for (int x = 0; x < 6; ++x) m += (Jm[i][x] * w) * dl[12 + x];
#pragma unroll
        for (int x = 0; x < 6; ++x) m += (Ji[i][x] * w) * dl[18 + x];
        sum -= m * (r[i] + 0.5 * m);
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (lane == 0) s_w[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double* out = bp_time + 4 * ((size_t)T + blockIdx.x);
    out[0] = 0.0; out[1] = 0.0; out[2] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
  }
}

}  // namespace rsba
