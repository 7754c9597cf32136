// Marker-chain model at scale: many times x markers x cameras.
//
// The residual blocks of /root/reference/Main_Calibration/bundle_adjustment.h:56-343 touch up to three 6-dof blocks:
// a camera transform, a marker transform and the pose of the base marker at one TIME.  Every residual block has
// exactly one time block, and no residual couples two times: given the cameras and markers the time blocks are
// mutually independent, the same structure the 3-D points have in the point model (and the reason Ceres' DENSE_SCHUR
// ordering would eliminate them first).  So the time blocks are eliminated,
//
//     S = U - sum_t W_t' (V_t + D_t)^-1 W_t        rhs = g_r - sum_t W_t' (V_t + D_t)^-1 g_t
//
// leaving a dense system over the (cameras + markers) only, which goes through the same Cholesky kernels as the
// reduced camera system of the point model, and the time steps come from back-substitution.  The one-workgroup dense
// solver of ba_marker_kernels.hpp stays for the committed 114-parameter data; this path takes over when the normal
// equations no longer fit it (rsba_options.schur_impl: 0 dense, 1 automatic, 2 always eliminate).
//
//   k_marker_eval        thread per residual block: r (8), J (8 x 18) by forward-mode duals      [ba_marker_kernels.hpp]
//   k_time_eliminate     workgroup per chunk of consecutive times, one time after the other: V, g, W and the reduced
//                        gradient from the staged Jacobians, E = (V + D)^-1, Y = E W, then every entry of the time's
//                        local block of U - W'Y is added to the workgroup's PRIVATE partial system (fixed order:
//                        bitwise reproducible, no atomics)
//   k_marker_reduce      thread per entry: the partial systems summed in chunk order, mirrored to full symmetric
//   k_marker_reduced_solve / k_sys_build + k_chol_step + k_marker_chol_finish     (n_r <= 384 / larger)
//   k_time_backsub_terms wavefront per time: delta_t = -E (g_t + W_t delta_r), candidate time pose, then the model cost
//                        change and the candidate's residuals of the time's residual blocks
//   k_marker_schur_finish   ordered final sums -> the 16-double result block
//
// Scaling and damping follow the point model's formulation: the elimination runs in unscaled coordinates with the
// effective damping D_t = clamp(s^2 V_ii) / (radius s^2), the Jacobi scale and the LM diagonal of the reduced blocks
// are applied by the Cholesky's panel loads (PanelSource).
#pragma once
#include <type_traits>

#include "ba_cholesky_large.hpp"
#include "ba_cholesky_tiles.hpp"
#include "ba_marker_kernels.hpp"
#include "ba_marker_plan.hpp"

namespace rsba {

// (RSBA_MT_TILE, RSBA_MT_MAXD, RSBA_MT_THREADS, RSBA_MT_JLD, PartLayout, TimeSlots: ba_marker_plan.hpp)
// (ablation hooks of the profiling builds: tools/ablate_marker.sh)
#ifndef RSBA_ABL_Q
#define RSBA_ABL_Q 8
#endif
#ifndef RSBA_ABL_SUMS
#define RSBA_ABL_SUMS 1
#endif
#ifndef RSBA_ABL_STAGE
#define RSBA_ABL_STAGE 1
#endif
#define RSBA_MT_PW (RSBA_MT_JLD + 8)   // doubles of a residual block's products (they take the place of its rows and residuals)

// LDS written by some lanes of a wavefront, read by others of the same wavefront.
#define RSBA_WAVE_LDS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// 6 x 6 SPD inverse through Cholesky on the first 36 lanes of a wavefront (all 64 call it): A (LDS, row-major, the lower
// triangle is read) -> E (LDS, both halves); Mx: 36 doubles of LDS scratch.  Every lane factors A (the same 21 entries of
// L), lane j < 6 inverts column j of L, lane e < 36 forms entry e of E = M'M: the operations of one thread doing all of
// it (sums padded with exact zeros), without the 200 registers that takes.  False (on every lane) when a pivot is not
// positive and finite.
__device__ inline bool InvertSpd6Lanes(int lane, const double* A, double* Mx, double* E) {
  double L[6][6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = A[j * 6 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    if (!(s > 0.0) || !(s <= DBL_MAX)) { ok = false; s = 1.0; }
    const double l = sqrt(s), inv = 1.0 / l;
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t * inv;
    }
  }
  {
    // column j = lane of M = L^-1: zeros above the diagonal
    const int j = lane;
    double m[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < i; ++k) t -= L[i][k] * m[k];
      m[i] = i < j ? 0.0 : (i == j ? 1.0 / L[i][i] : t / L[i][i]);
    }
    if (j < 6) {
#pragma unroll
      for (int i = 0; i < 6; ++i) Mx[i * 6 + j] = m[i];
    }
  }
  RSBA_WAVE_LDS_SYNC();
  if (lane < 36) {
    const int r = lane / 6, c = lane - 6 * r, hi = r > c ? r : c, lo = r > c ? c : r;
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) t += Mx[k * 6 + hi] * Mx[k * 6 + lo];
    E[lane] = t;
  }
  RSBA_WAVE_LDS_SYNC();
  return ok;
}

// Constants of every pose of the parameter array at the current linearisation (rotation matrix, left Jacobian of SO(3),
// translation, AngleAxisRotatePoint's branch): once per pose instead of once per corner of every residual block.
__global__ void __launch_bounds__(256) k_pose_constants(int nposes, const double* __restrict__ params, double* __restrict__ posec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nposes) return;
  const double zero4[4] = {0.0, 0.0, 0.0, 0.0};
  double cc[CC_STRIDE];
  CameraConstants(params + 6 * (size_t)i, zero4, cc);
#pragma unroll
  for (int q = 0; q < CC_STRIDE; ++q) posec[(size_t)i * CC_STRIDE + q] = cc[q];
}

struct ElimArgs {
  int nr, dmax, nblocks;
  const int* __restrict__ chunk_ptr;   // [G + 1] times of each workgroup
  const int* __restrict__ time_ptr;    // [T + 1] residual blocks of each time
  const int* __restrict__ slot_ptr;    // [T + 1] slots (distinct camera / marker blocks) of each time
  const int* __restrict__ slot_col;    // first reduced column of each slot, ascending inside a time
  const int* __restrict__ time_full;   // offset of the time block in the full parameter array
  const int* __restrict__ col_full;    // reduced column -> index in the full parameter array
  const TimeSlots* __restrict__ ts;
  // the residual blocks' Jacobians are NOT stored: every tile of 32 blocks is evaluated where it is used, analytically
  // (MarkerCornerResidualJacobian, ba_math.hpp) from the poses' constants of this linearisation
  const MarkerObs* __restrict__ mo;    // [N]
  const double* __restrict__ obs8;     // [N][8]
  const double* __restrict__ intr;     // [C][4]
  const double* __restrict__ posec;    // [poses][CC_STRIDE]: R, left Jacobian, t, branch flag of every pose at x (k_pose_constants)
  double half_side;
  const double* __restrict__ params_x;
  double* __restrict__ scale_t;        // [6 T]
  double* __restrict__ tdata;          // [T][48]: E (36), g_t (6)
  double* __restrict__ part;           // [G][RedLayout(nr).size()]; S lower triangle only
  IterParams ip;
  // kConst instances only: the times' pose-only slots (full offsets of their constant camera / marker blocks) and constant flags
  const int* __restrict__ cs_ptr;      // [T + 1]
  const int* __restrict__ cs_full;
  const int* __restrict__ tconst;      // [T]
  int pmax;                            // the widest pose cache (free + pose-only slots); dmax stays the widest free part
};
// the kDist instances' argument: the same and the cameras' distortion coefficients [C][5], indexed as intr
struct ElimArgsDist : ElimArgs { const double* __restrict__ dist; };
template <bool kDist> struct ElimArgT { typedef ElimArgs type; };
template <> struct ElimArgT<true> { typedef ElimArgsDist type; };
__device__ __forceinline__ const double* DistOf(const ElimArgs&, int) { return nullptr; }
__device__ __forceinline__ const double* DistOf(const ElimArgsDist& a, int camera) { return a.dist + 5 * camera; }

#ifdef RSBA_PROFILE_PHASES
__device__ long long g_mt_cycles[16];
#define RSBA_MT_STAMP(k) do { __syncthreads(); if (blockIdx.x == 0 && threadIdx.x == 0) { long long _t = clock64(); g_mt_cycles[k] += _t - _t0; _t0 = _t; } } while (0)
#else
#define RSBA_MT_STAMP(k) do {} while (0)
#endif

// Workgroup barrier that orders LDS only: the staging lanes' loads from HBM for the next tile stay in flight across it.
#define RSBA_MT_BARRIER() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); } while (0)

__device__ __forceinline__ int LocalColumn(int slot, int q, int sc, int sm) { return slot == sc ? q : (slot == sm ? 12 + q : -1); }

// Constant camera / marker blocks have no column but their transform is applied: a time's constant blocks get pose-only slots
// behind its nslot free ones (slot -2 - j in TimeSlots -> pose-cache entry nslot + j, ConstSlotPose).  A time's constant flag
// eliminates it with E = 0 (infinitely stiff): no step, no W'EW, its rows still add U and g_r.
__device__ __forceinline__ int ConstSlotPose(int slot, int nslot) { return nslot - 2 - slot; }

template <bool kLdsS, bool kConst = false, bool kDist = false>
__global__ void __launch_bounds__(RSBA_MT_THREADS)
k_time_eliminate(typename ElimArgT<kDist>::type a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, nr = a.nr, dmax = a.dmax;
  const PartLayout RL{nr};
  double* W = lds;                        // [6][d]
  double* Y = W + 6 * dmax;               // [6][d]
  double* Gr = Y + 6 * dmax;              // [d]
  double* Vs = Gr + dmax;                 // V 36 | g 6 | (pad 6) | E 36 | Eg 6
  double* Jt = Vs + 96;                   // [TILE][145]: odd stride, the lanes of pass 2 read different residual blocks
  double* rt = Jt + RSBA_MT_TILE * RSBA_MT_JLD;   // [TILE][8]
  double* sqv = rt + RSBA_MT_TILE * 8;    // [TILE] squared residual norms
  double* PA = Jt;                        // [TILE][153] a residual block's products, in the place of its rows and residuals once those are read
  int* sl = (int*)(sqv + RSBA_MT_TILE);   // [TILE][2] slots, then per slot of the time [dmax / 6 + 1] each:
  int* scol = sl + 2 * RSBA_MT_TILE;      //   first reduced column
  int* mk = scol + dmax / 6 + 1;          //   bit i: staged residual block i has the slot
  int* kb = mk + dmax / 6 + 1;            //   where the slot's block sits in a residual's Jacobian: column 0 (camera) or 12 (marker)
  // the chunk's sum of S (packed lower triangle) and of the three vectors: in LDS when they fit, else straight in the workgroup's partial system
  // pose constants of the current time: the time pose, then one per slot (camera / marker block of the time)
  double* pcl = (double*)(sl + ((2 * RSBA_MT_TILE + 3 * (dmax / 6 + 1) + 1) & ~1));   // [dmax / 6 + 2][CC_STRIDE] (kConst: pmax + 2)
  double* Sl = pcl + (size_t)((kConst ? a.pmax : dmax / 6) + 2) * CC_STRIDE;
  double* P = a.part + (size_t)blockIdx.x * RL.size();
  double* Sacc = kLdsS ? Sl : P + RL.S();
  const size_t nacc = RL.packed() + 3 * (size_t)nr;   // S, then the three vectors behind it (PartLayout): all of them in LDS or none
  for (size_t e = tid; e < nacc; e += RSBA_MT_THREADS) Sacc[e] = 0.0;
  for (size_t e = nacc + tid; e < RL.size(); e += RSBA_MT_THREADS) P[e] = 0.0;
  double cost = 0.0, xn2 = 0.0, gmax = 0.0, fail = 0.0;   // thread 0's running sums over the chunk's times
#ifdef RSBA_PROFILE_PHASES
  long long _t0 = clock64();
#endif
  __threadfence_block();
  __syncthreads();

  // staging lanes: part (camera, time, marker block of the rows) x residual block of the tile x corner
  const int sp = tid >> 7, sb_i = (tid & 127) >> 2, sk = tid & 3;
  int nsc = -1, nsm = -1, ncam = 0;
  double nu = 0.0, nv = 0.0;
  auto fetch = [&](int first) {   // what the lane needs of the tile that starts at residual block first
    const int i = min(first + sb_i, a.nblocks - 1);
    nsc = a.ts[i].slot_cam; nsm = a.ts[i].slot_marker; ncam = a.ts[i].camera;
    nu = a.obs8[8 * (size_t)i + 2 * sk]; nv = a.obs8[8 * (size_t)i + 2 * sk + 1];
  };
  if (tid < 3 * 4 * RSBA_MT_TILE) fetch(a.time_ptr[a.chunk_ptr[blockIdx.x]]);
  RSBA_MT_STAMP(0);
  for (int t = a.chunk_ptr[blockIdx.x]; t < a.chunk_ptr[blockIdx.x + 1]; ++t) {
    const int o0 = a.time_ptr[t], nobs = a.time_ptr[t + 1] - o0;
    const int s0 = a.slot_ptr[t], nslot = a.slot_ptr[t + 1] - s0, d = 6 * nslot;
    // the time's Jacobi scale and parameters, wanted after pass 1
    double pre_scale = 1.0, pre_x = 0.0;
    if (tid < 6) { if (!a.ip.first) pre_scale = a.scale_t[6 * t + tid]; pre_x = a.params_x[a.time_full[t] + tid]; }
    for (int e = tid; e < 6 * d; e += RSBA_MT_THREADS) W[e] = 0.0;
    for (int e = tid; e < d; e += RSBA_MT_THREADS) Gr[e] = 0.0;
    if (tid < 43) Vs[tid] = 0.0;
    for (int e = tid; e < nslot; e += RSBA_MT_THREADS) scol[e] = a.slot_col[s0 + e];
    if constexpr (kConst) {
      const int c0 = a.cs_ptr[t], npose = nslot + a.cs_ptr[t + 1] - c0;
      for (int e = tid; e < (npose + 1) * CC_STRIDE; e += RSBA_MT_THREADS) {
        const int ps = e / CC_STRIDE, q = e - ps * CC_STRIDE;
        const int pose = (ps == 0 ? a.time_full[t] : (ps <= nslot ? a.col_full[a.slot_col[s0 + ps - 1]] : a.cs_full[c0 + ps - 1 - nslot])) / 6;
        pcl[e] = a.posec[(size_t)pose * CC_STRIDE + q];
      }
    } else {
      for (int e = tid; e < (nslot + 1) * CC_STRIDE; e += RSBA_MT_THREADS) {
        const int ps = e / CC_STRIDE, q = e - ps * CC_STRIDE;
        const int pose = (ps == 0 ? a.time_full[t] : a.col_full[a.slot_col[s0 + ps - 1]]) / 6;
        pcl[e] = a.posec[(size_t)pose * CC_STRIDE + q];
      }
    }
    const int ntile = (nobs + RSBA_MT_TILE - 1) / RSBA_MT_TILE;
    auto stage = [&](int tile) {
      const int b0 = o0 + tile * RSBA_MT_TILE, nb = min(RSBA_MT_TILE, nobs - tile * RSBA_MT_TILE);
      RSBA_MT_BARRIER();   // the previous tile has been consumed
      if (tid < 3 * 4 * RSBA_MT_TILE) {
        // one corner of one residual block per three lanes: the residuals (2) and one 2 x 6 block of the Jacobian rows each
        // (the rows go straight into the staged tile; the poses' constants come from LDS, staged once per time).  What the
        // lane read from HBM was fetched a tile ago; the next tile's (of this time or the first of the next: the residual
        // blocks are in time order) is on its way while this one is consumed.
        const int slot_cam = nsc, slot_marker = nsm;
        const double* in = a.intr + 4 * ncam;   // a handful of cameras per chunk: from the L1
        const double u = nu, v = nv, fx = in[0], fy = in[1], ppx = in[2], ppy = in[3];
        const double* ds = DistOf(a, ncam);
        fetch(b0 + nb);
        if (sb_i < RSBA_ABL_STAGE * nb) {
          const double hs = a.half_side;
          const double cx = (sk == 0 || sk == 3) ? -hs : hs, cy = sk < 2 ? hs : -hs;
          auto pose_of = [&](int slot) -> const double* {
            if (slot >= 0) return pcl + (size_t)(1 + slot) * CC_STRIDE;
            if (kConst && slot <= -2) return pcl + (size_t)(1 + ConstSlotPose(slot, nslot)) * CC_STRIDE;
            return nullptr;
          };
          MarkerCornerJacobianPart<kDist>(sp, pose_of(slot_cam), pcl, pose_of(slot_marker),
                                          fx, fy, ppx, ppy, cx, cy, u, v, rt + sb_i * 8 + 2 * sk, Jt + sb_i * RSBA_MT_JLD + 36 * sk, ds);
          if (sp == 0 && sk == 0) { sl[2 * sb_i] = slot_cam; sl[2 * sb_i + 1] = slot_marker; }
        }
      }
      for (int e = tid; e < nslot; e += RSBA_MT_THREADS) mk[e] = 0;
      RSBA_MT_BARRIER();
      // the last wavefront (the products below keep the first fifteen busy), no barrier: wanted by the sums, two barriers on
      const int mt = tid - (RSBA_MT_THREADS - 64);
      if (mt >= 0 && mt < nb) {   // squared residual norm of a block, corner by corner (before the products take the residuals' place)
        double ss = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) ss += rt[mt * 8 + 2 * k] * rt[mt * 8 + 2 * k] + rt[mt * 8 + 2 * k + 1] * rt[mt * 8 + 2 * k + 1];
        sqv[mt] = ss;
        // which staged residual blocks belong to a slot (bit order = block order: the sums below run in a fixed order)
        const int sc = sl[2 * mt], sm = sl[2 * mt + 1];
        if (sc >= 0) { atomicOr(&mk[sc], 1 << mt); kb[sc] = 0; }
        if (sm >= 0) { atomicOr(&mk[sm], 1 << mt); kb[sm] = 12; }
      }
      return nb;
    };
    RSBA_MT_STAMP(1);
    // ---- pass 1 (the only one over the Jacobians): V, g_t, W = J_t' J_r, reduced gradient, U
    for (int tile = 0; tile < ntile; ++tile) {
      const int nb = stage(tile);
      RSBA_MT_STAMP(8);
      // Products of a residual block's rows J_i (8 x 18: camera, time, marker block), a column per lane: with the time block (J_t' J_side = a block of W, or
      // V), with the residuals (reduced gradient, g_t), with the lane's own block (U's diagonal blocks), marker with camera
      // (U's cross block: every (time, camera, marker) occurs once, so it goes straight into the sum).  The rows are read
      // once per residual block here, not once per entry of the sums; the products then take the rows' place in LDS.
      // Five roles of 192 lanes (three wavefronts each, so a role's branch is uniform): 0 camera columns x time block + gradient,
      // 1 time columns (V, g_t), 2 marker columns x time block + gradient + cross block, 3 camera block x itself, 4 marker block x itself.
      double pt[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, pg = 0.0;   // (roles 3, 4: pt holds the block's own products)
      const int p_role = tid / (6 * RSBA_MT_TILE), p_in = tid - p_role * 6 * RSBA_MT_TILE, p_i = p_in / 6, p_c = p_in - 6 * p_i;
      const int p_sd = p_role == 1 ? 1 : ((p_role == 0 || p_role == 3) ? 0 : 2);
      const bool p_on = p_role < 5 && p_i < nb && (p_sd == 1 || sl[2 * p_i + (p_sd >> 1)] >= 0);
      if (p_on) {
        // row by row (q): the accumulators are what stays live, not a hundred loads
        double px[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double* Jq = Jt + p_i * RSBA_MT_JLD;
        const double* ri = rt + p_i * 8;
        const int other = p_role >= 3 ? 6 * p_sd : 6;   // the block the lane's column is multiplied with
#pragma unroll 2
        for (int q = 0; q < RSBA_ABL_Q; ++q, Jq += 18) {
          const double own = Jq[6 * p_sd + p_c];
#pragma unroll
          for (int x = 0; x < 6; ++x) pt[x] = fma(Jq[other + x], own, pt[x]);
          if (p_role < 3) pg = fma(own, ri[q], pg);
          if (p_role == 2) {
#pragma unroll
            for (int cq = 0; cq < 6; ++cq) px[cq] = fma(own, Jq[cq], px[cq]);
          }
        }
        if (p_role == 2 && sl[2 * p_i] >= 0) {
          const int gr = scol[sl[2 * p_i + 1]] + p_c, gc = scol[sl[2 * p_i]];
#pragma unroll
          for (int cq = 0; cq < 6; ++cq) Sacc[(size_t)gr * (gr + 1) / 2 + gc + cq] += px[cq];
        }
      }
      RSBA_MT_BARRIER();   // the rows have been read
      if (p_on) {
        // per residual block (stride RSBA_MT_PW): camera W, g (42) | marker W, g (42) | camera U (21) | marker U (21) | V (21) | g_t (6);
        // the symmetric blocks as lower triangles (row r >= column c at r (r + 1) / 2 + c)
        double* out = PA + p_i * RSBA_MT_PW;
        if (p_role == 0 || p_role == 2) {
          double* o1 = out + 42 * (p_sd >> 1) + p_c;
#pragma unroll
          for (int x = 0; x < 6; ++x) o1[6 * x] = pt[x];
          o1[36] = pg;
        } else if (p_role >= 3) {
          double* o2 = out + 84 + 21 * (p_sd >> 1);
#pragma unroll
          for (int r = 0; r < 6; ++r) if (r >= p_c) o2[r * (r + 1) / 2 + p_c] = pt[r];
        } else {
#pragma unroll
          for (int x = 0; x < 6; ++x) if (x >= p_c) out[126 + x * (x + 1) / 2 + p_c] = pt[x];
          out[147 + p_c] = pg;
        }
      }
      RSBA_MT_BARRIER();
      RSBA_MT_STAMP(9);
      // W = J_t' J_r (row x of the time block, reduced column col) and the reduced gradient (x = 6): the products of the
      // slot's residual blocks in block order
      for (int e = tid; e < RSBA_ABL_SUMS * 7 * d; e += RSBA_MT_THREADS) {
        const int x = e / d, col = e - x * d, s = col / 6;
        const double* pw = PA + (kb[s] ? 42 : 0) + 6 * x + (col - 6 * s);
        double acc = 0.0;
        for (unsigned m = (unsigned)mk[s]; m; m &= m - 1) acc += pw[(__ffs(m) - 1) * RSBA_MT_PW];
        if (x < 6) W[e] += acc; else Gr[col] += acc;
      }
      // U: a diagonal block per slot, the sum over the slot's residual blocks in block order (cameras have the lower
      // columns; two different cameras (or markers) never meet in a residual)
      for (int e = tid; e < RSBA_ABL_SUMS * nslot * 21; e += RSBA_MT_THREADS) {
        const int sidx = e / 21, tri = e - 21 * sidx;
        int rq = (int)((sqrtf(8.0f * (float)tri + 1.0f) - 1.0f) * 0.5f);
        while (rq * (rq + 1) / 2 > tri) --rq;
        while ((rq + 1) * (rq + 2) / 2 <= tri) ++rq;
        const int cq = tri - rq * (rq + 1) / 2;
        const double* pw = PA + 84 + (kb[sidx] ? 21 : 0) + tri;
        double u = 0.0;
        for (unsigned m = (unsigned)mk[sidx]; m; m &= m - 1) u += pw[(__ffs(m) - 1) * RSBA_MT_PW];
        const int gr = scol[sidx] + rq, gc = scol[sidx] + cq;
        if (rq == cq) Sacc[RL.diagU() + gr] += u;
        Sacc[(size_t)gr * (gr + 1) / 2 + gc] += u;
      }
      // V (21, mirrored), g_t (6), cost (1): every staged residual block contributes; eight lanes per entry take every
      // eighth block, a fixed shuffle tree adds them
      {
        const int t2 = tid - (RSBA_MT_THREADS - 28 * 8);   // the last waves: the first ones have the longest sums above
        if (t2 >= 0) {
          const int ent = t2 >> 3, k = t2 & 7;
          double acc = 0.0;
          if (ent < 27) { for (int i = k; i < nb; i += 8) acc += PA[i * RSBA_MT_PW + 126 + ent]; }
          else { for (int i = k; i < nb; i += 8) acc += sqv[i]; }
          acc += __shfl_xor(acc, 1, 64); acc += __shfl_xor(acc, 2, 64); acc += __shfl_xor(acc, 4, 64);
          if (k == 0) {
            if (ent < 21) {
              int x = (int)((sqrtf(8.0f * (float)ent + 1.0f) - 1.0f) * 0.5f);
              while (x * (x + 1) / 2 > ent) --x;
              while ((x + 1) * (x + 2) / 2 <= ent) ++x;
              const int y = ent - x * (x + 1) / 2;
              Vs[6 * x + y] += acc;
              if (x != y) Vs[6 * y + x] += acc;
            } else if (ent < 27) Vs[36 + ent - 21] += acc;
            else Vs[42] += acc;
          }
        }
      }
      RSBA_MT_STAMP(10);
    }
    __syncthreads();
    RSBA_MT_STAMP(2);
    // ---- E = (V + D)^-1, E g_t: the first wavefront (the residual blocks' products are dead: the damped block and the inverse's scratch)
    const bool tcon = kConst && a.tconst[t] != 0;
    if (kConst && tcon) {
      // a constant time: E = 0, E g_t = 0 (so Y = 0 and no correction below); only its cost counts
      if (tid < 36) { Vs[48 + tid] = 0.0; a.tdata[(size_t)t * 48 + tid] = 0.0; }
      if (tid < 6) { Vs[84 + tid] = 0.0; a.tdata[(size_t)t * 48 + 36 + tid] = Vs[36 + tid]; }
      cost += Vs[42];
    } else if (tid < 64) {
      double* Vd = PA + 36;
      double sc = 1.0;
      if (tid < 6) {
        if (a.ip.first) { sc = a.ip.jacobi_scaling ? 1.0 / (1.0 + sqrt(Vs[7 * tid])) : 1.0; a.scale_t[6 * t + tid] = sc; }
        else sc = pre_scale;
      }
      const double s2 = sc * sc;
      const double dd = tid < 6 ? fmin(fmax(s2 * Vs[7 * tid], a.ip.min_lm_diagonal), a.ip.max_lm_diagonal) / (a.ip.radius * s2) : 0.0;
      {
        const int x = tid < 36 ? tid / 6 : 0, y = tid - 6 * x;
        const double dx = __shfl(dd, x, 64);
        if (tid < 36) Vd[tid] = x == y ? Vs[tid] + dx : Vs[tid];
      }
#pragma unroll
      for (int x = 0; x < 6; ++x) {
        const double xv = __shfl(pre_x, x, 64);
        gmax = fmax(gmax, fabs(Vs[36 + x]));
        xn2 += xv * xv;
      }
      RSBA_WAVE_LDS_SYNC();
      if (!InvertSpd6Lanes(tid, Vd, PA, Vs + 48)) fail += 1.0;
      if (tid < 36) a.tdata[(size_t)t * 48 + tid] = Vs[48 + tid];
      if (tid < 6) {
        double e = 0.0;
#pragma unroll
        for (int y = 0; y < 6; ++y) e += Vs[48 + 6 * tid + y] * Vs[36 + y];
        Vs[84 + tid] = e;
        a.tdata[(size_t)t * 48 + 36 + tid] = Vs[36 + tid];
      }
      cost += Vs[42];
    }
    __syncthreads();
    RSBA_MT_STAMP(3);
    for (int e = tid; e < 6 * d; e += RSBA_MT_THREADS) {
      const int x = e / d, col = e - x * d;
      double s = 0.0;
#pragma unroll
      for (int y = 0; y < 6; ++y) s += Vs[48 + 6 * x + y] * W[y * d + col];
      Y[e] = s;
    }
    __syncthreads();
    RSBA_MT_STAMP(4);
    // ---- pass 2: minus W'Y, the dense part of the time's block.  One item = a row of a 6 x 6 block (rs, cs <= rs):
    // lower triangle only (slots ascend, so does the reduced column), six outputs per six + 36 loads
    {
      const int nbp = nslot * (nslot + 1) / 2;
      for (int it = tid; it < 6 * nbp; it += RSBA_MT_THREADS) {
        const int bp = it / 6, rq = it - 6 * bp;
        int rs = (int)((sqrtf(8.0f * (float)bp + 1.0f) - 1.0f) * 0.5f);
        while (rs * (rs + 1) / 2 > bp) --rs;
        while ((rs + 1) * (rs + 2) / 2 <= bp) ++rs;
        const int cs = bp - rs * (rs + 1) / 2;
        double wr[6];
#pragma unroll
        for (int x = 0; x < 6; ++x) wr[x] = W[x * d + 6 * rs + rq];
        const int gr = scol[rs] + rq;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          if (rs == cs && c > rq) continue;
          double wy = 0.0;
#pragma unroll
          for (int x = 0; x < 6; ++x) wy += wr[x] * Y[x * d + 6 * cs + c];
          Sacc[(size_t)gr * (gr + 1) / 2 + scol[cs] + c] -= wy;
        }
      }
    }
    RSBA_MT_STAMP(5);
    for (int e = tid; e < d; e += RSBA_MT_THREADS) {
      const int s = e / 6, gcol = scol[s] + (e - 6 * s);
      double c = 0.0;
#pragma unroll
      for (int x = 0; x < 6; ++x) c += W[x * d + e] * Vs[84 + x];
      Sacc[RL.gc() + gcol] += Gr[e];
      Sacc[RL.corr() + gcol] -= c;
    }
    __threadfence_block();
    __syncthreads();
    RSBA_MT_STAMP(6);
  }
  if (kLdsS) for (size_t e = tid; e < nacc; e += RSBA_MT_THREADS) P[e] = Sl[e];
  if (tid == 0) { P[RL.scal() + 0] = cost; P[RL.scal() + 1] = xn2; P[RL.scal() + 2] = fail; P[RL.scal() + 3] = gmax; }
}

// Partial systems -> red (full symmetric S | gc | corr | diagU | scal), chunk order.
// A workgroup takes 64 consecutive entries of the PACKED partial systems, wavefront k the chunks g = k (mod 8) in ascending
// order, eight loads in flight: every load of a wavefront is 512 contiguous bytes of one partial system (the round-3 form read
// the packed triangle twice — once per half of the full square it writes — with eight partial systems per load instruction:
// 29 us for 20 MB).  The eight wavefronts' sums meet in LDS in the order the eight lanes' did: ((0+1)+(2+3))+((4+5)+(6+7)) — the
// same bits.  An entry of the triangle is written to both halves of S.
__global__ void __launch_bounds__(512)
k_marker_reduce(int nr, int G, const double* __restrict__ part, double* __restrict__ red) {
  const RedLayout RL{nr};
  const PartLayout PL{nr};
  __shared__ double s_w[8][64];
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  const size_t src = (size_t)blockIdx.x * 64 + lane;
  const bool live = src < PL.size();
  const bool is_max = src == PL.scal() + 3;
  double s = 0.0;
  if (live) {
    int g = k;
    for (; g + 56 < G; g += 64) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(g + 8 * u) * PL.size() + src];
#pragma unroll
      for (int u = 0; u < 8; ++u) s = is_max ? fmax(s, v[u]) : s + v[u];
    }
    for (; g < G; g += 8) { const double v = part[(size_t)g * PL.size() + src]; s = is_max ? fmax(s, v) : s + v; }
  }
  s_w[k][lane] = s;
  __syncthreads();
  if (k != 0 || !live) return;
  auto add = [&](double x, double y) { return is_max ? fmax(x, y) : x + y; };
  const double t = add(add(add(s_w[0][lane], s_w[1][lane]), add(s_w[2][lane], s_w[3][lane])), add(add(s_w[4][lane], s_w[5][lane]), add(s_w[6][lane], s_w[7][lane])));
  if (src < PL.packed()) {
    size_t i = (size_t)((sqrt(8.0 * (double)src + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > src) --i;
    while ((i + 1) * (i + 2) / 2 <= src) ++i;
    const size_t j = src - i * (i + 1) / 2;
    red[i * nr + j] = t;
    red[j * nr + i] = t;
  } else {
    red[(size_t)nr * nr + (src - PL.packed())] = t;
  }
}

// Step of the reduced blocks from the solution y of the scaled system; candidate parameters; norms.
//   out[0..4] = |delta_r|^2, |x_r|^2, |x_r + delta_r|^2, max |g_r|, factorisation ok
__device__ __forceinline__ void ReducedStepEpilogue(int nr, const double* __restrict__ red, RedLayout RL, const double* __restrict__ scale_r,
                                                    const double* __restrict__ ysol, const int* __restrict__ col_full,
                                                    const double* __restrict__ params_x, double* __restrict__ params_c,
                                                    double* __restrict__ delta_r, double* __restrict__ out, int ok, double* scr) {
  const int tid = threadIdx.x, nt = blockDim.x;
  double d2 = 0, x2 = 0, xc2 = 0, gm = 0;
  for (int i = tid; i < nr; i += nt) {
    const double dd = -scale_r[i] * ysol[i];
    delta_r[i] = dd;
    const double x = params_x[col_full[i]], xc = x + dd;
    params_c[col_full[i]] = xc;
    d2 += dd * dd; x2 += x * x; xc2 += xc * xc; gm = fmax(gm, fabs(red[RL.gc() + i]));
  }
  __syncthreads();
  scr[tid] = d2; scr[nt + tid] = x2; scr[2 * nt + tid] = xc2; scr[3 * nt + tid] = gm;
  __syncthreads();
  for (int off = nt / 2; off > 0; off >>= 1) {
    if (tid < off) {
      scr[tid] += scr[tid + off]; scr[nt + tid] += scr[nt + tid + off]; scr[2 * nt + tid] += scr[2 * nt + tid + off];
      scr[3 * nt + tid] = fmax(scr[3 * nt + tid], scr[3 * nt + tid + off]);
    }
    __syncthreads();
  }
  if (tid == 0) { out[0] = scr[0]; out[1] = scr[nt]; out[2] = scr[2 * nt]; out[3] = scr[3 * nt]; out[4] = ok ? 1.0 : 0.0; }
}

__global__ void __launch_bounds__(512)
k_marker_reduced_solve(int nr, const double* __restrict__ red, double* __restrict__ A, double* __restrict__ scale_r,
                       const int* __restrict__ col_full, const double* __restrict__ params_x, double* __restrict__ params_c,
                       double* __restrict__ delta_r, double* __restrict__ out, IterParams ip) {
  extern __shared__ double lds[];
  const RedLayout RL{nr};
  const int tid = threadIdx.x, nt = blockDim.x;
  __shared__ int s_ok;
  for (int i = tid; i < nr; i += nt)
    if (ip.first) scale_r[i] = ip.jacobi_scaling ? 1.0 / (1.0 + sqrt(red[RL.diagU() + i])) : 1.0;
  __threadfence_block();
  __syncthreads();
  for (int i = tid; i < nr; i += nt) A[(size_t)nr * nr + i] = scale_r[i] * (red[RL.gc() + i] + red[RL.corr() + i]);
  __threadfence_block();
  __syncthreads();
  double* ysol = A + (size_t)nr * nr;
  CholeskySolvePanelLDS(nr, A, ysol, &s_ok, lds,
                        PanelSource{red + RL.S(), scale_r, red + RL.diagU(), ip.min_lm_diagonal, ip.max_lm_diagonal, 1.0 / ip.radius, nullptr, nullptr, 0},
                        StageGate{nullptr, 0, 0, nullptr, nullptr, nullptr, 0});
  __syncthreads();
  ReducedStepEpilogue(nr, red, RL, scale_r, ysol, col_full, params_x, params_c, delta_r, out, s_ok > 0, lds);
}

// k_marker_reduced_solve for systems of up to 160 columns (26 camera + marker blocks: the 8 x 5000 x 16 benchmark has 132) with the WHOLE
// lower triangle in LDS.  CholeskySolvePanelLDS keeps a panel there and the matrix in memory: per 32-column panel the panel comes
// in, the strip of L to its left comes in, the panel goes back out — three dependent trips to memory around 7 us of factorisation,
// 12 us a panel, 77 us for the five of 132 columns (a quarter of the iteration once the elimination was split, ba_marker_split.hpp).
// Here the lower triangle lies in LDS as five column panels of 33-double rows (the right-hand side rides along as every panel's last
// row; padding columns are identity), loaded once; right-looking: per panel DiagFactorInverse (one wavefront), X = rows T' and the
// trailing panels' updates on the matrix cores, T kept where L_pp was; then L' x = y from LDS.  Nothing goes to memory but x.
// Same scaling and damping as PanelSource's (ba_cholesky.hpp); fixed orders: bitwise reproducible.
// (RSBA_MRS_MAXP, its five panels, and MarkerSolveLdsDoubles, its LDS: ba_marker_plan.hpp)
__global__ void __launch_bounds__(512)
k_marker_reduced_solve_lds(int nr, const double* __restrict__ red, double* __restrict__ A, double* __restrict__ scale_r,
                           const int* __restrict__ col_full, const double* __restrict__ params_x, double* __restrict__ params_c,
                           double* __restrict__ delta_r, double* __restrict__ out, IterParams ip) {
  extern __shared__ double lds[];
  const RedLayout RL{nr};
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = nt >> 6, mi = lane & 15, kk = lane >> 4;
  const int np = (nr + RSBA_PB - 1) / RSBA_PB, npad = RSBA_PB * np;
  __shared__ int s_ok;
  __shared__ double s_red[8][4];
  int poff[RSBA_MRS_MAXP + 1];   // panel p: rows 32 p .. npad (the right-hand side) of its 32 columns
  poff[0] = 0;
#pragma unroll
  for (int p = 0; p < RSBA_MRS_MAXP; ++p) poff[p + 1] = poff[p] + (npad + 1 - RSBA_PB * p) * RSBA_PLD;
  double* T = lds + poff[np];
  double* Lt = T + RSBA_PB * RSBA_PLD;
  double* invd = Lt + RSBA_PB * RSBA_PLD;
  double* scl = invd + RSBA_PB;        // npad
  double* yv = scl + npad;             // npad: the damping diagonal while the panels are filled, then y, then x
  double* tmp32 = invd;                // (the back-substitution's 32 doubles: the inverse pivots are done with by then)
  if (tid == 0) s_ok = 1;
  // ---- everything the kernel reads from memory, asked for in ONE go: the thread's entry of the vectors (nr <= 160 < 512: one each),
  // then its entries of S — element e = tid + 512 u of panel p's (rows x 32) block, at most eleven a panel.  (Entry by entry under
  // their branches the loads were 30 dependent trips to memory a thread: 15 us of the kernel's 78.)
  const bool mine = tid < nr;
  const double my_du = mine ? red[RL.diagU() + tid] : 0.0, my_gc = mine ? red[RL.gc() + tid] : 0.0, my_corr = mine ? red[RL.corr() + tid] : 0.0;
  const double my_sc_old = (mine && !ip.first) ? scale_r[tid] : 1.0;
  const int my_cf = mine ? col_full[tid] : 0;
  constexpr int kMaxE = (RSBA_PB * RSBA_MRS_MAXP + 1 + 15) / 16;   // 11
  double sv[RSBA_MRS_MAXP][kMaxE];
#pragma unroll
  for (int p = 0; p < RSBA_MRS_MAXP; ++p) {
#pragma unroll
    for (int u = 0; u < kMaxE; ++u) {
      sv[p][u] = 0.0;
      if (u < kMaxE - 2 * p) {   // (panel p has 161 - 32 p rows at most: 11, 9, 7, 5, 3 elements a thread)
        const int kb = RSBA_PB * p, e = tid + u * nt, gi = kb + (e >> 5), gj = kb + (e & 31);
        if (p < np && gi < nr && gj < nr) sv[p][u] = red[RL.S() + (size_t)gi * nr + gj];
      }
    }
  }
  const double my_x = mine ? params_x[my_cf] : 0.0;
  if (tid < npad) {
    double sc = 1.0;
    if (mine) { sc = ip.first ? (ip.jacobi_scaling ? 1.0 / (1.0 + sqrt(my_du)) : 1.0) : my_sc_old; if (ip.first) scale_r[tid] = sc; }
    scl[tid] = sc;
    yv[tid] = my_du;
  }
  __syncthreads();
  const double inv_radius = 1.0 / ip.radius;
#pragma unroll
  for (int p = 0; p < RSBA_MRS_MAXP; ++p) {
    if (p < np) {
      const int kb = RSBA_PB * p, R = npad + 1 - kb;
      double* Pan = lds + poff[p];
#pragma unroll
      for (int u = 0; u < kMaxE; ++u) {
        const int e = tid + u * nt;
        if (u < kMaxE - 2 * p && e < R * RSBA_PB) {
          const int r = e >> 5, c = e & 31, gi = kb + r, gj = kb + c;
          double v;
          if (gi == npad) v = 0.0;   // (the right-hand side: below)
          else if (gi >= nr || gj >= nr) v = gi == gj ? 1.0 : 0.0;
          else {
            v = sv[p][u] * (scl[gi] * scl[gj]);
            if (gi == gj) v += fmin(fmax(scl[gi] * scl[gi] * yv[gi], ip.min_lm_diagonal), ip.max_lm_diagonal) * inv_radius;
          }
          Pan[r * RSBA_PLD + c] = v;
        }
      }
    }
  }
  __syncthreads();   // (the damping diagonal in yv has been read)
  if (mine) { const int p = tid >> 5; (lds + poff[p])[(npad - RSBA_PB * p) * RSBA_PLD + (tid & 31)] = scl[tid] * (my_gc + my_corr); }   // s_j (g_j + corr_j): the panel's last row
  __syncthreads();
#pragma unroll
  for (int p = 0; p < RSBA_MRS_MAXP; ++p) {
    if (p >= np) break;
    const int R = npad + 1 - RSBA_PB * p;   // rows of the panel, the right-hand side's included
    double* Pan = lds + poff[p];
    if (wave == 0 && !DiagFactorInverseCall((lds_double*)Pan, RSBA_PB, (lds_double*)T, (lds_double*)Lt, (lds_double*)invd, lane) && lane == 0) s_ok = 0;
    __syncthreads();
    // X = rows T' for the rows below the diagonal block (CholeskySolvePanelLDS, step 4)
    {
      const int nrb = (R - RSBA_PB + 15) >> 4;
      for (int rb = wave; rb < nrb; rb += nwave) {
        const int prow = RSBA_PB + rb * 16 + mi;
        d4_t acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
        for (int qs = 0; qs < RSBA_PB; qs += 4) {
          const double a = prow < R ? Pan[prow * RSBA_PLD + qs + kk] : 0.0;
          acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, T[mi * RSBA_PLD + qs + kk], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, T[(16 + mi) * RSBA_PLD + qs + kk], acc1, 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();   // all of this block's rows are read before any is overwritten
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const int r = RSBA_PB + rb * 16 + kk + 4 * tt;
          if (r < R) { Pan[r * RSBA_PLD + mi] = acc0[tt]; Pan[r * RSBA_PLD + 16 + mi] = acc1[tt]; }
        }
      }
    }
    __syncthreads();
    // T_p takes L_pp's place (the back-substitution wants T_p and the blocks below; L_pp itself is done with)
    for (int e = tid; e < RSBA_PB * RSBA_PB; e += nt) Pan[(e >> 5) * RSBA_PLD + (e & 31)] = T[(e >> 5) * RSBA_PLD + (e & 31)];
    // the trailing panels: (i, j) -= sum_k L(i, k) L(j, k) over this panel's columns k — 16 x 16 tiles, both operands from this panel
    {
      int tile0 = 0;
#pragma unroll
      for (int q = 1; q < RSBA_MRS_MAXP; ++q) {
        if (q <= p || q >= np) continue;
        const int Rq = npad + 1 - RSBA_PB * q, nrt = (Rq + 15) >> 4;     // rows of panel q, its 16-row tiles (two column tiles each)
        double* Pq = lds + poff[q];
        const int roff = RSBA_PB * (q - p);                                 // panel q's row 0 / column block inside panel p
        const int m = tile0 & (nwave - 1);
        for (int t = wave - m + (wave < m ? nwave : 0); t < 2 * nrt; t += nwave) {   // (tile tile0 + t is wavefront (tile0 + t) mod 8's)
          const int rt = t >> 1, ct = t & 1;
          const int prow = roff + 16 * rt + mi;
          d4_t acc = {0, 0, 0, 0};
#pragma unroll
          for (int qs = 0; qs < RSBA_PB; qs += 4) {
            const double a = prow < R ? Pan[prow * RSBA_PLD + qs + kk] : 0.0;
            const double b = Pan[(roff + 16 * ct + mi) * RSBA_PLD + qs + kk];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
          }
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) {
            const int r = 16 * rt + kk + 4 * tt;
            if (r < Rq) Pq[r * RSBA_PLD + 16 * ct + mi] -= acc[tt];
          }
        }
        tile0 += 2 * nrt;
      }
    }
    __syncthreads();
  }
  // y (the panels' last rows) and L' x = y, block by block from the last: one wavefront, lane (c, h) half of a column's terms
  if (wave == 0) {
    const int c = lane & 31, h = lane >> 5;
    for (int p = 0; p < np; ++p) if (lane < RSBA_PB) yv[RSBA_PB * p + lane] = (lds + poff[p])[(npad - RSBA_PB * p) * RSBA_PLD + lane];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int p = np - 1; p >= 0; --p) {
      const double* Pan = lds + poff[p];
      // t = y_p - sum over the rows below of L(row, 32 p + c) x(row)
      double t = 0.0;
      const int nbelow = npad - RSBA_PB * (p + 1);
      for (int r = h; r < nbelow; r += 2) t = fma(Pan[(RSBA_PB + r) * RSBA_PLD + c], yv[RSBA_PB * (p + 1) + r], t);
      t += __shfl_xor(t, 32, 64);
      const double tv = yv[RSBA_PB * p + c] - t;
      __builtin_amdgcn_wave_barrier();
      if (lane < RSBA_PB) tmp32[lane] = tv;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // x_p = T_p' t  (T_p lies where L_pp was: T[i][c], i >= c)
      double x = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) x = fma(Pan[(16 * h + k) * RSBA_PLD + c], tmp32[16 * h + k], x);
      x += __shfl_xor(x, 32, 64);
      __builtin_amdgcn_wave_barrier();
      if (lane < RSBA_PB) yv[RSBA_PB * p + lane] = x;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  __syncthreads();
  // the step of the reduced blocks and its norms (ReducedStepEpilogue's arithmetic on what this thread already holds; the lanes by
  // butterfly, the wavefronts in order: one barrier instead of a tree of eleven)
  double d2 = 0.0, x2 = 0.0, xc2 = 0.0, gm = 0.0;
  if (mine) {
    const double dd = -scl[tid] * yv[tid], xc = my_x + dd;
    delta_r[tid] = dd;
    params_c[my_cf] = xc;
    d2 = dd * dd; x2 = my_x * my_x; xc2 = xc * xc; gm = fabs(my_gc);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    d2 += __shfl_xor(d2, off, 64); x2 += __shfl_xor(x2, off, 64); xc2 += __shfl_xor(xc2, off, 64); gm = fmax(gm, __shfl_xor(gm, off, 64));
  }
  if (lane == 0) { s_red[wave][0] = d2; s_red[wave][1] = x2; s_red[wave][2] = xc2; s_red[wave][3] = gm; }
  __syncthreads();
  if (tid == 0) {
    double t4[4] = {s_red[0][0], s_red[0][1], s_red[0][2], s_red[0][3]};
    for (int w8 = 1; w8 < nwave; ++w8) { t4[0] += s_red[w8][0]; t4[1] += s_red[w8][1]; t4[2] += s_red[w8][2]; t4[3] = fmax(t4[3], s_red[w8][3]); }
    out[0] = t4[0]; out[1] = t4[1]; out[2] = t4[2]; out[3] = t4[3]; out[4] = s_ok > 0 ? 1.0 : 0.0;
  }
  (void)A;
}

__global__ void __launch_bounds__(1024)
k_marker_chol_finish(int nr, const double* __restrict__ red, double* __restrict__ F, const double* __restrict__ scale_r,
                     const int* __restrict__ col_full, const double* __restrict__ params_x, double* __restrict__ params_c,
                     double* __restrict__ delta_r, double* __restrict__ out, const int* __restrict__ ok_flag) {
  extern __shared__ double lds[];
  const RedLayout RL{nr};
  const int tid = threadIdx.x, nt = blockDim.x;
  double* y = BackSubstituteBlocks(nr, F, lds);
  double* ysol = F + (size_t)nr * nr;
  for (int i = tid; i < nr; i += nt) ysol[i] = y[i];
  __threadfence_block();
  __syncthreads();
  ReducedStepEpilogue(nr, red, RL, scale_r, ysol, col_full, params_x, params_c, delta_r, out, *ok_flag, lds);
}

// Back-substitution of one time and everything that follows from its step, one wavefront per time:
//   pass 1  lanes over the time's residual blocks: delta_t = -E (g_t + sum J_t' (J_c delta_c + J_m delta_m)) (fixed
//           shuffle tree), candidate time pose;
//   pass 2  the same residual blocks again (their Jacobians are still in the L2): the model cost change
//           -(J d).(r + J d / 2) and the squared residuals of the candidate (four corners through the three candidate poses).
// Per workgroup (four times): |delta_t|^2, |x_t + delta_t|^2, model cost change, candidate sum of squares.
// kLoss: the rows scaled by sqrt(rho') at x (wsq, k_mc_block_weight); the candidate's raw sum as without a loss, the workgroup's
// a rho(s_c) - s_c (wts: the blocks' weights, the device's time order) to drho_c[blockIdx.x] (k_marker_schur_finish<true>).
// kConst: a constant time (tconst[t]) takes a zero step (E = 0) and its |x_t|^2 stays out of the candidate's norm.
template <bool kLoss, bool kConst = false, bool kDist = false>
__global__ void __launch_bounds__(256)
k_time_backsub_terms(int T, const int* __restrict__ time_ptr, const int* __restrict__ time_full, const TimeSlots* __restrict__ ts,
                     const MarkerObs* __restrict__ mo, const double* __restrict__ obs8, typename IntrArg<kDist>::type intr, double half_side,
                     const double* __restrict__ posec /* pose constants at x */, const double* __restrict__ tdata,
                     const double* __restrict__ delta_r, const double* __restrict__ params_x, double* __restrict__ params_c,
                     double* __restrict__ delta_t, double* __restrict__ bpart /* gridDim.x x 4 */, double loss = 0.0,
                     const double* __restrict__ wsq = nullptr, double* __restrict__ drho_c = nullptr, const int* __restrict__ tconst = nullptr,
                     const double* __restrict__ wts = nullptr) {
  __shared__ double s_part[4][4];
  __shared__ double s_dcc[kLoss ? 4 : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x * 4 + wave;
  double d2 = 0, xc2 = 0, mcc = 0, cc = 0, dcc = 0;
  if (t < T) {
    const int o0 = time_ptr[t], o1 = time_ptr[t + 1], tf = time_full[t];
    double h[6] = {0, 0, 0, 0, 0, 0};
    for (int i = o0 + lane; i < o1; i += 64) {
      const TimeSlots s = ts[i];
      double dc[6], dm[6];
#pragma unroll
      for (int x = 0; x < 6; ++x) { dc[x] = s.col_cam >= 0 ? delta_r[s.col_cam + x] : 0.0; dm[x] = s.col_marker >= 0 ? delta_r[s.col_marker + x] : 0.0; }
      // the block's Jacobian rows, corner by corner, recomputed (never stored: see ElimArgs)
      const MarkerObs o = mo[i];
      const double* pcc = o.full_cam >= 0 ? posec + (size_t)(o.full_cam / 6) * CC_STRIDE : nullptr;
      const double* pct = posec + (size_t)(o.full_time / 6) * CC_STRIDE;
      const double* pcm = o.full_marker >= 0 ? posec + (size_t)(o.full_marker / 6) * CC_STRIDE : nullptr;
#pragma unroll 1
      for (int k = 0; k < 4; ++k) {
        double rr[2], Jc[36];
        MarkerCornerResidualJacobian<kDist>(pcc, pct, pcm, IntrOf(intr) + 4 * o.camera, (k == 0 || k == 3) ? -half_side : half_side, k < 2 ? half_side : -half_side,
                                            obs8[8 * (size_t)i + 2 * k], obs8[8 * (size_t)i + 2 * k + 1], rr, Jc, DistOf(intr, o.camera));
        if constexpr (kLoss) {
          const double w = wsq[i];
#pragma unroll
          for (int e = 0; e < 36; ++e) Jc[e] *= w;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          double m = 0.0;
#pragma unroll
          for (int x = 0; x < 6; ++x) m += Jc[q * 18 + x] * dc[x] + Jc[q * 18 + 12 + x] * dm[x];
#pragma unroll
          for (int x = 0; x < 6; ++x) h[x] += Jc[q * 18 + 6 + x] * m;
        }
      }
    }
#pragma unroll
    for (int x = 0; x < 6; ++x) {
      for (int off = 32; off > 0; off >>= 1) h[x] += __shfl_down(h[x], off, 64);
      h[x] = __shfl(h[x], 0, 64) + tdata[(size_t)t * 48 + 36 + x];
    }
    double dt[6], tc[6];   // the time's step and candidate pose, in every lane
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double sum = 0.0;
#pragma unroll
      for (int y = 0; y < 6; ++y) sum += tdata[(size_t)t * 48 + 6 * a + y] * h[y];
      dt[a] = -sum;
      tc[a] = params_x[tf + a] + dt[a];
      d2 += dt[a] * dt[a]; xc2 += tc[a] * tc[a];   // identical in every lane; lane 0's copy is used
    }
    if constexpr (kConst) { if (tconst[t]) xc2 = 0.0; }
    if (lane < 6) {
      double dsel = dt[0], csel = tc[0];
#pragma unroll
      for (int a = 1; a < 6; ++a) if (lane == a) { dsel = dt[a]; csel = tc[a]; }
      delta_t[6 * t + lane] = dsel;
      params_c[tf + lane] = csel;
    }
    // pass 2
    const double cx[4] = {-half_side, half_side, half_side, -half_side};
    const double cy[4] = {half_side, half_side, -half_side, -half_side};
    for (int i = o0 + lane; i < o1; i += 64) {
      const TimeSlots s = ts[i];
      const MarkerObs o = mo[i];
      double dl[18];
#pragma unroll
      for (int x = 0; x < 6; ++x) {
        dl[x] = s.col_cam >= 0 ? delta_r[s.col_cam + x] : 0.0;
        dl[6 + x] = dt[x];
        dl[12 + x] = s.col_marker >= 0 ? delta_r[s.col_marker + x] : 0.0;
      }
      {
        const double* pcc = o.full_cam >= 0 ? posec + (size_t)(o.full_cam / 6) * CC_STRIDE : nullptr;
        const double* pct = posec + (size_t)(o.full_time / 6) * CC_STRIDE;
        const double* pcm = o.full_marker >= 0 ? posec + (size_t)(o.full_marker / 6) * CC_STRIDE : nullptr;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
          double rr[2], Jc[36];
          MarkerCornerResidualJacobian<kDist>(pcc, pct, pcm, IntrOf(intr) + 4 * o.camera, (k == 0 || k == 3) ? -half_side : half_side, k < 2 ? half_side : -half_side,
                                              obs8[8 * (size_t)i + 2 * k], obs8[8 * (size_t)i + 2 * k + 1], rr, Jc, DistOf(intr, o.camera));
          if constexpr (kLoss) {
            const double w = wsq[i];
            rr[0] *= w; rr[1] *= w;
#pragma unroll
            for (int e = 0; e < 36; ++e) Jc[e] *= w;
          }
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            double m = 0.0;
#pragma unroll
            for (int x = 0; x < 18; ++x) m += Jc[q * 18 + x] * dl[x];
            mcc -= m * (rr[q] + 0.5 * m);
          }
        }
      }
      // candidate residuals: cameras and markers of the candidate are in params_c already (reduced solve), the time here
      const double fx = IntrOf(intr)[4 * o.camera], fy = IntrOf(intr)[4 * o.camera + 1], ppx = IntrOf(intr)[4 * o.camera + 2], ppy = IntrOf(intr)[4 * o.camera + 3];
      double sb = 0.0;   // (kLoss: the block's s_c)
      for (int k = 0; k < 4; ++k) {
        double pt[3] = {cx[k], cy[k], 0.0};
        if (o.full_marker >= 0) { const double* m = params_c + o.full_marker; RotateD(m, pt); pt[0] += m[3]; pt[1] += m[4]; pt[2] += m[5]; }
        RotateD(tc, pt); pt[0] += tc[3]; pt[1] += tc[4]; pt[2] += tc[5];
        if (o.full_cam >= 0) { const double* c = params_c + o.full_cam; RotateD(c, pt); pt[0] += c[3]; pt[1] += c[4]; pt[2] += c[5]; }
        double r0, r1;
        ProjectCornerResidual<kDist>(pt[0], pt[1], pt[2], fx, fy, ppx, ppy, DistOf(intr, o.camera),
                                     obs8[8 * (size_t)i + 2 * k], obs8[8 * (size_t)i + 2 * k + 1], &r0, &r1);
        cc += r0 * r0 + r1 * r1;
        if constexpr (kLoss) sb += r0 * r0 + r1 * r1;
      }
      if constexpr (kLoss) { double sq; dcc += wts[i] * LossAndScale(loss, sb, &sq) - sb; }
    }
  }
  // the lanes' sums in a fixed tree, then the four times of the workgroup in wave order
  for (int off = 32; off > 0; off >>= 1) { mcc += __shfl_down(mcc, off, 64); cc += __shfl_down(cc, off, 64); }
  if (lane == 0) { s_part[wave][0] = d2; s_part[wave][1] = xc2; s_part[wave][2] = mcc; s_part[wave][3] = cc; }
  if constexpr (kLoss) {
    for (int off = 32; off > 0; off >>= 1) dcc += __shfl_down(dcc, off, 64);
    if (lane == 0) s_dcc[wave] = dcc;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    bpart[4 * blockIdx.x + k] = ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k];
  }
  if constexpr (kLoss) {
    if (threadIdx.x == 0) drho_c[blockIdx.x] = ((s_dcc[0] + s_dcc[1]) + s_dcc[2]) + s_dcc[3];
  }
}

// Pose constants of the poses behind the reduced columns (cameras, markers) of a parameter array: the candidate's, once the
// reduced solve has written them — k_time_backsub_wg rotates the candidate's corners with matrices instead of three
// sin / cos per corner.
__global__ void __launch_bounds__(64) k_pose_constants_reduced(int nred_poses, const int* __restrict__ col_full, const double* __restrict__ params,
                                                               double* __restrict__ posec) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nred_poses) return;
  const int pose = col_full[6 * k] / 6;
  const double zero4[4] = {0.0, 0.0, 0.0, 0.0};
  double cc[CC_STRIDE];
  CameraConstants(params + 6 * (size_t)pose, zero4, cc);
#pragma unroll
  for (int q = 0; q < CC_STRIDE; ++q) posec[(size_t)pose * CC_STRIDE + q] = cc[q];
}

// k_time_backsub_terms with a WORKGROUP per time and a corner of a residual block per lane (round 4).  The wavefront-per-time
// form evaluates every corner's Jacobian rows twice — once for W_t delta_r, once more for the model cost change, which needs
// delta_t — on two residual blocks x four corners per lane one after the other, and rotates every candidate corner through three
// angle-axis poses (a sin / cos pair each).  Here a lane keeps what the second pass needs of its (at most kPer) corners in
// registers — J_r delta_r, the residual and the time block's two rows: 16 doubles a corner — so the rows are formed once; the
// candidate's cameras and markers come as rotation matrices (k_pose_constants_reduced), the time's own is formed once per lane.
// Sums in a fixed order: lanes by butterfly, the four wavefronts in order.  bpart: one entry (4 doubles) per time.
// kConst: the time's constant camera / marker blocks as pose-only slots behind the free ones (cs_ptr / cs_full: ElimArgs); their
// candidate is their pose at x.
// kDist: held to its sibling's two wavefronts a SIMD (256 registers; it would take 258) by the launch bounds' second argument (0: not set).
template <int kPer, int kThreads, bool kConst = false, bool kDist = false>
__global__ void __launch_bounds__(kThreads, kDist ? 2 : 0)
k_time_backsub_wg(int T, const int* __restrict__ time_ptr, const int* __restrict__ time_full, const TimeSlots* __restrict__ ts,
                  const MarkerObs* __restrict__ mo, const double* __restrict__ obs8, typename IntrArg<kDist>::type intr, double half_side,
                  const double* __restrict__ posec /* pose constants at x */, const double* __restrict__ posec_c /* candidate: cameras, markers */,
                  const double* __restrict__ tdata, const double* __restrict__ delta_r, const double* __restrict__ params_x,
                  double* __restrict__ params_c, double* __restrict__ delta_t, double* __restrict__ bpart /* T x 4 */,
                  const int* __restrict__ slot_ptr, const int* __restrict__ slot_col, const int* __restrict__ col_full,
                  const int* __restrict__ cs_ptr = nullptr, const int* __restrict__ cs_full = nullptr, const int* __restrict__ tconst = nullptr) {
  constexpr int kWaves = kThreads / 64;
  __shared__ double s_h[kWaves][8];
  extern __shared__ double s_tab[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x;
  const int o0 = time_ptr[t], o1 = time_ptr[t + 1], tf = time_full[t], ncorner = 4 * (o1 - o0);
  // the shot's tables, once per workgroup instead of three dependent trips to memory per lane (slot -> column -> pose -> constants):
  // pose constants at x of the time (row 0) and of its slots' cameras / markers, the candidate's rotation and translation of
  // the slots, the slots' part of delta_r
  const int s0 = slot_ptr[t], nslot = slot_ptr[t + 1] - s0;
  const int c0 = kConst ? cs_ptr[t] : 0, npose = kConst ? nslot + cs_ptr[t + 1] - c0 : nslot;   // (kConst: the pose-only slots behind)
  double* s_pc = s_tab;                                  // [(npose + 1)][CC_STRIDE]
  double* s_cd = s_pc + (size_t)(npose + 1) * CC_STRIDE;   // [npose][12]
  double* s_dr = s_cd + (size_t)npose * 12;               // [nslot][6]
  if constexpr (kConst) {
    for (int e = tid; e < (npose + 1) * CC_STRIDE; e += kThreads) {
      const int ps = e / CC_STRIDE, q = e - ps * CC_STRIDE;
      const int pose = (ps == 0 ? tf : (ps <= nslot ? col_full[slot_col[s0 + ps - 1]] : cs_full[c0 + ps - 1 - nslot])) / 6;
      s_pc[e] = posec[(size_t)pose * CC_STRIDE + q];
    }
    for (int e = tid; e < npose * 12; e += kThreads) {
      const int ps = e / 12, q = e - 12 * ps;
      const bool fr = ps < nslot;
      const int pose = (fr ? col_full[slot_col[s0 + ps]] : cs_full[c0 + ps - nslot]) / 6;
      s_cd[e] = (fr ? posec_c : posec)[(size_t)pose * CC_STRIDE + (q < 9 ? CC_R + q : CC_T + q - 9)];
    }
  } else {
    for (int e = tid; e < (nslot + 1) * CC_STRIDE; e += kThreads) {
      const int ps = e / CC_STRIDE, q = e - ps * CC_STRIDE;
      const int pose = (ps == 0 ? tf : col_full[slot_col[s0 + ps - 1]]) / 6;
      s_pc[e] = posec[(size_t)pose * CC_STRIDE + q];
    }
    for (int e = tid; e < nslot * 12; e += kThreads) {
      const int ps = e / 12, q = e - 12 * ps;
      const int pose = col_full[slot_col[s0 + ps]] / 6;
      s_cd[e] = posec_c[(size_t)pose * CC_STRIDE + (q < 9 ? CC_R + q : CC_T + q - 9)];
    }
  }
  for (int e = tid; e < nslot * 6; e += kThreads) { const int ps = e / 6; s_dr[e] = delta_r[slot_col[s0 + ps] + (e - 6 * ps)]; }
  // (lanes 0..5: their row of E, g_t and the time's parameters, wanted between the passes)
  double e_row[6] = {0, 0, 0, 0, 0, 0}, g_all[6] = {0, 0, 0, 0, 0, 0}, x_mine = 0.0;
  if (tid < 6) {
#pragma unroll
    for (int y = 0; y < 6; ++y) { e_row[y] = tdata[(size_t)t * 48 + 6 * tid + y]; g_all[y] = tdata[(size_t)t * 48 + 36 + y]; }
    x_mine = params_x[tf + tid];
  }
  __syncthreads();
  double m1[kPer][2], rk[kPer][2], jt[kPer][2][6];
  double h[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int e = tid + kThreads * u;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      m1[u][q] = 0.0; rk[u][q] = 0.0;
#pragma unroll
      for (int x = 0; x < 6; ++x) jt[u][q][x] = 0.0;
    }
    if (e < ncorner) {
      const int i = o0 + (e >> 2), k = e & 3;
      const TimeSlots sl = ts[i];
      double dc[6], dm[6];
#pragma unroll
      for (int x = 0; x < 6; ++x) { dc[x] = sl.slot_cam >= 0 ? s_dr[6 * sl.slot_cam + x] : 0.0; dm[x] = sl.slot_marker >= 0 ? s_dr[6 * sl.slot_marker + x] : 0.0; }
      const double* pcc = sl.slot_cam >= 0 ? s_pc + (size_t)(1 + sl.slot_cam) * CC_STRIDE
                          : (kConst && sl.slot_cam <= -2 ? s_pc + (size_t)(1 + ConstSlotPose(sl.slot_cam, nslot)) * CC_STRIDE : nullptr);
      const double* pct = s_pc;
      const double* pcm = sl.slot_marker >= 0 ? s_pc + (size_t)(1 + sl.slot_marker) * CC_STRIDE
                          : (kConst && sl.slot_marker <= -2 ? s_pc + (size_t)(1 + ConstSlotPose(sl.slot_marker, nslot)) * CC_STRIDE : nullptr);
      double rr[2], Jc[36];
      MarkerCornerResidualJacobian<kDist>(pcc, pct, pcm, IntrOf(intr) + 4 * sl.camera, (k == 0 || k == 3) ? -half_side : half_side, k < 2 ? half_side : -half_side,
                                          obs8[8 * (size_t)i + 2 * k], obs8[8 * (size_t)i + 2 * k + 1], rr, Jc, DistOf(intr, sl.camera));
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        double m = 0.0;
#pragma unroll
        for (int x = 0; x < 6; ++x) m += Jc[q * 18 + x] * dc[x] + Jc[q * 18 + 12 + x] * dm[x];
        m1[u][q] = m; rk[u][q] = rr[q];
#pragma unroll
        for (int x = 0; x < 6; ++x) { jt[u][q][x] = Jc[q * 18 + 6 + x]; h[x] += Jc[q * 18 + 6 + x] * m; }
      }
    }
  }
  // W_t delta_r: the lanes by butterfly (the same value in every lane), the wavefronts in order
#pragma unroll
  for (int x = 0; x < 6; ++x) {
    for (int off = 32; off > 0; off >>= 1) h[x] += __shfl_xor(h[x], off, 64);
    if (lane == 0) s_h[wave][x] = h[x];
  }
  __syncthreads();
  // the time's step and candidate pose: entry a on lane a of the first wavefront, the candidate's rotation matrix on one lane —
  // once per time, not once per lane (E h is 36 loads and as many FMAs, the matrix a sin / cos pair)
  __shared__ double s_dt[6], s_tc[6], s_rt[9], s_n2[2];
  if (tid < 6) {
    double hh[6];
#pragma unroll
    for (int x = 0; x < 6; ++x) {
      double sum = s_h[0][x];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) sum += s_h[w][x];
      hh[x] = sum + g_all[x];
    }
    double sum = 0.0;
#pragma unroll
    for (int y = 0; y < 6; ++y) sum += e_row[y] * hh[y];
    const double d = -sum, c = x_mine + d;
    s_dt[tid] = d; s_tc[tid] = c;
    delta_t[6 * t + tid] = d;
    params_c[tf + tid] = c;
  }
  __syncthreads();
  double dt[6], tc[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) { dt[a] = s_dt[a]; tc[a] = s_tc[a]; }
  if (tid == 0) {
    const double zero4[4] = {0.0, 0.0, 0.0, 0.0};
    double cct[CC_STRIDE];
    CameraConstants(tc, zero4, cct);
#pragma unroll
    for (int q = 0; q < 9; ++q) s_rt[q] = cct[CC_R + q];
    double d2 = 0.0, xc2 = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) { d2 += dt[a] * dt[a]; xc2 += tc[a] * tc[a]; }
    s_n2[0] = d2; s_n2[1] = (kConst && tconst[t]) ? 0.0 : xc2;
  }
  // pass 2: the model cost change from what the lane kept (while one lane forms the candidate's rotation matrix), then the
  // candidate's residuals with the candidate's rotation matrices
  double mcc = 0.0, cc = 0.0;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int e = tid + kThreads * u;
    if (e < ncorner) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        double m = m1[u][q];
#pragma unroll
        for (int x = 0; x < 6; ++x) m += jt[u][q][x] * dt[x];
        mcc -= m * (rk[u][q] + 0.5 * m);
      }
    }
  }
  __syncthreads();
  double Rt[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) Rt[q] = s_rt[q];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int e = tid + kThreads * u;
    if (e < ncorner) {
      const int i = o0 + (e >> 2), k = e & 3;
      const TimeSlots sl = ts[i];
      const double fx = IntrOf(intr)[4 * sl.camera], fy = IntrOf(intr)[4 * sl.camera + 1], ppx = IntrOf(intr)[4 * sl.camera + 2], ppy = IntrOf(intr)[4 * sl.camera + 3];
      double pt[3] = {(k == 0 || k == 3) ? -half_side : half_side, k < 2 ? half_side : -half_side, 0.0};
      auto apply = [&](const double* R, const double* tr) {
        const double a0 = R[0] * pt[0] + R[1] * pt[1] + R[2] * pt[2], a1 = R[3] * pt[0] + R[4] * pt[1] + R[5] * pt[2], a2 = R[6] * pt[0] + R[7] * pt[1] + R[8] * pt[2];
        pt[0] = a0 + tr[0]; pt[1] = a1 + tr[1]; pt[2] = a2 + tr[2];
      };
      if (sl.slot_marker >= 0) { const double* pc = s_cd + 12 * sl.slot_marker; apply(pc, pc + 9); }
      else if (kConst && sl.slot_marker <= -2) { const double* pc = s_cd + 12 * ConstSlotPose(sl.slot_marker, nslot); apply(pc, pc + 9); }
      apply(Rt, tc + 3);
      if (sl.slot_cam >= 0) { const double* pc = s_cd + 12 * sl.slot_cam; apply(pc, pc + 9); }
      else if (kConst && sl.slot_cam <= -2) { const double* pc = s_cd + 12 * ConstSlotPose(sl.slot_cam, nslot); apply(pc, pc + 9); }
      double r0, r1;
      ProjectCornerResidual<kDist>(pt[0], pt[1], pt[2], fx, fy, ppx, ppy, DistOf(intr, sl.camera),
                                   obs8[8 * (size_t)i + 2 * k], obs8[8 * (size_t)i + 2 * k + 1], &r0, &r1);
      cc += r0 * r0 + r1 * r1;
    }
  }
  for (int off = 32; off > 0; off >>= 1) { mcc += __shfl_down(mcc, off, 64); cc += __shfl_down(cc, off, 64); }
  __syncthreads();   // (s_h has been read)
  if (lane == 0) { s_h[wave][0] = mcc; s_h[wave][1] = cc; }
  __syncthreads();
  if (tid == 0) {
    bpart[4 * t + 0] = s_n2[0]; bpart[4 * t + 1] = s_n2[1];
    double sm = s_h[0][0], sc = s_h[0][1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) { sm += s_h[w][0]; sc += s_h[w][1]; }
    bpart[4 * t + 2] = sm; bpart[4 * t + 3] = sc;
  }
}

// (1024 threads, an entry = 32 bytes in two 16-byte loads, four entries in flight a thread, the lanes by butterfly and the sixteen
//  wavefronts in order: 256 threads walking 27 entries each, one dependent trip to memory after the other, and a tree of eight
//  barriers were 11 us for 200 KB)
// kLoss: the candidate's cost is 1/2 (sum r_c^2 + sum of drho_c [nd], the workgroups' sums of rho(s_c) - s_c); its raw sum of squares as
// without a loss.
template <bool kLoss>
__global__ void __launch_bounds__(1024)
k_marker_schur_finish(int nb_time, const double* __restrict__ bp_time, const double* __restrict__ red_scal,
                      const double* __restrict__ solve_out, double* __restrict__ res, int nd = 0, const double* __restrict__ drho_c = nullptr) {
  __shared__ double s[kLoss ? 5 : 4][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double v[kLoss ? 5 : 4] = {};
  const double2* __restrict__ bp2 = reinterpret_cast<const double2*>(bp_time);
  for (int b0 = tid; b0 < nb_time; b0 += 4 * 1024) {
    double2 lo[4], hi[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int b = min(b0 + 1024 * u, nb_time - 1); lo[u] = bp2[2 * b]; hi[u] = bp2[2 * b + 1]; }
#pragma unroll
    for (int u = 0; u < 4; ++u) if (b0 + 1024 * u < nb_time) { v[0] += lo[u].x; v[1] += lo[u].y; v[2] += hi[u].x; v[3] += hi[u].y; }
  }
  if constexpr (kLoss) for (int i = tid; i < nd; i += 1024) v[4] += drho_c[i];
  constexpr int kV = kLoss ? 5 : 4;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < kV; ++k) v[k] += __shfl_xor(v[k], off, 64);
  if (lane == 0) for (int k = 0; k < kV; ++k) s[k][wave] = v[k];
  __syncthreads();
  if (tid == 0) {
    for (int k = 0; k < kV; ++k) { double t = s[k][0]; for (int w = 1; w < 16; ++w) t += s[k][w]; s[k][0] = t; }
    res[RES_COST_X] = 0.5 * red_scal[0];
    res[RES_GMAX] = fmax(red_scal[3], solve_out[3]);
    res[RES_XNORM2] = red_scal[1] + solve_out[1];
    res[RES_POINT_FAIL] = red_scal[2];
    res[RES_CHOL_OK] = (solve_out[4] != 0.0 && red_scal[2] == 0.0) ? 1.0 : 0.0;
    res[RES_STEP2] = solve_out[0] + s[0][0];
    res[RES_XCNORM2] = solve_out[2] + s[1][0];
    res[RES_MCC] = s[2][0];
    double c = 0.5 * (kLoss ? s[3][0] + s[4][0] : s[3][0]);
    if (!(c == c) || !(fabs(c) <= DBL_MAX)) c = DBL_MAX;
    res[RES_COST_C] = c;
    res[RES_SUMSQ_C] = s[3][0];
    res[RES_STALL] = 0.0; res[RES_WAIT_TIMEOUT] = 0.0;
  }
}

// The priors (PriorDevice) on the time-eliminating path: ONE MORE PARTIAL SYSTEM behind the chunks', summed by k_marker_reduce in its
// fixed order.  The partial system is zeroed ONCE, at create (MarkerSchurDevice::Upload): which blocks carry a prior is fixed there, so
// every step writes the same entries and no other — per prior the packed lower triangle of A'A on its block's diagonal, A'A (x - b)
// into gc, diag(A'A) into diagU and, by thread 0 in the priors' order, sum |A (x - b)|^2 into scal[0] (the chunks' convention: twice
// the cost).  The columns of a block's constant components are taken out of A first (exact zeros: the unit diagonal
// is k_mc_subset_slots'), the residual keeps the held values.  A prior on a constant block (col < 0) counts in the cost only.
// One workgroup, thread per prior.
__global__ void __launch_bounds__(256) k_mc_prior_system(int nr, int K, const int* __restrict__ full, const int* __restrict__ col,
                                                         const int* __restrict__ mask, const double* __restrict__ ab,
                                                         const double* __restrict__ params_x, double* __restrict__ P, double* __restrict__ pe) {
  const PartLayout PL{nr};
  const int tid = threadIdx.x;
  for (int k = tid; k < K; k += 256) {
    const double* __restrict__ A = ab + 42 * (size_t)k;
    const double* __restrict__ x = params_x + full[k];
    double d[6], r[6], ss = 0.0;
    for (int q = 0; q < 6; ++q) d[q] = x[q] - A[36 + q];
    for (int i = 0; i < 6; ++i) { double t = 0.0; for (int q = 0; q < 6; ++q) t += A[6 * i + q] * d[q]; r[i] = t; ss += t * t; }
    pe[k] = ss;
    const int c = col[k], m = mask[k];
    if (c < 0) continue;
    for (int a = 0; a < 6; ++a) {
      const bool ha = (m >> a) & 1;
      double g = 0.0;
      for (int i = 0; i < 6; ++i) g += (ha ? 0.0 : A[6 * i + a]) * r[i];
      P[PL.gc() + c + a] = g;
      for (int b = 0; b <= a; ++b) {
        const bool hb = (m >> b) & 1;
        double h = 0.0;
        for (int i = 0; i < 6; ++i) h += (ha ? 0.0 : A[6 * i + a]) * (hb ? 0.0 : A[6 * i + b]);
        P[PL.S() + (size_t)(c + a) * (c + a + 1) / 2 + (c + b)] = h;
        if (a == b) P[PL.diagU() + c + a] = h;
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0) { double t = 0.0; for (int k = 0; k < K; ++k) t += pe[k]; P[PL.scal()] = t; }
}

// ... and behind the reduced solve: the priors' share of the model cost change -(A d).(r + A d / 2) (d: the block's reduced step) as one
// more entry (0, 0, mcc, 0) of bp_time, and sum |A (x_c - b)|^2 at the candidate as one more entry of drho_c: it joins the candidate's
// cost and stays out of its raw sum of squares (k_marker_schur_finish<true>).  One workgroup, thread per prior, the sums by thread 0.
__global__ void __launch_bounds__(256) k_mc_prior_candidate(int K, const int* __restrict__ full, const int* __restrict__ col,
                                                            const int* __restrict__ mask, const double* __restrict__ ab,
                                                            const double* __restrict__ params_x, const double* __restrict__ params_c,
                                                            const double* __restrict__ delta_r, double* __restrict__ pe,
                                                            double* __restrict__ bp_entry, double* __restrict__ drho_entry) {
  const int tid = threadIdx.x;
  for (int k = tid; k < K; k += 256) {
    const double* __restrict__ A = ab + 42 * (size_t)k;
    const double* __restrict__ x = params_x + full[k];
    const double* __restrict__ xc = params_c + full[k];
    const int c = col[k], m = mask[k];
    double d[6], dc[6], dl[6];
    for (int q = 0; q < 6; ++q) { d[q] = x[q] - A[36 + q]; dc[q] = xc[q] - A[36 + q]; dl[q] = (c < 0 || ((m >> q) & 1)) ? 0.0 : delta_r[c + q]; }
    double mcc = 0.0, sc = 0.0;
    for (int i = 0; i < 6; ++i) {
      double r = 0.0, rc = 0.0, mr = 0.0;
      for (int q = 0; q < 6; ++q) { r += A[6 * i + q] * d[q]; rc += A[6 * i + q] * dc[q]; mr += A[6 * i + q] * dl[q]; }
      mcc -= mr * (r + 0.5 * mr);
      sc += rc * rc;
    }
    pe[2 * k] = mcc; pe[2 * k + 1] = sc;
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    double m = 0.0, c = 0.0;
    for (int k = 0; k < K; ++k) { m += pe[2 * k]; c += pe[2 * k + 1]; }
    bp_entry[0] = 0.0; bp_entry[1] = 0.0; bp_entry[2] = m; bp_entry[3] = 0.0;
    drho_entry[0] = c;
  }
}

}  // namespace rsba
#include "ba_marker_split.hpp"
#include "ba_marker_intr_split.hpp"
namespace rsba {

// Runtime flags as template arguments: Dispatch(f, a, b) calls f(std::integral_constant<bool, a>(), std::integral_constant<bool, b>()).
// f's body is instantiated for every combination of the flags: a launch whose kernel exists only for some of them rules the others
// out with if constexpr.
template <typename F> void Dispatch(F&& f) { f(); }
template <typename F, typename... R> void Dispatch(F&& f, bool b, R... rest) {
  if (b) Dispatch([&](auto... c) { f(std::true_type(), c...); }, rest...);
  else Dispatch([&](auto... c) { f(std::false_type(), c...); }, rest...);
}

// The time-eliminating path on the device: what PlanMarkerChain (ba_marker_plan.hpp) planned, allocated and uploaded, and the step
// that launches from the plan.
struct MarkerSchurDevice {
  MarkerPlan plan;   // Upload; its tables are dropped once they are on the device
  // the split elimination (ba_marker_split.hpp)
  int* x_order = nullptr;
  int4 *sb_blk = nullptr, *xi_blk = nullptr;
  int *slot_order = nullptr, *slot_time = nullptr, *sb_ptr = nullptr, *xi_ptr = nullptr, *xi_cc = nullptr, *xi_cm = nullptr, *xc_ptr = nullptr;
  double *sp = nullptr, *xout = nullptr, *tscal = nullptr;
  int* blk_time = nullptr;
  hipStream_t fork_s[2] = {nullptr, nullptr};   // the three product kernels side by side
  hipEvent_t fork_ev[3] = {nullptr, nullptr, nullptr};
  double* posec_c = nullptr; // pose constants of the candidate's cameras and markers
  double *wsq = nullptr, *drho = nullptr, *drho_c = nullptr;   // [N] each: sqrt(rho'), rho(s) - s at x (k_mc_block_weight); per candidate
                                                                 // workgroup (at most N): its blocks' rho(s_c) - s_c (with_loss only)
  double* wts = nullptr;         // [N] the blocks' weights in the device's time order (with_loss only; all ones when the problem had none)
  MarkerObs* mo = nullptr;
  TimeSlots* ts = nullptr;
  int *chunk_ptr = nullptr, *time_ptr = nullptr, *slot_ptr = nullptr, *slot_col = nullptr, *time_full = nullptr, *col_full = nullptr,
      *ok_flag = nullptr;
  double *obs8 = nullptr, *intr = nullptr, *params[2] = {nullptr, nullptr}, *params0 = nullptr;
  double *posec = nullptr, *ss_x = nullptr, *scale_t = nullptr, *scale_r = nullptr, *tdata = nullptr,
         *part = nullptr, *red = nullptr, *A = nullptr, *Wm = nullptr, *delta_r = nullptr, *delta_t = nullptr, *bp_time = nullptr,
         *solve_out = nullptr, *res = nullptr;
  int cur = 0;
  int* tc_flags = nullptr;   // persistent tiled factorisation of a large reduced system (ba_cholesky_tiles.hpp)
  double* tc_hand = nullptr; // ... its diagonal chain's hand-over buffers
  int* tc_map = nullptr;     // ... which tile each workgroup takes (TileOrder)
  int tc_tag = 0;
  // constant blocks (has_const only): the times' pose-only slots, constant flags, the constant poses some residual applies
  int *cs_ptr = nullptr, *cs_full = nullptr, *tconst = nullptr, *cpose_full = nullptr;
  double* dist = nullptr;           // [C][5], indexed as intr (with_dist only)
  int* tflags = nullptr;            // [T] bit 0: a constant time; bits 8..13: the time's constant components (with_subset only)
  unsigned char* rmask = nullptr;   // [nr / 6] the reduced blocks' constant components (with_subset only)
  PriorDevice prior;                // K priors: one more partial system and one more bp_time / drho_c entry (with_loss then)
  double* prior_pe = nullptr;       // [2 K] the priors' terms, summed in order by thread 0
  // free intrinsics (plan.with_intr only; ba_marker_intr_split.hpp): params[2] / params0 continue behind the nfull pose values with six
  // values per camera, as MarkerDevice has them; intr / dist above stay the problem's values (dist then always there, zeros where the
  // problem has none), the kernels read the current (x) and candidate (c) copies, scattered from the state in every step
  int nstate = 0;                   // doubles of params[2] / params0
  std::vector<int> intr_mask;       // [C] the masks this solver was created with
  double *intr_x = nullptr, *dist_x = nullptr, *intr_c = nullptr, *dist_c = nullptr;
  IntrSlots* ti = nullptr;
  int *is_slot = nullptr, *is_cam = nullptr, *ib_ptr = nullptr, *ib_blk = nullptr, *xs_item = nullptr, *xs_ptr = nullptr, *xs_src = nullptr;
  double* xsrc = nullptr;           // [nislots + nib][36] the source records of the pair items with an intrinsics row

  // Every device buffer above has one owner: Alloc records the member it fills, Free releases what was recorded.
  std::vector<void**> owned;
  // n elements (at least 8 bytes), and h's n elements in them when h is given
  template <typename Td, typename Th = Td>
  bool Alloc(Td** q, size_t n, const Th* h = nullptr) {
    static_assert(sizeof(Td) == sizeof(Th), "uploaded as it lies on the host");
    if (hipMalloc((void**)q, std::max<size_t>(n * sizeof(Td), 8)) != hipSuccess) return false;
    owned.push_back((void**)q);
    return h == nullptr || n == 0 || hipMemcpy(*q, h, n * sizeof(Td), hipMemcpyHostToDevice) == hipSuccess;
  }
  template <typename Td, typename Th>
  bool Alloc(Td** q, const std::vector<Th>& h) { return Alloc(q, h.size(), h.data()); }
  void Free() {
    prior.Free();
    for (void** q : owned) { (void)hipFree(*q); *q = nullptr; }
    owned.clear();
    for (auto& q : fork_s) if (q) { (void)hipStreamDestroy(q); q = nullptr; }
    for (auto& q : fork_ev) if (q) { (void)hipEventDestroy(q); q = nullptr; }
  }

  // true when the problem should take this path (schur_impl: 0 never, 1 when the dense system outgrows one workgroup, 2 always)
  static bool Wanted(const rsba_problem& p, int schur_impl) {
    if (schur_impl == 0) return false;
    if (schur_impl >= 2) return true;
    const int nblocks = p.num_cameras + p.num_times + p.num_markers;
    return 6 * nblocks > RSBA_CHOL_MAXN;
  }

  // The kernels whose dynamic LDS can exceed the default limit, by the plan: Upload raises the limit of, and Step launches, the same one.
  auto AccKernel() const -> void (*)(AccArgs) {
    const MarkerPlan& P = plan;
    return P.acc_tiles == 3 ? (P.acc_tb == 2 ? k_mc_accumulate_mfma<3, 2> : k_mc_accumulate_mfma<3, 1>) : P.acc_tiles == 8 ? k_mc_accumulate_mfma<8, 1>
           : P.lds_s ? k_mc_accumulate<true> : k_mc_accumulate<false>;
  }
  template <typename F> void WithElimKernel(F&& f) const {   // f(kernel, D)
    Dispatch([&](auto S, auto Cn, auto D) { f(k_time_eliminate<S.value, Cn.value, D.value>, D); }, plan.lds_s, plan.has_const, plan.with_dist);
  }
  template <typename F> void WithBacksubWgKernel(F&& f) const {   // f(kernel, D)
    Dispatch([&](auto Cn, auto D) { f(k_time_backsub_wg<2, 256, Cn.value, D.value>, D); }, plan.has_const, plan.with_dist);
  }
  static bool RaiseLds(const void* kernel, size_t bytes) {
    return bytes <= 48 * 1024 || hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
  }

  // loss: a robust loss is set, or the problem carries observation weights or priors (PlanMarkerChain).  RSBA_ERR_UNSUPPORTED: the
  // solver takes the dense path.
  // want_intr: the problem's free intrinsics join the reduced system (schur_impl = 3)
  int Upload(const rsba_problem& p, bool loss = false, bool want_intr = false) {
    int cus = 256;
    { int dev = 0; hipDeviceProp_t prop; if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount; }
    const int rc = want_intr ? PlanMarkerChain(p, loss, cus, MarkerSwitches::FromEnv(), &plan, true) : PlanMarkerChain(p, loss, cus, MarkerSwitches::FromEnv(), &plan);
    if (rc != RSBA_OK) return rc;
    const MarkerPlan& P = plan;
    const MarkerTables& B = plan.tab;
    const size_t N = P.N, T = P.T, nr = P.nr, nfull = P.nfull, np = P.np;
    const size_t nA = (nr + 2) * nr, npart = PartLayout{P.nr}.size();
    const size_t C = (size_t)p.num_cameras;
    nstate = (int)(nfull + (P.with_intr ? 6 * C : 0));
    // the state: the poses, then (with_intr) fx fy cx cy k1 k2 of every camera; the coefficients as an array that is always there then
    std::vector<double> hstate(p.parameters), hdist(p.distortion);
    if (P.with_intr) {
      if (hdist.empty()) hdist.assign(5 * C, 0.0);
      hstate.resize((size_t)nstate);
      intr_mask.assign(C, 0);
      for (size_t k = 0; k < C; ++k) {
        intr_mask[k] = p.intrinsics_free_mask((int)k);
        for (int q = 0; q < 4; ++q) hstate[nfull + 6 * k + q] = p.intrinsics[4 * k + q];
        hstate[nfull + 6 * k + 4] = hdist[5 * k]; hstate[nfull + 6 * k + 5] = hdist[5 * k + 1];
      }
    }
    if (np && (prior.Upload(p, B.pcols) != RSBA_OK || !Alloc(&prior_pe, 2 * (size_t)prior.K))) return RSBA_ERR_HIP;
    bool ok = Alloc(&mo, B.hmo) && Alloc(&ts, B.hts) && Alloc(&chunk_ptr, B.cptr) && Alloc(&time_ptr, B.tptr) && Alloc(&slot_ptr, B.sptr) &&
              Alloc(&slot_col, B.scol) && Alloc(&time_full, B.tfull) && Alloc(&col_full, B.cf) && Alloc(&ok_flag, 1) && Alloc(&obs8, B.hobs) &&
              Alloc(&intr, p.intrinsics) && Alloc(&params[0], (size_t)nstate) && Alloc(&params[1], (size_t)nstate) && Alloc(&params0, hstate) &&
              Alloc(&posec, nfull / 6 * CC_STRIDE) && Alloc(&posec_c, nfull / 6 * CC_STRIDE) && Alloc(&ss_x, N) && Alloc(&scale_t, 6 * T) &&
              Alloc(&scale_r, nr) && Alloc(&tdata, 48 * T) && Alloc(&part, (P.G + np) * npart) && Alloc(&red, RedLayout{P.nr}.size()) && Alloc(&A, nA) &&
              (P.nr <= RSBA_CHOL_MAXN || Alloc(&Wm, nA)) && Alloc(&delta_r, nr) && Alloc(&delta_t, 6 * T) && Alloc(&bp_time, 4 * (P.nb_time + np)) &&
              Alloc(&solve_out, 8) && Alloc(&res, RES_SIZE) &&
              (!P.with_loss || (Alloc(&wsq, N) && Alloc(&drho, N) && Alloc(&drho_c, N + np) && Alloc(&wts, N))) &&
              (!P.with_dist || Alloc(&dist, hdist)) &&
              (!P.with_intr || (Alloc(&intr_x, p.intrinsics) && Alloc(&intr_c, p.intrinsics) && Alloc(&dist_x, hdist) && Alloc(&dist_c, hdist) && Alloc(&ti, B.hti) &&
                                Alloc(&is_slot, B.h_is_slot) && Alloc(&is_cam, B.h_is_cam) && Alloc(&ib_ptr, B.h_ib_ptr) && Alloc(&ib_blk, B.h_ib_blk) &&
                                Alloc(&xs_item, B.h_xs_item) && Alloc(&xs_ptr, B.h_xs_ptr) && Alloc(&xs_src, B.h_xs_src) &&
                                Alloc(&xsrc, ((size_t)P.nislots + P.nib) * 36))) &&
              (!P.has_const || (Alloc(&cs_ptr, B.csptr) && Alloc(&cs_full, B.csfull) && Alloc(&tconst, B.htc) && Alloc(&cpose_full, B.cpf))) &&
              (!P.with_subset || (Alloc(&tflags, B.htflags) && Alloc(&rmask, B.hrmask))) &&
              (!P.split || (Alloc(&slot_order, B.h_order) && Alloc(&x_order, B.h_xorder) && Alloc(&slot_time, B.h_slot_time) && Alloc(&sb_ptr, B.h_sb_ptr) &&
                            Alloc(&sb_blk, B.h_sb_blk) && Alloc(&xi_ptr, B.h_xi_ptr) && Alloc(&xi_blk, B.h_xi_blk) && Alloc(&xi_cc, B.h_xi_cc) &&
                            Alloc(&xi_cm, B.h_xi_cm) && Alloc(&xc_ptr, B.h_xc_ptr) && Alloc(&sp, (size_t)P.nslots * RSBA_SP_STRIDE) &&
                            Alloc(&xout, (size_t)P.nx * 36) && Alloc(&tscal, 4 * T))) &&
              (!P.split_backsub || Alloc(&blk_time, B.h_bt)) &&
              (P.tc_tiles == 0 || (Alloc(&tc_flags, P.tc_flags) && Alloc(&tc_map, B.tc_map) && Alloc(&tc_hand, P.tc_hand)));
    if (!ok) return RSBA_ERR_HIP;
    if (P.with_loss) {
      const std::vector<double> ones(p.observation_weights.empty() ? N : 0, 1.0);
      if (SetWeights(p.observation_weights.empty() ? ones.data() : p.observation_weights.data()) != RSBA_OK) return RSBA_ERR_HIP;
    }
    if (hipMemset(res, 0, RES_SIZE * 8) != hipSuccess) return RSBA_ERR_HIP;
    // the priors' partial system: zeros for good (which blocks carry a prior is fixed here), k_mc_prior_system writes the prior blocks' entries only
    if (np && hipMemset(part + P.G * npart, 0, npart * 8) != hipSuccess) return RSBA_ERR_HIP;
    if (P.nr == 0) {
      // no reduced system: the solve's result block is that of an empty one, once
      const double empty[5] = {0.0, 0.0, 0.0, 0.0, 1.0};
      if (hipMemcpy(solve_out, empty, sizeof(empty), hipMemcpyHostToDevice) != hipSuccess) return RSBA_ERR_HIP;
    }
    // the tiled factorisation's flags start at zero, its hand-overs with the sentinel everywhere
    if (P.tc_tiles > 0 && (hipMemset(tc_flags, 0, P.tc_flags * sizeof(int)) != hipSuccess || hipMemset(tc_hand, 0xff, P.tc_hand * sizeof(double)) != hipSuccess))
      return RSBA_ERR_HIP;
    if (P.fork) {
      for (auto& q : fork_s) ok = ok && hipStreamCreateWithFlags(&q, hipStreamNonBlocking) == hipSuccess;
      for (auto& q : fork_ev) ok = ok && hipEventCreateWithFlags(&q, hipEventDisableTiming) == hipSuccess;
    }
    // dynamic LDS above the default limit, for the kernels the path runs
    if (P.split) ok = ok && RaiseLds((const void*)AccKernel(), P.lds_acc);
    else WithElimKernel([&](auto k, auto) { ok = ok && RaiseLds((const void*)k, P.lds_elim); });
    if (P.backsub_wg) WithBacksubWgKernel([&](auto k, auto) { ok = ok && RaiseLds((const void*)k, P.lds_bw); });
    if (P.nr > RSBA_CHOL_MAXN) {
      ok = ok && RaiseLds((const void*)k_chol_step, CholStepLdsDoubles() * sizeof(double));
      if (P.tc_tiles > 0) ok = ok && RaiseLds((const void*)k_chol_tiles_persistent, TileCholLdsDoubles() * sizeof(double));
    } else if (P.nr > 0) {
      ok = ok && RaiseLds((const void*)k_marker_reduced_solve, P.lds_solve);
      if (P.debug) fprintf(stderr, "rsba: marker reduced system %d columns, solve in LDS: %d (%zu bytes)\n", P.nr, (int)P.solve_lds, P.lds_solve_lds);
      if (P.solve_lds) ok = ok && RaiseLds((const void*)k_marker_reduced_solve_lds, P.lds_solve_lds);
    }
    plan.tab = MarkerTables();
    return ok ? RSBA_OK : RSBA_ERR_HIP;
  }
  // the blocks' weights, given in the problem's order, into the device's time order (a solver that runs the kLoss instances)
  int SetWeights(const double* w) {
    std::vector<double> h((size_t)plan.N);
    for (int k = 0; k < plan.N; ++k) h[k] = w[plan.order[k]];
    return hipMemcpy(wts, h.data(), (size_t)plan.N * 8, hipMemcpyHostToDevice) == hipSuccess ? RSBA_OK : RSBA_ERR_HIP;
  }
  int Reset(hipStream_t st) {
    if (hipMemcpyAsync(params[0], params0, (size_t)nstate * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return RSBA_ERR_HIP;
    if (hipMemcpyAsync(params[1], params0, (size_t)nstate * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return RSBA_ERR_HIP;
    if (plan.ncpose > 0) {
      // the constant cameras' and markers' candidate pose constants are those at x, for the whole run
      k_pose_constants_reduced<<<(plan.ncpose + 63) / 64, 64, 0, st>>>(plan.ncpose, cpose_full, params0, posec_c);
      if (hipGetLastError() != hipSuccess) return RSBA_ERR_HIP;
    }
    cur = 0;
    return RSBA_OK;
  }
  void Accept() { cur = 1 - cur; }

  // A kernel templated on loss, constant blocks, distortion or subset masks is launched once, through Dispatch; the arguments of the
  // instances that do not read them (wsq, drho_c, wts without a loss; tconst, cs_ptr, cs_full without constant blocks) are the null
  // pointers those members hold then.
  template <typename Timer>
  int Step(hipStream_t st, const rsba_options& o, double radius, bool first, double* res_host, Timer& Tm) {
    const MarkerPlan& P = plan;
    const int N = P.N, T = P.T, nr = P.nr, nfull = P.nfull, G = P.G, np = P.np, nb_time = P.nb_time;
    const double half_side = P.half_side;
    IterParams ip;
    ip.radius = radius; ip.min_lm_diagonal = o.min_lm_diagonal; ip.max_lm_diagonal = o.max_lm_diagonal; ip.huber_delta = 0.0;
    ip.first = first ? 1 : 0; ip.jacobi_scaling = o.jacobi_scaling;
    // the robust loss, read as the point model reads it (signed: see LossAndScale); Upload was told whether there is one
    // (with_loss and huber_delta = 0: observation weights alone, rho(s) = s)
    const double loss = P.with_loss && o.huber_delta > 0.0 ? (o.loss_type == RSBA_LOSS_CAUCHY ? -o.huber_delta : o.huber_delta) : 0.0;
    const int x = cur, c = 1 - cur;
    if (hipMemcpyAsync(params[c], params[x], (size_t)nstate * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return RSBA_ERR_HIP;
    auto chk = [&](const char* what) {
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) { fprintf(stderr, "rsba: %s launch failed: %s\n", what, hipGetErrorString(e)); return false; }
      return true;
    };
    if (!chk("(before marker step)")) return RSBA_ERR_HIP;
    const RedLayout RL{nr};
    // free intrinsics: every kernel at x reads the state's values through the current copies (so a rejected candidate's values are
    // never seen by a linearisation), the candidate's residuals the candidate copies
    const int ncams = (int)intr_mask.size();
    const double* intr_u = P.with_intr ? intr_x : intr;
    const double* dist_u = P.with_intr ? dist_x : dist;
    if (P.with_intr) {
      Tm.Begin("k_mc_intr_state", st);
      k_mc_intr_state<<<(ncams + 63) / 64, 64, 0, st>>>(ncams, nfull, params[x], intr_x, dist_x);
      Tm.End(st);
    }
    auto intr_of = [&](auto D) { return IntrPass<D.value>(intr_u, dist_u); };
    Tm.Begin("k_pose_constants", st);
    k_pose_constants<<<(nfull / 6 + 255) / 256, 256, 0, st>>>(nfull / 6, params[x], posec);
    Tm.End(st);
    if (P.split) {
      // (nslots: the threads of k_mc_slot_products, the only kernel that reads it — the pose slots; an intrinsics slot has its own kernel)
      SplitArgs sa{P.nslots_pose, T, P.nx, P.ncam_cols, P.nx_threads, slot_order, x_order, slot_time, slot_col, sb_ptr, sb_blk, time_ptr, time_full, col_full, ts, mo, obs8, intr_u, posec, half_side,
                   xi_ptr, xi_blk, xi_cc, xi_cm, sp, xout, wsq, drho};
      SplitArgsDist sad; static_cast<SplitArgs&>(sad) = sa; sad.dist = dist_u;
      const IntrSplitArgs ia{P.nislots, P.nib, is_slot, is_cam, ib_ptr, ib_blk, slot_time, time_full, mo, obs8, intr_x, dist_x, posec, half_side, P.with_loss ? wsq : nullptr, sp, xsrc};
      auto split_args = [&](auto D) -> const typename SplitArgT<D.value>::type& { if constexpr (D.value) return sad; else return sa; };
      if (P.with_loss) {
        // the corrector's weights at x, wanted by all three product kernels
        Tm.Begin("k_mc_block_weight", st);
        Dispatch([&](auto D) { k_mc_block_weight<D.value><<<(N + 255) / 256, 256, 0, st>>>(N, ts, mo, obs8, intr_of(D), half_side, posec, loss, wts, wsq, drho); }, P.with_dist);
        Tm.End(st);
      }
      // the three product kernels are independent and none fills the chip: side by side on three streams (one after the other
      // when every kernel is timed)
      const bool fork = fork_s[0] != nullptr && !Tm.enabled();
      hipStream_t s_time = fork ? fork_s[0] : st, s_cross = fork ? fork_s[1] : st;
      if (fork) {
        if (hipEventRecord(fork_ev[0], st) != hipSuccess || hipStreamWaitEvent(s_time, fork_ev[0], 0) != hipSuccess ||
            hipStreamWaitEvent(s_cross, fork_ev[0], 0) != hipSuccess) return RSBA_ERR_HIP;
      }
      if (P.nslots > 0) {   // (none: n_r = 0)
        if (P.nslots_pose > 0) {
          Tm.Begin("k_mc_slot_products", st);
          Dispatch([&](auto L, auto D) { k_mc_slot_products<L.value, D.value><<<(P.nslots_pose + 255) / 256, 256, 0, st>>>(split_args(D)); }, P.with_loss, P.with_dist);
          Tm.End(st);
        }
        if (P.nislots > 0) {
          Tm.Begin("k_mc_intr_slot_products", st);
          k_mc_intr_slot_products<<<(P.nislots + 255) / 256, 256, 0, st>>>(ia);
          Tm.End(st);
        }
        if (P.with_subset) {
          Tm.Begin("k_mc_subset_slots", st);
          k_mc_subset_slots<<<(unsigned)(((size_t)P.nslots * 64 + 255) / 256), 256, 0, st>>>(P.nslots, slot_time, slot_col, tflags, rmask, sp);
          Tm.End(st);
        }
      }
      Tm.Begin("k_mc_time_products", st);
      Dispatch([&](auto L, auto Cn, auto D, auto Sb) {
        // (subset masks ride on the constant-block instances: no <*, false, D, true>; the time's flags arrive where tconst does)
        if constexpr (Cn.value || !Sb.value)
          k_mc_time_products<L.value, Cn.value, D.value, Sb.value><<<(T + 3) / 4, 256, 0, s_time>>>(split_args(D), ip, params[x], scale_t, tdata, tscal, Sb.value ? tflags : tconst);
      }, P.with_loss, P.has_const, P.with_dist, P.with_subset);
      Tm.End(st);
      if (P.nx > 0) {
        if (P.nx_threads > 0) {
          Tm.Begin("k_mc_cross", st);
          Dispatch([&](auto L, auto D) { k_mc_cross<L.value, D.value><<<(P.nx_threads + 255) / 256, 256, 0, s_cross>>>(split_args(D)); }, P.with_loss, P.with_dist);
          Tm.End(st);
        }
        if (P.nxs > 0) {
          // the items with an intrinsics row: the (camera, intrinsics) records come from k_mc_intr_slot_products, on the solver's stream
          if (fork && (hipEventRecord(fork_ev[1], st) != hipSuccess || hipStreamWaitEvent(s_cross, fork_ev[1], 0) != hipSuccess)) return RSBA_ERR_HIP;
          Tm.Begin("k_mc_intr_marker_cross", st);
          k_mc_intr_marker_cross<<<(P.nib + 255) / 256, 256, 0, s_cross>>>(ia);
          Tm.End(st);
          Tm.Begin("k_mc_intr_cross_sum", st);
          k_mc_intr_cross_sum<<<(unsigned)(((size_t)P.nxs * 36 + 255) / 256), 256, 0, s_cross>>>(P.nxs, xs_item, xs_ptr, xs_src, xsrc, xout);
          Tm.End(st);
        }
        if (P.with_subset) {
          Tm.Begin("k_mc_subset_cross", st);
          k_mc_subset_cross<<<(unsigned)(((size_t)P.nx * 36 + 255) / 256), 256, 0, s_cross>>>(P.nx, xi_cc, xi_cm, rmask, xout);
          Tm.End(st);
        }
      }
      if (fork) {
        if (hipEventRecord(fork_ev[1], s_time) != hipSuccess || hipEventRecord(fork_ev[2], s_cross) != hipSuccess ||
            hipStreamWaitEvent(st, fork_ev[1], 0) != hipSuccess || hipStreamWaitEvent(st, fork_ev[2], 0) != hipSuccess) return RSBA_ERR_HIP;
      }
      AccArgs aa{nr, P.dmax, chunk_ptr, slot_ptr, slot_col, sp, tdata, tscal, xc_ptr, xi_cc, xi_cm, xout, part};
      Tm.Begin("k_mc_accumulate", st);
      AccKernel()<<<G, RSBA_MT_THREADS, P.lds_acc, st>>>(aa);
      Tm.End(st);
      if (!chk("split elimination")) return RSBA_ERR_HIP;
    } else {
      ElimArgs ea{nr, P.dmax, N, chunk_ptr, time_ptr, slot_ptr, slot_col, time_full, col_full, ts, mo, obs8, intr, posec, half_side, params[x], scale_t, tdata, part, ip,
                  cs_ptr, cs_full, tconst, P.pmax};
      ElimArgsDist ead; static_cast<ElimArgs&>(ead) = ea; ead.dist = dist;
      Tm.Begin("k_time_eliminate", st);
      WithElimKernel([&](auto k, auto D) { if constexpr (D.value) k<<<G, RSBA_MT_THREADS, P.lds_elim, st>>>(ead); else k<<<G, RSBA_MT_THREADS, P.lds_elim, st>>>(ea); });
      Tm.End(st);
      if (!chk("k_time_eliminate")) return RSBA_ERR_HIP;
    }
    if (np) {
      Tm.Begin("k_mc_prior_system", st);
      k_mc_prior_system<<<1, 256, 0, st>>>(nr, prior.K, prior.full, prior.col, prior.mask, prior.ab, params[x], part + (size_t)G * PartLayout{nr}.size(), prior_pe);
      Tm.End(st);
    }
    Tm.Begin("k_marker_reduce", st);
    k_marker_reduce<<<(unsigned)((PartLayout{nr}.size() + 63) / 64), 512, 0, st>>>(nr, G + np, part, red);
    Tm.End(st);
    if (nr == 0) {
      // nothing but time blocks are free: solve_out holds the empty system's result (Upload)
    } else if (nr <= RSBA_CHOL_MAXN) {
      Tm.Begin("k_marker_reduced_solve", st);
      if (P.solve_lds) k_marker_reduced_solve_lds<<<1, 512, P.lds_solve_lds, st>>>(nr, red, A, scale_r, col_full, params[x], params[c], delta_r, solve_out, ip);
      else k_marker_reduced_solve<<<1, 512, P.lds_solve, st>>>(nr, red, A, scale_r, col_full, params[x], params[c], delta_r, solve_out, ip);
      Tm.End(st);
    } else {
      Tm.Begin("k_sys_build", st);
      k_sys_build<<<nr + 1, 256, 0, st>>>(red, RL, Wm, nullptr, nullptr, scale_r, ip, 1, ok_flag);
      Tm.End(st);
      if (P.tc_tiles > 0) {
        Tm.Begin("k_chol_tiles_persistent", st);
        k_chol_tiles_persistent<<<P.tc_tiles, 256, TileCholLdsDoubles() * sizeof(double), st>>>(
            nr, Wm, A, ok_flag, TileCholFlags{tc_flags, tc_flags + P.tc_np, tc_flags + (size_t)P.tc_np * (P.tc_nrt + 1), P.tc_nrt, tc_hand, tc_tag & 1, 0, tc_map}, tc_tag + 1, res, TileSysSource{});
        ++tc_tag;
        Tm.End(st);
      } else {
        const size_t lds_s = CholStepLdsDoubles() * sizeof(double);
        Tm.Begin("k_chol_step(all panels)", st);
        for (int kb = 0; kb < nr; kb += RSBA_PB) {
          const int r0 = kb + std::min(RSBA_PB, nr - kb);
          const int nrt = (nr + 1 - r0 + RSBA_CT - 1) / RSBA_CT;
          k_chol_step<<<nrt * (nrt + 1) / 2, 256, lds_s, st>>>(nr, kb, Wm, A, ok_flag);
        }
        Tm.End(st);
      }
      Tm.Begin("k_marker_chol_finish", st);
      k_marker_chol_finish<<<1, 1024, P.lds_finish, st>>>(nr, red, A, scale_r, col_full, params[x], params[c], delta_r, solve_out, ok_flag);
      Tm.End(st);
    }
    if (!chk("reduced solve")) return RSBA_ERR_HIP;
    Tm.Begin("k_time_backsub_terms", st);
    if (P.split_backsub) {
      if (P.nr_pose > 0) k_pose_constants_reduced<<<(P.nr_pose / 6 + 63) / 64, 64, 0, st>>>(P.nr_pose / 6, col_full, params[c], posec_c);
      if (P.with_intr) k_mc_intr_state<<<(ncams + 63) / 64, 64, 0, st>>>(ncams, nfull, params[c], intr_c, dist_c);
      Dispatch([&](auto Cn) { k_mc_time_step<Cn.value><<<(8 * T + 255) / 256, 256, 0, st>>>(T, slot_ptr, slot_col, time_full, sp, tdata, delta_r, params[x], params[c], delta_t, posec_c, bp_time, tconst); },
               P.has_const);
      // the two halves of the candidate's evaluation side by side (one after the other when every kernel is timed)
      const bool fork2 = fork_s[0] != nullptr && !Tm.enabled();
      hipStream_t s_cost = fork2 ? fork_s[0] : st;
      if (fork2 && (hipEventRecord(fork_ev[0], st) != hipSuccess || hipStreamWaitEvent(s_cost, fork_ev[0], 0) != hipSuccess)) return RSBA_ERR_HIP;
      auto candidate = [&](auto half, hipStream_t s) {   // (the weights: the cost's half only)
        constexpr int kHalf = decltype(half)::value;
        if (P.with_intr) {
          // the model cost change with the third block; the candidate's residuals at the candidate's intrinsics through the existing part 1
          if constexpr (kHalf == 0) k_mc_intr_candidate<<<P.ncand_wg, 256, 0, s>>>(N, T, ts, ti, mo, obs8, intr_x, dist_x, half_side, posec, delta_r, delta_t, blk_time, bp_time, P.with_loss ? wsq : nullptr);
          else Dispatch([&](auto L) {
            k_mc_candidate<1, L.value, true><<<P.ncand_wg, 256, 0, s>>>(N, T, ts, mo, obs8, IntrDist{intr_c, dist_c}, half_side, posec, posec_c, delta_r, delta_t, blk_time, bp_time, loss, wsq, drho_c, wts);
          }, P.with_loss);
          return;
        }
        Dispatch([&](auto L, auto D) {
          k_mc_candidate<kHalf, L.value, D.value><<<P.ncand_wg, 256, 0, s>>>(N, T, ts, mo, obs8, intr_of(D), half_side, posec, posec_c, delta_r, delta_t, blk_time, bp_time, loss, wsq, drho_c,
                                                                                    kHalf == 1 ? wts : nullptr);
        }, P.with_loss, P.with_dist);
      };
      candidate(std::integral_constant<int, 0>(), st);
      candidate(std::integral_constant<int, 1>(), s_cost);
      if (fork2 && (hipEventRecord(fork_ev[1], s_cost) != hipSuccess || hipStreamWaitEvent(st, fork_ev[1], 0) != hipSuccess)) return RSBA_ERR_HIP;
    } else if (P.backsub_wg) {
      if (nr > 0) k_pose_constants_reduced<<<(nr / 6 + 63) / 64, 64, 0, st>>>(nr / 6, col_full, params[c], posec_c);
      WithBacksubWgKernel([&](auto k, auto D) {
        k<<<T, 256, P.lds_bw, st>>>(T, time_ptr, time_full, ts, mo, obs8, intr_of(D), half_side, posec, posec_c, tdata, delta_r, params[x], params[c], delta_t, bp_time, slot_ptr, slot_col, col_full,
                                    cs_ptr, cs_full, tconst);
      });
    } else {
      Dispatch([&](auto L, auto Cn, auto D) {
        k_time_backsub_terms<L.value, Cn.value, D.value><<<nb_time, 256, 0, st>>>(T, time_ptr, time_full, ts, mo, obs8, intr_of(D), half_side, posec, tdata, delta_r, params[x], params[c], delta_t, bp_time,
                                                                                  loss, wsq, drho_c, tconst, wts);
      }, P.with_loss, P.has_const, P.with_dist);
    }
    Tm.End(st);
    const int nd = P.split_backsub ? P.ncand_wg : nb_time;
    if (np) {
      Tm.Begin("k_mc_prior_candidate", st);
      k_mc_prior_candidate<<<1, 256, 0, st>>>(prior.K, prior.full, prior.col, prior.mask, prior.ab, params[x], params[c], delta_r, prior_pe, bp_time + 4 * (size_t)nb_time, drho_c + nd);
      Tm.End(st);
    }
    Tm.Begin("k_marker_schur_finish", st);
    if (P.with_loss) k_marker_schur_finish<true><<<1, 1024, 0, st>>>(nb_time + np, bp_time, red + RL.scal(), solve_out, res, nd + np, drho_c);
    else k_marker_schur_finish<false><<<1, 1024, 0, st>>>(nb_time, bp_time, red + RL.scal(), solve_out, res);
    Tm.End(st);
    if (!chk("k_marker_schur_finish")) return RSBA_ERR_HIP;
    if (hipMemcpyAsync(res_host, res, RES_SIZE * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) return RSBA_ERR_HIP;
    { hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) { fprintf(stderr, "rsba: marker-chain step failed: %s\n", hipGetErrorString(e)); return RSBA_ERR_HIP; } }
    if (P.tc_tiles > 0 && res_host[RES_STALL] != 0.0) {
      // the tiles of the persistent factorisation were not all running side by side: the multi-launch path then
      fprintf(stderr, "rsba: persistent tiled Cholesky stalled; using the multi-launch factorisation\n");
      plan.tc_tiles = 0;
      if (hipMemset(res, 0, RES_SIZE * sizeof(double)) != hipSuccess) return RSBA_ERR_HIP;
      return Step(st, o, radius, first, res_host, Tm);
    }
    return RSBA_OK;
  }
  int SumSquares(hipStream_t st, double* out) {
    const int N = plan.N;
    if (Reset(st) != RSBA_OK) return RSBA_ERR_HIP;
    Dispatch([&](auto D) { k_marker_eval<false, D.value><<<(N + 63) / 64, 64, 0, st>>>(N, mo, obs8, params[0], IntrPass<D.value>(intr, dist), plan.half_side, 0, nullptr, nullptr, ss_x); }, plan.with_dist);
    std::vector<double> h(N);
    if (hipMemcpyAsync(h.data(), ss_x, N * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return RSBA_ERR_HIP;
    double s = 0; for (double v : h) s += v;
    *out = s;
    return RSBA_OK;
  }
  int Download(rsba_problem* p) {
    if (hipMemcpy(p->parameters.data(), params[cur], plan.nfull * 8, hipMemcpyDeviceToHost) != hipSuccess) return RSBA_ERR_HIP;
    if (plan.with_intr) {
      // the state's six values of EVERY camera into the problem's own arrays: the refined ones, and those rsba_solver_set_parameters
      // changed under the extended layout (a held component, a camera without a block).  Without such a call these keep their bits: the
      // state started from them.  A distortion array appears when the problem had none and k1 or k2 was free, or was set to non-zero
      const int C = (int)intr_mask.size();
      std::vector<double> hs(6 * (size_t)C);
      if (hipMemcpy(hs.data(), params[cur] + plan.nfull, hs.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return RSBA_ERR_HIP;
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
