// Covariance of the solved parameters (ceres::Covariance) for the point model: (J'J)^-1 of the unscaled parameters at the
// solver's current state, without any LM damping.  Runs once per rsba_solver_covariance_compute, on buffers of its own: nothing
// the LM loop reads is written here.
//
//   k_cov_lin      undamped reduced camera system S = U - sum_j W_j V_j^-1 W_j' over the FREE referenced cameras (compact index),
//                  one wavefront per point, one lane per observation, fp64 atomics (upper blocks); rank check of every V_j
//   k_cov_scale    A = D S D, D = diag(S)^-1/2 (Jacobi scaling), full symmetric, padded to whole 16-wide blocks with identity
//   k_cov_pivot    } block sweep (Gauss-Jordan on an SPD matrix): for every 16-wide block k the pivot block's Cholesky (the
//   k_cov_sweep    } rank check: the same pivots a blocked Cholesky of A meets) and its inverse, then the rank-16 update of every
//                    tile with v_mfma_f64_16x16x4_f64.  After the last block A holds -A^-1.
//   k_cov_unscale  S^-1 = -D A D, mirrored from the upper triangle, so that block (b, a) is block (a, b)' bit for bit
//   k_cov_mc_lin   marker-chain models: the normal matrix of the free camera / marker blocks (and, on the dense path, time blocks),
//                  one wavefront per time block; on the time-eliminating path every free time block is eliminated as a point is
//                  (S -= W_t V_t^-1 W_t'); with a loss (kLoss) every row's J through the solve's corrector, sqrt(rho'(s)) with s
//                  over the residual block's 8 residuals
//   k_cov_points   per point j: V_j^-1 + sum_{a,b} (W_a V_j^-1)' (S^-1)_{c_a c_b} (W_b V_j^-1), the 2x6 / 2x3 blocks recomputed
//                  in registers from the observations, written in the problem's own point order
#pragma once
#include <hip/hip_runtime.h>

#include "ba_covariance_plan.hpp"   // CovReq, COV_REQ_*, CovMcRow, RSBA_COV_MC_MAXBLK: shared with the host plan
#include "ba_math.hpp"
#include "ba_point_kernels.hpp"

namespace rsba {

#define RSBA_COV_NB 16   // block width of the sweep (one 16 x 16 MFMA tile)

enum { COV_FLAG_SYSTEM = 0, COV_FLAG_POINT = 1, COV_FLAG_WORDS = 2 };

// One observation's corrected residual Jacobian blocks (the corrector of the solve: sqrt(rho') on J, no second-order term).
__device__ __forceinline__ void CovObsJacobian(const double* __restrict__ camc, int cam, const double X[3], double u, double v, double loss,
                                               double jc[12], double jp[6]) {
  double r[2];
  ResidualJacobian(camc + (size_t)cam * CC_STRIDE, X, u, v, r, jc, jp);
  double sq;
  (void)LossAndScale(loss, r[0] * r[0] + r[1] * r[1], &sq);
  if (sq != 1.0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) jc[i] *= sq;
#pragma unroll
    for (int i = 0; i < 6; ++i) jp[i] *= sq;
  }
}

// V = Jp'Jp summed over the point's observations (symmetric 3x3 as 00 01 02 11 12 22), every lane gets the sum.
__device__ __forceinline__ void CovPointBlock(const double* __restrict__ camc, const double* __restrict__ obs_u, const double* __restrict__ obs_v,
                                              const int* __restrict__ obs_cam, int b, int k, const double X[3], double loss, int lane, double V[6]) {
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int q = lane; q < k; q += 64) {
    double jc[12], jp[6];
    CovObsJacobian(camc, obs_cam[b + q], X, obs_u[b + q], obs_v[b + q], loss, jc, jp);
    acc[0] += jp[0] * jp[0] + jp[3] * jp[3]; acc[1] += jp[0] * jp[1] + jp[3] * jp[4]; acc[2] += jp[0] * jp[2] + jp[3] * jp[5];
    acc[3] += jp[1] * jp[1] + jp[4] * jp[4]; acc[4] += jp[1] * jp[2] + jp[4] * jp[5]; acc[5] += jp[2] * jp[2] + jp[5] * jp[5];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) V[i] = WaveSum(acc[i]);
}

// Inverse of a point block with the rank test of the reduced system: the Cholesky pivots of the Jacobi-scaled block must exceed
// rcond (its largest diagonal entry is 1).  false: rank deficient (Vi is then zero).
__device__ __forceinline__ bool CovPointInverse(const double V[6], double rcond, double Vi[6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) Vi[i] = 0.0;
  if (!(V[0] > 0.0) || !(V[3] > 0.0) || !(V[5] > 0.0)) return false;
  const double s[3] = {1.0 / sqrt(V[0]), 1.0 / sqrt(V[3]), 1.0 / sqrt(V[5])};
  const double m01 = s[0] * s[1] * V[1], m02 = s[0] * s[2] * V[2], m12 = s[1] * s[2] * V[4];
  const double l10 = m01, l20 = m02;
  const double d11 = 1.0 - l10 * l10;
  if (!(d11 > rcond)) return false;
  const double l11 = sqrt(d11), i11 = 1.0 / l11;
  const double l21 = (m12 - l20 * l10) * i11;
  const double d22 = 1.0 - l20 * l20 - l21 * l21;
  if (!(d22 > rcond)) return false;
  const double i22 = 1.0 / sqrt(d22);
  const double a10 = -l10 * i11, a20 = -(l20 + l21 * a10) * i22, a21 = -l21 * i11 * i22;
  Vi[0] = s[0] * s[0] * (1.0 + a10 * a10 + a20 * a20);
  Vi[1] = s[0] * s[1] * (a10 * i11 + a20 * a21);
  Vi[2] = s[0] * s[2] * (a20 * i22);
  Vi[3] = s[1] * s[1] * (i11 * i11 + a21 * a21);
  Vi[4] = s[1] * s[2] * (a21 * i22);
  Vi[5] = s[2] * s[2] * (i22 * i22);
  return true;
}

// Y = W Vi, W = Jc'Jp (6x3)
__device__ __forceinline__ void CovWY(const double jc[12], const double jp[6], const double Vi[6], double W[18], double Y[18]) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) W[3 * a + c] = jc[a] * jp[c] + jc[6 + a] * jp[3 + c];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    Y[3 * a + 0] = W[3 * a] * Vi[0] + W[3 * a + 1] * Vi[1] + W[3 * a + 2] * Vi[2];
    Y[3 * a + 1] = W[3 * a] * Vi[1] + W[3 * a + 1] * Vi[3] + W[3 * a + 2] * Vi[4];
    Y[3 * a + 2] = W[3 * a] * Vi[2] + W[3 * a + 1] * Vi[4] + W[3 * a + 2] * Vi[5];
  }
}

// S (n x n, zeroed by the caller) += U - W V^-1 W' into the upper blocks; cam_pos[c] = 6 x (compact index) or -1 (constant or
// unreferenced camera: no columns).  Observations are walked in chunks of 64 (any number of views per point).
__global__ void __launch_bounds__(256)
k_cov_lin(int P, const double* __restrict__ obs_u, const double* __restrict__ obs_v, const int* __restrict__ obs_cam, const int* __restrict__ pt_ptr,
          const double* __restrict__ camc, const double* __restrict__ pts, const int* __restrict__ cam_pos, const unsigned char* __restrict__ pt_const,
          double loss, double rcond, int n, double* __restrict__ S, int* __restrict__ flags) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  for (int j = blockIdx.x * nwave + wave; j < P; j += gridDim.x * nwave) {
    const int b = pt_ptr[j], k = pt_ptr[j + 1] - b;
    if (k == 0) continue;
    const double X[3] = {pts[3 * (size_t)j], pts[3 * (size_t)j + 1], pts[3 * (size_t)j + 2]};
    const bool pconst = pt_const != nullptr && pt_const[j] != 0;
    // U = Jc'Jc of every observation into its camera's diagonal block
    for (int q = lane; q < k; q += 64) {
      const int cam = obs_cam[b + q], pa = cam_pos[cam];
      if (pa < 0) continue;
      double jc[12], jp[6];
      CovObsJacobian(camc, cam, X, obs_u[b + q], obs_v[b + q], loss, jc, jp);
      double* Sb = S + (size_t)pa * n + pa;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = a; c < 6; ++c) unsafeAtomicAdd(&Sb[(size_t)a * n + c], jc[a] * jc[c] + jc[6 + a] * jc[6 + c]);
    }
    if (pconst) continue;   // a constant point has no columns: nothing to eliminate
    double V[6], Vi[6];
    CovPointBlock(camc, obs_u, obs_v, obs_cam, b, k, X, loss, lane, V);
    if (!CovPointInverse(V, rcond, Vi)) {
      if (lane == 0) atomicOr(&flags[COV_FLAG_POINT], 1);
      continue;
    }
    // -Y_a W_b' for every pair of observations whose cameras are free, into the upper block (pos_a <= pos_b)
    for (int qa0 = 0; qa0 < k; qa0 += 64) {
      const int qa = qa0 + lane;
      const bool acta = qa < k;
      int pa = -1;
      double Ya[18], Wa[18];
#pragma unroll
      for (int i = 0; i < 18; ++i) { Ya[i] = 0.0; Wa[i] = 0.0; }
      if (acta) {
        const int cam = obs_cam[b + qa];
        pa = cam_pos[cam];
        double jc[12], jp[6];
        CovObsJacobian(camc, cam, X, obs_u[b + qa], obs_v[b + qa], loss, jc, jp);
        CovWY(jc, jp, Vi, Wa, Ya);
      }
      for (int qb0 = 0; qb0 < k; qb0 += 64) {
        int pb = -1;
        double Wb[18];
        if (qb0 == qa0) {
          pb = pa;
#pragma unroll
          for (int i = 0; i < 18; ++i) Wb[i] = Wa[i];
        } else {
          const int qb = qb0 + lane;
#pragma unroll
          for (int i = 0; i < 18; ++i) Wb[i] = 0.0;
          if (qb < k) {
            const int cam = obs_cam[b + qb];
            pb = cam_pos[cam];
            double jc[12], jp[6], Yb[18];
            CovObsJacobian(camc, cam, X, obs_u[b + qb], obs_v[b + qb], loss, jc, jp);
            CovWY(jc, jp, Vi, Wb, Yb);
          }
        }
        const int nb = min(64, k - qb0);
        for (int bb = 0; bb < nb; ++bb) {
          const int pbb = __shfl(pb, bb, 64);
          double w[18];
#pragma unroll
          for (int i = 0; i < 18; ++i) w[i] = __shfl(Wb[i], bb, 64);
          if (pa < 0 || pbb < 0 || pa > pbb) continue;
          double* Sb = S + (size_t)pa * n + pbb;
#pragma unroll
          for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
              if (pa == pbb && c < a) continue;   // diagonal blocks: upper triangle only
              unsafeAtomicAdd(&Sb[(size_t)a * n + c], -(Ya[3 * a] * w[3 * c] + Ya[3 * a + 1] * w[3 * c + 1] + Ya[3 * a + 2] * w[3 * c + 2]));
            }
        }
      }
    }
  }
}

// A sharded solver adds its partial S to the other ranks': the upper triangle row by row, n (n + 1) / 2 values, and behind it one
// more, 1.0 when a point block of this shard was rank deficient (the all-ranks sum counts the shards that met one).
__device__ __forceinline__ size_t CovTriIndex(int n, int i, int j) { return (size_t)i * n - (size_t)i * (i - 1) / 2 + (size_t)(j - i); }   // i <= j

__global__ void __launch_bounds__(256) k_cov_tri_pack(int n, const double* __restrict__ S, const int* __restrict__ flags, double* __restrict__ tri) {
  const size_t nn = (size_t)n * n;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e <= nn; e += (size_t)gridDim.x * blockDim.x) {
    if (e == nn) { tri[(size_t)n * (n + 1) / 2] = flags[COV_FLAG_POINT] != 0 ? 1.0 : 0.0; continue; }
    const int i = (int)(e / n), j = (int)(e - (size_t)i * n);
    if (i <= j) tri[CovTriIndex(n, i, j)] = S[e];
  }
}

// ... and the sums back into the upper triangle of S (all that k_cov_scale reads) and into the point flag.
__global__ void __launch_bounds__(256) k_cov_tri_unpack(int n, const double* __restrict__ tri, double* __restrict__ S, int* __restrict__ flags) {
  const size_t nn = (size_t)n * n;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e <= nn; e += (size_t)gridDim.x * blockDim.x) {
    if (e == nn) { flags[COV_FLAG_POINT] = tri[(size_t)n * (n + 1) / 2] > 0.0 ? 1 : 0; continue; }
    const int i = (int)(e / n), j = (int)(e - (size_t)i * n);
    if (i <= j) S[e] = tri[CovTriIndex(n, i, j)];
  }
}

// A (np x np) = D S D from the upper triangle of S, identity in the padding; dscale[i] = S_ii^-1/2.  A zero or negative diagonal is
// a rank deficiency (flag), the row is then scaled by 1 so that no NaN enters the sweep.
__global__ void __launch_bounds__(256) k_cov_scale(int n, int np, const double* __restrict__ S, double* __restrict__ A, double* __restrict__ dscale,
                                                   int* __restrict__ flags) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)np * np; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / np), j = (int)(e - (size_t)i * np);
    if (i >= n || j >= n) { A[e] = i == j ? 1.0 : 0.0; continue; }
    const double sii = S[(size_t)i * n + i], sjj = S[(size_t)j * n + j];
    const double di = sii > 0.0 ? 1.0 / sqrt(sii) : 1.0, dj = sjj > 0.0 ? 1.0 / sqrt(sjj) : 1.0;
    A[e] = (i <= j ? S[(size_t)i * n + j] : S[(size_t)j * n + i]) * di * dj;
    if (i == j) {
      dscale[i] = di;
      if (!(sii > 0.0)) atomicOr(&flags[COV_FLAG_SYSTEM], 1);
    }
  }
}

// Sweep step, part 1 (one workgroup of 64): the pivot block's Cholesky with the rank test, D = pivot^-1 into piv[0..255], and the
// block column k of A (np x 16, before the update) into panel.  A failed pivot raises the flag and leaves D = 0.
__global__ void __launch_bounds__(64) k_cov_pivot(int np, int kb, const double* __restrict__ A, double* __restrict__ piv, double* __restrict__ panel,
                                                  double rcond, int* __restrict__ flags) {
  __shared__ double L[RSBA_COV_NB][RSBA_COV_NB + 1], Li[RSBA_COV_NB][RSBA_COV_NB + 1];
  __shared__ int bad;
  const int t = threadIdx.x, k0 = kb * RSBA_COV_NB;
  for (int e = t; e < np * RSBA_COV_NB; e += 64) {
    const int r = e / RSBA_COV_NB, c = e - r * RSBA_COV_NB;
    panel[e] = A[(size_t)r * np + k0 + c];
  }
  for (int e = t; e < RSBA_COV_NB * RSBA_COV_NB; e += 64) {
    const int r = e / RSBA_COV_NB, c = e - r * RSBA_COV_NB;
    L[r][c] = A[(size_t)(k0 + r) * np + k0 + c];
    Li[r][c] = 0.0;
  }
  if (t == 0) bad = 0;
  __syncthreads();
  // column-by-column Cholesky: lanes own rows
  for (int c = 0; c < RSBA_COV_NB; ++c) {
    if (t == 0) {
      const double d = L[c][c];
      if (!(d > rcond)) bad = 1;
      L[c][c] = d > 0.0 ? sqrt(d) : 1.0;
    }
    __syncthreads();
    if (t > c && t < RSBA_COV_NB) L[t][c] /= L[c][c];
    __syncthreads();
    if (t > c && t < RSBA_COV_NB)
      for (int c2 = c + 1; c2 <= t; ++c2) L[t][c2] -= L[t][c] * L[c2][c];
    __syncthreads();
  }
  // Li = L^-1 (lower), one column per lane
  if (t < RSBA_COV_NB) {
    for (int r = t; r < RSBA_COV_NB; ++r) {
      double v = r == t ? 1.0 : 0.0;
      for (int m = t; m < r; ++m) v -= L[r][m] * Li[m][t];
      Li[r][t] = v / L[r][r];
    }
  }
  __syncthreads();
  // D = Li' Li
  for (int e = t; e < RSBA_COV_NB * RSBA_COV_NB; e += 64) {
    const int r = e / RSBA_COV_NB, c = e - r * RSBA_COV_NB;
    double v = 0.0;
    for (int m = max(r, c); m < RSBA_COV_NB; ++m) v += Li[m][r] * Li[m][c];
    piv[e] = bad ? 0.0 : v;
  }
  if (t == 0 && bad) atomicOr(&flags[COV_FLAG_SYSTEM], 1);
}

typedef double cov_d4_t __attribute__((ext_vector_type(4)));

// 16 x 16 product of a 16 x 16 fragment pair with v_mfma_f64_16x16x4_f64: acc += X Y, X and Y read from row-major 16 x 16 tiles
// with leading dimensions ldx / ldy (Xt: X is read transposed).  Operand maps: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]
// of each k-step; the result's register i of lane l is row (l >> 4) + 4 i, column l & 15.
template <bool kXt>
__device__ __forceinline__ cov_d4_t CovMfma16(const double* __restrict__ Xp, int ldx, const double* __restrict__ Yp, int ldy, cov_d4_t acc, int lane) {
  const int r = lane & 15, kk = lane >> 4;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const double a = kXt ? Xp[(size_t)(4 * s + kk) * ldx + r] : Xp[(size_t)r * ldx + 4 * s + kk];
    const double b = Yp[(size_t)(4 * s + kk) * ldy + r];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// Sweep step, part 2: one wavefront per 16 x 16 tile (bi, bj) of A, from the panel (block column k before the step) and D:
//   Q_i = panel_i D;  bi, bj != k: A_ij -= Q_i panel_j';  A_ik = Q_i;  A_kj = Q_j';  A_kk = -D
__global__ void __launch_bounds__(64) k_cov_sweep(int np, int kb, double* __restrict__ A, const double* __restrict__ piv, const double* __restrict__ panel) {
  __shared__ double Q[RSBA_COV_NB * RSBA_COV_NB], Qj[RSBA_COV_NB * RSBA_COV_NB];
  const int nb = np / RSBA_COV_NB, bi = blockIdx.x / nb, bj = blockIdx.x - bi * nb, lane = threadIdx.x;
  const int rr = lane >> 4, cc = lane & 15;
  double* Aij = A + (size_t)bi * RSBA_COV_NB * np + (size_t)bj * RSBA_COV_NB;
  if (bi == kb && bj == kb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) Aij[(size_t)(rr + 4 * i) * np + cc] = -piv[(rr + 4 * i) * RSBA_COV_NB + cc];
    return;
  }
  const double* Pi = panel + (size_t)bi * RSBA_COV_NB * RSBA_COV_NB;
  const double* Pj = panel + (size_t)bj * RSBA_COV_NB * RSBA_COV_NB;
  cov_d4_t z = {0.0, 0.0, 0.0, 0.0};
  if (bj == kb) {   // A_ik = panel_i D
    const cov_d4_t q = CovMfma16<false>(Pi, RSBA_COV_NB, piv, RSBA_COV_NB, z, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) Aij[(size_t)(rr + 4 * i) * np + cc] = q[i];
    return;
  }
  if (bi == kb) {   // A_kj = D panel_j' = (panel_j D)'
    const cov_d4_t q = CovMfma16<false>(Pj, RSBA_COV_NB, piv, RSBA_COV_NB, z, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) Aij[(size_t)cc * np + rr + 4 * i] = q[i];
    return;
  }
  const cov_d4_t q = CovMfma16<false>(Pi, RSBA_COV_NB, piv, RSBA_COV_NB, z, lane);
#pragma unroll
  for (int i = 0; i < 4; ++i) Q[(rr + 4 * i) * RSBA_COV_NB + cc] = q[i];
  // panel_j' as a row-major tile: Qj[m][c] = panel_j[c][m]
  for (int e = lane; e < RSBA_COV_NB * RSBA_COV_NB; e += 64) { const int m = e >> 4, c = e & 15; Qj[e] = Pj[c * RSBA_COV_NB + m]; }
  __syncthreads();
  const cov_d4_t u = CovMfma16<false>(Q, RSBA_COV_NB, Qj, RSBA_COV_NB, z, lane);
#pragma unroll
  for (int i = 0; i < 4; ++i) Aij[(size_t)(rr + 4 * i) * np + cc] -= u[i];
}

// S^-1 (n x n, full symmetric) = -D A D with A = -(DSD)^-1 from the sweep, every entry taken from the upper triangle
__global__ void __launch_bounds__(256) k_cov_unscale(int n, int np, const double* __restrict__ A, const double* __restrict__ dscale, double* __restrict__ Sinv) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)n * n; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / n), j = (int)(e - (size_t)i * n);
    const int a = min(i, j), b = max(i, j);
    Sinv[e] = -(A[(size_t)a * np + b] * dscale[a]) * dscale[b];
  }
}

// Point marginals: out[perm[j]] (9 doubles, row-major 3x3) = V_j^-1 + sum_{a,b} Y_a' (S^-1)_{c_a c_b} Y_b, Y = W V_j^-1; zeros for a
// constant or unreferenced point.  One wavefront per point; lane a takes observation a of each chunk, observation b's Y is broadcast.
__global__ void __launch_bounds__(256)
k_cov_points(int P, const double* __restrict__ obs_u, const double* __restrict__ obs_v, const int* __restrict__ obs_cam, const int* __restrict__ pt_ptr,
             const double* __restrict__ camc, const double* __restrict__ pts, const int* __restrict__ cam_pos, const unsigned char* __restrict__ pt_const,
             const int* __restrict__ perm, double loss, double rcond, int n, const double* __restrict__ Sinv, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  for (int j = blockIdx.x * nwave + wave; j < P; j += gridDim.x * nwave) {
    const int b = pt_ptr[j], k = pt_ptr[j + 1] - b;
    double* o = out + 9 * (size_t)(perm != nullptr ? perm[j] : j);
    if (k == 0 || (pt_const != nullptr && pt_const[j] != 0)) {
      if (lane < 9) o[lane] = 0.0;
      continue;
    }
    const double X[3] = {pts[3 * (size_t)j], pts[3 * (size_t)j + 1], pts[3 * (size_t)j + 2]};
    double V[6], Vi[6];
    CovPointBlock(camc, obs_u, obs_v, obs_cam, b, k, X, loss, lane, V);
    (void)CovPointInverse(V, rcond, Vi);   // (k_cov_lin has already raised the flag for a singular block)
    double acc[6] = {0, 0, 0, 0, 0, 0};   // 00 01 02 11 12 22
    for (int qa0 = 0; qa0 < k; qa0 += 64) {
      const int qa = qa0 + lane;
      int pa = -1;
      double Ya[18];
#pragma unroll
      for (int i = 0; i < 18; ++i) Ya[i] = 0.0;
      if (qa < k) {
        const int cam = obs_cam[b + qa];
        pa = cam_pos[cam];
        double jc[12], jp[6], W[18];
        CovObsJacobian(camc, cam, X, obs_u[b + qa], obs_v[b + qa], loss, jc, jp);
        CovWY(jc, jp, Vi, W, Ya);
      }
      for (int qb0 = 0; qb0 < k; qb0 += 64) {
        int pb = -1;
        double Yb[18];
        if (qb0 == qa0) {
          pb = pa;
#pragma unroll
          for (int i = 0; i < 18; ++i) Yb[i] = Ya[i];
        } else {
          const int qb = qb0 + lane;
#pragma unroll
          for (int i = 0; i < 18; ++i) Yb[i] = 0.0;
          if (qb < k) {
            const int cam = obs_cam[b + qb];
            pb = cam_pos[cam];
            double jc[12], jp[6], W[18];
            CovObsJacobian(camc, cam, X, obs_u[b + qb], obs_v[b + qb], loss, jc, jp);
            CovWY(jc, jp, Vi, W, Yb);
          }
        }
        const int nb = min(64, k - qb0);
        for (int bb = 0; bb < nb; ++bb) {
          const int pbb = __shfl(pb, bb, 64);
          double y[18];
#pragma unroll
          for (int i = 0; i < 18; ++i) y[i] = __shfl(Yb[i], bb, 64);
          if (pa < 0 || pbb < 0) continue;
          // Z = (S^-1)_{ab} Y_b (6x3), then acc += Y_a' Z
          const double* Sb = Sinv + (size_t)pa * n + pbb;
          double Z[18];
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            double s6[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) s6[c] = Sb[(size_t)r * n + c];
#pragma unroll
            for (int c3 = 0; c3 < 3; ++c3) {
              double v = 0.0;
#pragma unroll
              for (int c = 0; c < 6; ++c) v += s6[c] * y[3 * c + c3];
              Z[3 * r + c3] = v;
            }
          }
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            acc[0] += Ya[3 * r] * Z[3 * r];     acc[1] += Ya[3 * r] * Z[3 * r + 1];     acc[2] += Ya[3 * r] * Z[3 * r + 2];
            acc[3] += Ya[3 * r + 1] * Z[3 * r + 1]; acc[4] += Ya[3 * r + 1] * Z[3 * r + 2]; acc[5] += Ya[3 * r + 2] * Z[3 * r + 2];
          }
        }
      }
    }
    double m[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) m[i] = WaveSum(acc[i]) + Vi[i];
    if (lane == 0) {
      o[0] = m[0]; o[1] = m[1]; o[2] = m[2];
      o[3] = m[1]; o[4] = m[3]; o[5] = m[4];
      o[6] = m[2]; o[7] = m[4]; o[8] = m[5];
    }
  }
}


// ---- marker-chain models ------------------------------------------------------------------------------------------------
// (CovMcRow, a row of the marker-chain problem in time order: ba_covariance_plan.hpp)

// pose constants (CC_R, CC_K, CC_T, CC_SMALL) of every block of [C | T | M]
__global__ void __launch_bounds__(256) k_cov_pose_constants(int nb, const double* __restrict__ params, double* __restrict__ pc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  const double zero4[4] = {0.0, 0.0, 0.0, 0.0};
  double cc[CC_STRIDE];
  CameraConstants(params + 6 * (size_t)i, zero4, cc);
#pragma unroll
  for (int e = 0; e < CC_STRIDE; ++e) pc[(size_t)i * CC_STRIDE + e] = cc[e];
}

// Inverse of a symmetric 6 x 6 block (upper 21: row-major upper triangle) with the rank test of CovPointInverse.  false: rank deficient.
__device__ __forceinline__ bool CovSym6Inverse(const double U[21], double rcond, double Vi[36]) {
  double M[6][6], s[6];
  int t = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = a; c < 6; ++c) { M[a][c] = U[t]; M[c][a] = U[t]; ++t; }
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 6; ++a) { ok = ok && M[a][a] > 0.0; s[a] = M[a][a] > 0.0 ? 1.0 / sqrt(M[a][a]) : 1.0; }
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 6; ++c) M[a][c] *= s[a] * s[c];
  // Cholesky in place (lower), then L^-1 in place of the upper part's mirror
  double L[6][6];
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 6; ++c) L[a][c] = 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double d = M[c][c];
#pragma unroll
    for (int m = 0; m < c; ++m) d -= L[c][m] * L[c][m];
    ok = ok && d > rcond;
    L[c][c] = d > 0.0 ? sqrt(d) : 1.0;
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      double v = M[r][c];
#pragma unroll
      for (int m = 0; m < c; ++m) v -= L[r][m] * L[c][m];
      L[r][c] = v / L[c][c];
    }
  }
  double Li[6][6];
#pragma unroll
  for (int c = 0; c < 6; ++c)
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      if (r < c) { Li[r][c] = 0.0; continue; }
      double v = r == c ? 1.0 : 0.0;
#pragma unroll
      for (int m = c; m < r; ++m) v -= L[r][m] * Li[m][c];
      Li[r][c] = v / L[r][r];
    }
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double v = 0.0;
#pragma unroll
      for (int m = 0; m < 6; ++m) v += Li[m][a] * Li[m][c];
      Vi[6 * a + c] = ok ? v * s[a] * s[c] : 0.0;
    }
  return ok;
}

#define RSBA_COV_MC_LDS 73   // doubles per row of the staged W blocks: cam 6x6 | marker 6x6 (+1: bank padding)

// Constant components of partly constant blocks (ceres::SubsetParameterization; the kSub instances below).  sub18[q]: the constant
// components among row q's 18 local columns camera | time | marker (rows in the compute's order; 0 for a block without columns).
// Ceres evaluates such a block through its 6 x (6 - k) local Jacobian, inverts the system of the free components and lifts the result
// back with zeros.  Here: the rows' constant columns are set to exact zeros where the rows are formed, every constant component gets
// a unit diagonal (in V_t and, by k_cov_subset_diag, in S) — decoupled from the free ones, so the inverse of the rest is that of the
// system without it and no rank deficiency is reported because of it — and its rows and columns of the result are written as exact
// zeros (k_cov_subset_sinv for S^-1; k_cov_mc_cross for the blocks it forms).
// The masks travel in the argument that carries the intrinsics, so the instances without them keep the signature they had.
struct IntrDistSub : IntrDist { const int* sub18; };
template <bool kDist, bool kSub> struct CovIntrArg { typedef typename IntrArg<kDist>::type type; };
template <bool kDist> struct CovIntrArg<kDist, true> { typedef IntrDistSub type; };
__device__ __forceinline__ int SubOf(const double*, int) { return 0; }
__device__ __forceinline__ int SubOf(const IntrDist&, int) { return 0; }
__device__ __forceinline__ int SubOf(const IntrDistSub& a, int q) { return a.sub18[q]; }
// the constant columns of one corner's 2 x 18 rows
__device__ __forceinline__ void SubsetZeroColumns(int sub, double J[36]) {
#pragma unroll
  for (int e = 0; e < 36; ++e) if ((sub >> (e % 18)) & 1) J[e] = 0.0;
}
// the unit diagonal of a time's constant components in the upper triangle V (rows a, columns c >= a, row by row)
__device__ __forceinline__ void SubsetUnitDiagonal(int sub6, double V[21]) {
#pragma unroll
  for (int a = 0; a < 6; ++a) if ((sub6 >> a) & 1) V[6 * a - a * (a - 1) / 2] = 1.0;
}
// S (n x n, upper blocks, before the inverse): a one on the diagonal of every constant component.  bsub[b]: block b's mask.
__global__ void __launch_bounds__(256) k_cov_subset_diag(int nb, const int* __restrict__ pos, const unsigned char* __restrict__ bsub, int n, double* __restrict__ S) {
  const int g = blockIdx.x * 256 + threadIdx.x, b = g / 6, q = g - 6 * b;
  if (b >= nb || pos[b] < 0 || !((bsub[b] >> q) & 1)) return;
  const size_t i = (size_t)pos[b] + q;
  S[i * n + i] = 1.0;
}
// The priors of a marker-chain solver (PriorDevice): S += A~'A~ on the diagonal 6 x 6 of every prior block with columns in S, behind
// k_cov_mc_lin and in front of k_cov_subset_diag / the scaling.  A~: A without the columns of the block's constant components.
// Thread per entry; a block carries at most one prior, so no two threads meet.
__global__ void __launch_bounds__(256) k_cov_prior(int K, const int* __restrict__ full, const int* __restrict__ mask, const double* __restrict__ ab,
                                                   const int* __restrict__ pos, int n, double* __restrict__ S) {
  const int e = blockIdx.x * 256 + threadIdx.x, k = e / 36, a = (e - 36 * k) / 6, c = (e - 36 * k) % 6;
  if (k >= K) return;
  const int p0 = pos[full[k] / 6];
  if (p0 < 0 || ((mask[k] >> a) & 1) || ((mask[k] >> c) & 1)) return;
  double h = 0.0;
  for (int i = 0; i < 6; ++i) h += ab[42 * (size_t)k + 6 * i + a] * ab[42 * (size_t)k + 6 * i + c];
  S[(size_t)(p0 + a) * n + (p0 + c)] += h;
}
// S^-1: the rows and columns of the constant components as exact zeros (workgroup per block)
__global__ void __launch_bounds__(256) k_cov_subset_sinv(const int* __restrict__ pos, const unsigned char* __restrict__ bsub, int n, double* __restrict__ Sinv) {
  const int b = blockIdx.x, sub = bsub[b];
  if (pos[b] < 0 || sub == 0) return;
  for (int q = 0; q < 6; ++q) {
    if (!((sub >> q) & 1)) continue;
    const size_t i = (size_t)pos[b] + q;
    for (int j = threadIdx.x; j < n; j += 256) { Sinv[i * n + j] = 0.0; Sinv[(size_t)j * n + i] = 0.0; }
  }
}

// Normal matrix of the marker-chain problem into S (n x n, zeroed by the caller, upper blocks): one wavefront per time block,
// one lane per row (chunks of 64).  pos[block] = 6 x compact index or -1 (constant / unreferenced / eliminated).  elim[t] != 0:
// time block t is eliminated — S -= W_x V_t^-1 W_y' over the pairs of its rows' camera / marker blocks, W_x = sum J_x'J_t.
// kLoss: J of a row scaled by sqrt(rho'(s)) (loss: LossAndScale's signed parameter), s taken over its four corners first; wts
// (nullptr: none): the rows' weights a_q (ceres::ScaledLoss) in the rows' order, the factor sqrt(a_q) sqrt(rho').
// kDist: dist = the cameras' five distortion coefficients [C][5], indexed as intr.
// kSub: the rows' constant columns are zeros and V_t has a unit diagonal there (see IntrDistSub above; S gets its own from
// k_cov_subset_diag).
template <bool kLoss, bool kDist = false, bool kSub = false>
__global__ void __launch_bounds__(64)
k_cov_mc_lin(int T, const int* __restrict__ tptr, const CovMcRow* __restrict__ rows, const double* __restrict__ obs8, typename CovIntrArg<kDist, kSub>::type intr,
             const double* __restrict__ pc, const int* __restrict__ pos, const unsigned char* __restrict__ elim, double half_side, double rcond,
             int n, double* __restrict__ S, int* __restrict__ flags, double loss = 0.0, const double* __restrict__ wts = nullptr) {
  __shared__ double Wl[64 * RSBA_COV_MC_LDS];
  __shared__ int Pl[64][2];
  const int lane = threadIdx.x;
  const double cx[4] = {-half_side, half_side, half_side, -half_side};
  const double cy[4] = {half_side, half_side, -half_side, -half_side};
  // one row's four corners: J (2 x 18 each) through f(corner, J)
  auto corners = [&](int q, auto&& f) {
    const CovMcRow rw = rows[q];
    const double* o8 = obs8 + 8 * (size_t)q;
    const double* pcc = rw.cam_block >= 0 ? pc + (size_t)rw.cam_block * CC_STRIDE : nullptr;
    const double* pcm = rw.marker_block >= 0 ? pc + (size_t)rw.marker_block * CC_STRIDE : nullptr;
    double sq = 1.0;
    if constexpr (kLoss) {
      double ss = 0.0;
      for (int k = 0; k < 4; ++k) {
        double r[2], J[36];
        MarkerCornerResidualJacobian<kDist>(pcc, pc + (size_t)rw.time_block * CC_STRIDE, pcm, IntrOf(intr) + 4 * rw.camera, cx[k], cy[k], o8[2 * k], o8[2 * k + 1], r, J, DistOf(intr, rw.camera));
        ss += r[0] * r[0] + r[1] * r[1];
      }
      (void)LossAndScale(loss, ss, &sq);
      if (wts != nullptr) sq *= sqrt(wts[q]);
    }
    for (int k = 0; k < 4; ++k) {
      double r[2], J[36];
      MarkerCornerResidualJacobian<kDist>(pcc, pc + (size_t)rw.time_block * CC_STRIDE, pcm, IntrOf(intr) + 4 * rw.camera, cx[k], cy[k], o8[2 * k], o8[2 * k + 1], r, J, DistOf(intr, rw.camera));
      if constexpr (kLoss) {
        for (int e = 0; e < 36; ++e) J[e] *= sq;
      }
      if constexpr (kSub) SubsetZeroColumns(SubOf(intr, q), J);
      f(J);
    }
  };
  // stage W_cam, W_marker (= sum over corners of J_x' J_t) of row q into this lane's LDS row, with the blocks' positions
  auto stage = [&](int q, bool act) {
    double* w = Wl + lane * RSBA_COV_MC_LDS;
    for (int e = 0; e < 72; ++e) w[e] = 0.0;
    Pl[lane][0] = -1; Pl[lane][1] = -1;
    if (!act) return;
    const CovMcRow rw = rows[q];
    Pl[lane][0] = rw.cam_block >= 0 ? pos[rw.cam_block] : -1;
    Pl[lane][1] = rw.marker_block >= 0 ? pos[rw.marker_block] : -1;
    corners(q, [&](const double* J) {
      for (int x = 0; x < 2; ++x) {
        const int xo = x == 0 ? 0 : 12;
        for (int a = 0; a < 6; ++a)
          for (int l = 0; l < 6; ++l) w[36 * x + 6 * a + l] += J[xo + a] * J[6 + l] + J[18 + xo + a] * J[18 + 6 + l];
      }
    });
  };
  for (int t = blockIdx.x; t < T; t += gridDim.x) {
    const int b = tptr[t], k = tptr[t + 1] - b;
    if (k == 0) continue;
    const bool el = elim[t] != 0;
    double V[21];
#pragma unroll
    for (int e = 0; e < 21; ++e) V[e] = 0.0;
    // J'J of every row among its blocks that have columns (upper blocks), V_t for an eliminated time
    for (int q = lane; q < k; q += 64) {
      const CovMcRow rw = rows[b + q];
      const int blk[3] = {rw.cam_block, rw.time_block, rw.marker_block};
      int ps[3];
      for (int x = 0; x < 3; ++x) ps[x] = blk[x] >= 0 ? pos[blk[x]] : -1;
      corners(b + q, [&](const double* J) {
        for (int x = 0; x < 3; ++x)
          for (int y = 0; y < 3; ++y) {
            if (ps[x] < 0 || ps[y] < 0 || ps[x] > ps[y] || (ps[x] == ps[y] && x != y)) continue;
            double* Sb = S + (size_t)ps[x] * n + ps[y];
            for (int a = 0; a < 6; ++a)
              for (int c = (x == y ? a : 0); c < 6; ++c)
                unsafeAtomicAdd(&Sb[(size_t)a * n + c], J[6 * x + a] * J[6 * y + c] + J[18 + 6 * x + a] * J[18 + 6 * y + c]);
          }
        if (el) {
          int e = 0;
          for (int a = 0; a < 6; ++a)
            for (int c = a; c < 6; ++c) { V[e] += J[6 + a] * J[6 + c] + J[24 + a] * J[24 + c]; ++e; }
        }
      });
    }
    if (!el) continue;
#pragma unroll
    for (int e = 0; e < 21; ++e) V[e] = WaveSum(V[e]);
    if constexpr (kSub) SubsetUnitDiagonal((SubOf(intr, b) >> 6) & 63, V);
    double Vi[36];
    if (!CovSym6Inverse(V, rcond, Vi)) {
      if (lane == 0) atomicOr(&flags[COV_FLAG_POINT], 1);
      continue;
    }
    for (int qa0 = 0; qa0 < k; qa0 += 64) {
      __syncthreads();
      stage(b + qa0 + lane, qa0 + lane < k);
      __syncthreads();
      // Y_x = W_x V_t^-1 of this lane's row
      double Y[72];
      const double* w = Wl + lane * RSBA_COV_MC_LDS;
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int l = 0; l < 6; ++l) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) v += w[36 * x + 6 * a + m] * Vi[6 * m + l];
            Y[36 * x + 6 * a + l] = v;
          }
      const int pa[2] = {Pl[lane][0], Pl[lane][1]};
      for (int qb0 = 0; qb0 < k; qb0 += 64) {
        __syncthreads();
        stage(b + qb0 + lane, qb0 + lane < k);
        __syncthreads();
        const int nbq = min(64, k - qb0);
        for (int bb = 0; bb < nbq; ++bb) {
          const double* wb = Wl + bb * RSBA_COV_MC_LDS;
#pragma unroll
          for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) {
              const int px = pa[x], py = Pl[bb][y];
              if (px < 0 || py < 0 || px > py) continue;
              double* Sb = S + (size_t)px * n + py;
#pragma unroll
              for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                  if (px == py && c < a) continue;
                  double v = 0.0;
#pragma unroll
                  for (int l = 0; l < 6; ++l) v += Y[36 * x + 6 * a + l] * wb[36 * y + 6 * c + l];
                  unsafeAtomicAdd(&Sb[(size_t)a * n + c], -v);
                }
            }
        }
      }
    }
  }
}

#define RSBA_COV_MCI_LDS 109   // doubles per row of the staged W blocks: cam 6x6 | marker 6x6 | intrinsics 6x6 (+1: bank padding)

// k_cov_mc_lin for a solver with free intrinsics under the extended layout: a row has a fourth block, the detecting camera's
// fx fy cx cy k1 k2 (block nb + camera of pos; the base camera has one too), rows of 2 x 24 per corner — MarkerCornerResidualJacobian<true>'s
// 18 columns and the six analytic ones (MarkerCornerIntrinsicsTerms).  six: the compute's snapshot of the state's values, [C][6];
// dist: the path's coefficients [C][5], of which p1 p2 k3 are read.  One instance: the corrector and the weights are applied when
// loss != 0 or wts != nullptr (a factor of exactly one otherwise), the masks always travel — sub24[q]: the constant components among
// row q's 24 local columns camera | time | marker | intrinsics, a held intrinsics component being one (its column is zeros, S gets the
// unit diagonal from k_cov_subset_diag, S^-1 its zeros from k_cov_subset_sinv).
// An eliminated time: S -= W_x V_t^-1 W_y' over the camera, marker AND intrinsics blocks of its rows.  The three x blocks are taken one
// at a time — Y_x = W_x V_t^-1 of the lane's row is 36 doubles, all three would not fit beside V_t^-1 — and the rows' W are staged
// again for each (the rows are cheap to form again; nothing is kept between the passes).
__global__ void __launch_bounds__(64)
k_cov_mc_intr_lin(int T, const int* __restrict__ tptr, const CovMcRow* __restrict__ rows, const double* __restrict__ obs8, const double* __restrict__ six,
                  const double* __restrict__ dist, const int* __restrict__ sub24, const double* __restrict__ pc, const int* __restrict__ pos, int nb,
                  const unsigned char* __restrict__ elim, double half_side, double rcond, int n, double* __restrict__ S, int* __restrict__ flags,
                  double loss, const double* __restrict__ wts) {
  __shared__ double Wl[64 * RSBA_COV_MCI_LDS];
  __shared__ double Vil[36];   // V_t^-1 of the time at hand: read where Y is formed, not held in registers across the staging
  __shared__ int Pl[64][3];
  const int lane = threadIdx.x;
  // one row's four corners: J (2 x 24 each, row stride 24) through f(J)
  auto corners = [&](int q, auto&& f) {
    const CovMcRow rw = rows[q];
    const double* o8 = obs8 + 8 * (size_t)q;
    const double* pcc = rw.cam_block >= 0 ? pc + (size_t)rw.cam_block * CC_STRIDE : nullptr;
    const double* pct = pc + (size_t)rw.time_block * CC_STRIDE;
    const double* pcm = rw.marker_block >= 0 ? pc + (size_t)rw.marker_block * CC_STRIDE : nullptr;
    const double* sv = six + 6 * (size_t)rw.camera;
    const double intr4[4] = {sv[0], sv[1], sv[2], sv[3]};
    const double kd5[5] = {sv[4], sv[5], dist[5 * (size_t)rw.camera + 2], dist[5 * (size_t)rw.camera + 3], dist[5 * (size_t)rw.camera + 4]};
    double sq = 1.0;
    if (loss != 0.0 || wts != nullptr) {
      double ss = 0.0;
#pragma unroll 1
      for (int k = 0; k < 4; ++k) {
        const double cx = (k == 0 || k == 3) ? -half_side : half_side, cy = k < 2 ? half_side : -half_side;
        double r[2], J[36];
        MarkerCornerResidualJacobian<true>(pcc, pct, pcm, intr4, cx, cy, o8[2 * k], o8[2 * k + 1], r, J, kd5);
        ss += r[0] * r[0] + r[1] * r[1];
      }
      (void)LossAndScale(loss, ss, &sq);
      if (wts != nullptr) sq *= sqrt(wts[q]);
    }
    const int sub = sub24[q];
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      const double cx = (k == 0 || k == 3) ? -half_side : half_side, cy = k < 2 ? half_side : -half_side;
      double r[2], Jp[36], it[5], J[48];
      MarkerCornerResidualJacobian<true>(pcc, pct, pcm, intr4, cx, cy, o8[2 * k], o8[2 * k + 1], r, Jp, kd5);
      MarkerCornerIntrinsicsTerms(pcc, pct, pcm, intr4, kd5, cx, cy, it);
#pragma unroll
      for (int e = 0; e < 18; ++e) { J[e] = Jp[e]; J[24 + e] = Jp[18 + e]; }
      J[18] = it[0]; J[19] = 0.0; J[20] = 1.0; J[21] = 0.0; J[22] = it[2]; J[23] = it[2] * it[4];
      J[42] = 0.0; J[43] = it[1]; J[44] = 0.0; J[45] = 1.0; J[46] = it[3]; J[47] = it[3] * it[4];
#pragma unroll
      for (int e = 0; e < 48; ++e) J[e] = ((sub >> (e % 24)) & 1) ? 0.0 : J[e] * sq;
      f(J);
    }
  };
  // stage W_cam, W_marker, W_intr (= sum over corners of J_x' J_t) of row q into this lane's LDS row, with the blocks' positions
  auto stage = [&](int q, bool act) {
    double* w = Wl + lane * RSBA_COV_MCI_LDS;
    for (int e = 0; e < 108; ++e) w[e] = 0.0;
    Pl[lane][0] = -1; Pl[lane][1] = -1; Pl[lane][2] = -1;
    if (!act) return;
    const CovMcRow rw = rows[q];
    Pl[lane][0] = rw.cam_block >= 0 ? pos[rw.cam_block] : -1;
    Pl[lane][1] = rw.marker_block >= 0 ? pos[rw.marker_block] : -1;
    Pl[lane][2] = pos[nb + rw.camera];
    corners(q, [&](const double* J) {
      for (int x = 0; x < 3; ++x) {
        const int xo = x == 0 ? 0 : (x == 1 ? 12 : 18);
        for (int a = 0; a < 6; ++a)
          for (int l = 0; l < 6; ++l) w[36 * x + 6 * a + l] += J[xo + a] * J[6 + l] + J[24 + xo + a] * J[24 + 6 + l];
      }
    });
  };
  for (int t = blockIdx.x; t < T; t += gridDim.x) {
    const int b = tptr[t], k = tptr[t + 1] - b;
    if (k == 0) continue;
    const bool el = elim[t] != 0;
    double V[21];
#pragma unroll
    for (int e = 0; e < 21; ++e) V[e] = 0.0;
    // J'J of every row among its blocks that have columns (upper blocks), V_t for an eliminated time
    __syncthreads();   // (the last time's staged rows have been read)
    for (int q = lane; q < k; q += 64) {
      const CovMcRow rw = rows[b + q];
      const int blk[4] = {rw.cam_block, rw.time_block, rw.marker_block, nb + rw.camera};
      int ps[4];
      for (int x = 0; x < 4; ++x) ps[x] = blk[x] >= 0 ? pos[blk[x]] : -1;
      // (the corner's rows go through the lane's own LDS row, free until the staging below: the sixteen block pairs are walked by
      //  rolled loops that index the rows, which registers cannot be)
      double* jl = Wl + lane * RSBA_COV_MCI_LDS;
      corners(b + q, [&](const double* J) {
#pragma unroll
        for (int e = 0; e < 48; ++e) jl[e] = J[e];
#pragma unroll 1
        for (int xy = 0; xy < 16; ++xy) {
          const int x = xy >> 2, y = xy & 3;
          if (ps[x] < 0 || ps[y] < 0 || ps[x] > ps[y] || (ps[x] == ps[y] && x != y)) continue;
          double* Sb = S + (size_t)ps[x] * n + ps[y];
#pragma unroll 1
          for (int a = 0; a < 6; ++a) {
            const double ju = jl[6 * x + a], jv = jl[24 + 6 * x + a];
            for (int c = (x == y ? a : 0); c < 6; ++c) unsafeAtomicAdd(&Sb[(size_t)a * n + c], ju * jl[6 * y + c] + jv * jl[24 + 6 * y + c]);
          }
        }
        if (el) {
          int e = 0;
#pragma unroll
          for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) { V[e] += J[6 + a] * J[6 + c] + J[30 + a] * J[30 + c]; ++e; }
        }
      });
    }
    if (!el) continue;
#pragma unroll
    for (int e = 0; e < 21; ++e) V[e] = WaveSum(V[e]);
    SubsetUnitDiagonal((sub24[b] >> 6) & 63, V);
    {
      double Vi[36];
      const bool ok = CovSym6Inverse(V, rcond, Vi);
      if (!ok) {
        if (lane == 0) atomicOr(&flags[COV_FLAG_POINT], 1);
        continue;
      }
      if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 36; ++e) Vil[e] = Vi[e];
      }
    }
#pragma unroll 1
    for (int x = 0; x < 3; ++x) {
      for (int qa0 = 0; qa0 < k; qa0 += 64) {
        __syncthreads();
        stage(b + qa0 + lane, qa0 + lane < k);
        __syncthreads();
        // Y_x = W_x V_t^-1 of this lane's row
        double Y[36];
        const double* w = Wl + lane * RSBA_COV_MCI_LDS + 36 * x;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int l = 0; l < 6; ++l) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) v += w[6 * a + m] * Vil[6 * m + l];
            Y[6 * a + l] = v;
          }
        const int px = Pl[lane][x];
        for (int qb0 = 0; qb0 < k; qb0 += 64) {
          __syncthreads();
          stage(b + qb0 + lane, qb0 + lane < k);
          __syncthreads();
          const int nbq = min(64, k - qb0);
          for (int bb = 0; bb < nbq; ++bb) {
            const double* wb = Wl + bb * RSBA_COV_MCI_LDS;
#pragma unroll 1
            for (int y = 0; y < 3; ++y) {
              const int py = Pl[bb][y];
              if (px < 0 || py < 0 || px > py) continue;
              double* Sb = S + (size_t)px * n + py;
#pragma unroll
              for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                  if (px == py && c < a) continue;
                  double v = 0.0;
#pragma unroll
                  for (int l = 0; l < 6; ++l) v += Y[6 * a + l] * wb[36 * y + 6 * c + l];
                  unsafeAtomicAdd(&Sb[(size_t)a * n + c], -v);
                }
            }
          }
        }
      }
    }
  }
}

// ---- any pair of blocks (rsba_solver_covariance_blocks, rsba_solver_time_covariances) ----------------------------------------
// With e the eliminated blocks (time blocks on the time-eliminating marker-chain path, points on the point model), V_e the
// undamped corrected diagonal block, W_e the blocks J_x'J_e, Y_e = W_e V_e^-1 and Sigma = S^-1 (cov_sinv):
//   cov(e, e)  = V_e^-1 + sum_{a,b} Y_a' Sigma_ab Y_b        cov(e, e') = sum_{a in e, b in e'} Y_a' Sigma_ab Y'_b
//   cov(x, e)  = -sum_a Sigma_xa Y_a
// Every kernel takes a list of requests, one wavefront per request, and re-linearises from the snapshot that the compute left in
// its arena (never from the live parameters).  Sums run in a fixed order (lanes' rows in chunks of 64 in order, WaveSum): no
// floating-point atomics, two calls give the same bits.  One orientation of a pair is computed; the host transposes.
//   k_cov_gather    blocks that exist already: a 6 x 6 block of S^-1 (camera / marker pairs, and time blocks on the dense path),
//                   or a point's 3 x 3 marginal out of cov_pts
//   k_cov_mc_cross  (t, t') and (t, x) on the time-eliminating path.  The rows of one time are first summed into ONE W per distinct
//                   camera / marker block the time touches (at most RSBA_COV_MC_MAXBLK, in LDS; slots from the host's table), so
//                   the contraction with S^-1 runs over blocks, not rows: Y_d = W_d V_t^-1 in place.  (t, x) is then a sum over
//                   the blocks; (t, t') walks the rows of t with G = sum_d Sigma_{p, p_d} Y'_d per row block, M += W' G, and
//                   cov = V_t^-1 M (+ V_t^-1 for t = t')
//   k_cov_pt_cross  (camera, point j) and (point j, point k), on the pattern of k_cov_points
// (CovReq and its kinds: ba_covariance_plan.hpp, where the host plans the lists)

// a, b: row and column of the block in S^-1 (COV_REQ_SINV); a: the point, the problem's order (COV_REQ_POINT)
__global__ void __launch_bounds__(64)
k_cov_gather(int nreq, const CovReq* __restrict__ req, int n, const double* __restrict__ Sinv, const double* __restrict__ cov_pts, double* __restrict__ out) {
  const int lane = threadIdx.x;
  for (int i = blockIdx.x; i < nreq; i += gridDim.x) {
    const CovReq rq = req[i];
    if (lane >= 36) continue;
    double v = 0.0;
    if (rq.kind == COV_REQ_SINV) v = Sinv[(size_t)(rq.a + lane / 6) * n + rq.b + lane % 6];
    else if (lane < 9) v = cov_pts[9 * (size_t)rq.a + lane];
    out[36 * (size_t)rq.out + lane] = v;
  }
}

#define RSBA_COV_MC_STAGE 37     // doubles per staged row (+1: bank padding)

// The marker chain's snapshot (the compute's arena) and the host's slot tables: the distinct blocks of time t are
// dpos[dptr[t] .. dptr[t + 1]) (their positions in S^-1), rslot[2 q + x] is the slot of row q's camera (x = 0) / marker (x = 1)
// block among them, -1: no columns.
struct CovMcSnap {
  const int* tptr; const CovMcRow* rows; const double* obs8; const double* intr; const double* pc; const double* wts;
  const int* dptr; const int* dpos; const int* rslot;
  double half_side, rcond, loss;
  int lossy, n;
};
// k_cov_mc_cross<true>'s argument: the same and the cameras' distortion coefficients [C][5], indexed as intr
struct CovMcSnapDist : CovMcSnap { const double* dist; };
// the kSub instances': the same and the rows' constant columns (sub18, see IntrDistSub; dist unused without kDist)
struct CovMcSnapSub : CovMcSnapDist { const int* sub18; };
template <bool kDist, bool kSub = false> struct CovMcSnapT { typedef CovMcSnap type; };
template <> struct CovMcSnapT<true, false> { typedef CovMcSnapDist type; };
template <bool kDist> struct CovMcSnapT<kDist, true> { typedef CovMcSnapSub type; };
__device__ __forceinline__ const double* DistOf(const CovMcSnap&, int) { return nullptr; }
__device__ __forceinline__ const double* DistOf(const CovMcSnapDist& a, int camera) { return a.dist + 5 * camera; }

template <int kX> struct CovSide { static constexpr int value = kX; };

// COV_REQ_TIME_TIME: a = t, b = t' (a <= b; out = cov(t, t'), mirrored from its upper triangle for t = t');
// COV_REQ_TIME_X: a = t, b = x's position in S^-1 (out = cov(t, x)).
// kSub: constant components (see IntrDistSub above) — the rows' constant columns are zeros, V_t has a unit diagonal there as in
// k_cov_mc_lin<., ., true>, S^-1 arrives with their rows and columns zeroed (k_cov_subset_sinv), and the rows / columns of a time's
// constant components leave as exact zeros.
template <bool kDist = false, bool kSub = false>
__global__ void __launch_bounds__(64)
k_cov_mc_cross(int nreq, const CovReq* __restrict__ req, typename CovMcSnapT<kDist, kSub>::type sn, const double* __restrict__ Sinv, double* __restrict__ out) {
  __shared__ double Yd[RSBA_COV_MC_MAXBLK * 36];
  __shared__ double stage[32 * RSBA_COV_MC_STAGE];
  __shared__ int sl[64];
  const int lane = threadIdx.x, n = sn.n;
  const double cx[4] = {-sn.half_side, sn.half_side, sn.half_side, -sn.half_side};
  const double cy[4] = {sn.half_side, sn.half_side, -sn.half_side, -sn.half_side};
  // one row's four corners: J (2 x 18 each) through f(J), with k_cov_mc_lin<true>'s corrector and weights when sn.lossy
  auto corners = [&](int q, auto&& f) {
    const CovMcRow rw = sn.rows[q];
    const double* o8 = sn.obs8 + 8 * (size_t)q;
    const double* pcc = rw.cam_block >= 0 ? sn.pc + (size_t)rw.cam_block * CC_STRIDE : nullptr;
    const double* pcm = rw.marker_block >= 0 ? sn.pc + (size_t)rw.marker_block * CC_STRIDE : nullptr;
    double sq = 1.0;
    if (sn.lossy) {
      double ss = 0.0;
      for (int k = 0; k < 4; ++k) {
        double r[2], J[36];
        MarkerCornerResidualJacobian<kDist>(pcc, sn.pc + (size_t)rw.time_block * CC_STRIDE, pcm, sn.intr + 4 * rw.camera, cx[k], cy[k], o8[2 * k], o8[2 * k + 1], r, J, DistOf(sn, rw.camera));
        ss += r[0] * r[0] + r[1] * r[1];
      }
      (void)LossAndScale(sn.loss, ss, &sq);
      if (sn.wts != nullptr) sq *= sqrt(sn.wts[q]);
    }
    for (int k = 0; k < 4; ++k) {
      double r[2], J[36];
      MarkerCornerResidualJacobian<kDist>(pcc, sn.pc + (size_t)rw.time_block * CC_STRIDE, pcm, sn.intr + 4 * rw.camera, cx[k], cy[k], o8[2 * k], o8[2 * k + 1], r, J, DistOf(sn, rw.camera));
      if (sn.lossy) {
#pragma unroll
        for (int e = 0; e < 36; ++e) J[e] *= sq;
      }
      if constexpr (kSub) SubsetZeroColumns(sn.sub18[q], J);
      f(J);
    }
  };
  // a time's constant components (its rows carry them; a time in a request has rows)
  auto time_sub = [&](int t) { if constexpr (kSub) return (sn.sub18[sn.tptr[t]] >> 6) & 63; else return 0; };
  // V_t^-1 (every lane), V_t summed over the rows as k_cov_mc_lin sums it
  auto time_inverse = [&](int t, double Vi[36]) {
    const int b = sn.tptr[t], k = sn.tptr[t + 1] - b;
    double V[21];
#pragma unroll
    for (int e = 0; e < 21; ++e) V[e] = 0.0;
    for (int q = lane; q < k; q += 64)
      corners(b + q, [&](const double* J) {
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int c = a; c < 6; ++c) { V[e] += J[6 + a] * J[6 + c] + J[24 + a] * J[24 + c]; ++e; }
      });
#pragma unroll
    for (int e = 0; e < 21; ++e) V[e] = WaveSum(V[e]);
    if constexpr (kSub) SubsetUnitDiagonal(time_sub(t), V);
    (void)CovSym6Inverse(V, sn.rcond, Vi);   // (k_cov_mc_lin has already raised the flag for a singular block)
  };
  for (int i = blockIdx.x; i < nreq; i += gridDim.x) {
    const CovReq rq = req[i];
    double* o = out + 36 * (size_t)rq.out;
    const int tb = rq.kind == COV_REQ_TIME_TIME ? rq.b : rq.a;
    const int b = sn.tptr[tb], k = sn.tptr[tb + 1] - b, d0 = sn.dptr[tb], nd = sn.dptr[tb + 1] - d0;
    // ---- W_d = sum over the rows of tb that touch block d of J_d'J_t, rows in order
    __syncthreads();
    for (int idx = lane; idx < nd * 36; idx += 64) Yd[idx] = 0.0;
    for (int q0 = 0; q0 < k; q0 += 64) {
      const int q = q0 + lane;
      auto side = [&](auto xc) {
        constexpr int x = decltype(xc)::value, xo = x == 0 ? 0 : 12;
        const int slot = q < k ? sn.rslot[2 * (size_t)(b + q) + x] : -1;
        double w[36];
#pragma unroll
        for (int e = 0; e < 36; ++e) w[e] = 0.0;
        if (slot >= 0)
          corners(b + q, [&](const double* J) {
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
              for (int l = 0; l < 6; ++l) w[6 * a + l] += J[xo + a] * J[6 + l] + J[18 + xo + a] * J[24 + l];
          });
        __syncthreads();
        sl[lane] = slot;
        for (int h = 0; h < 2; ++h) {   // half a chunk at a time through the staging rows
          if ((lane >> 5) == h) {
            double* st = stage + (lane & 31) * RSBA_COV_MC_STAGE;
#pragma unroll
            for (int e = 0; e < 36; ++e) st[e] = w[e];
          }
          __syncthreads();
          const int nr = min(32, k - q0 - 32 * h);
          for (int idx = lane; idx < nd * 36; idx += 64) {
            const int d = idx / 36, e = idx - 36 * d;
            double v = Yd[idx];
            for (int bb = 0; bb < nr; ++bb)
              if (sl[32 * h + bb] == d) v += stage[bb * RSBA_COV_MC_STAGE + e];
            Yd[idx] = v;
          }
          __syncthreads();
        }
      };
      side(CovSide<0>{});
      side(CovSide<1>{});
    }
    // ---- Y_d = W_d V_tb^-1 in place (a lane per row of six)
    {
      double Vi[36];
      time_inverse(tb, Vi);
      for (int r = lane; r < nd * 6; r += 64) {
        double w6[6], y6[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) w6[m] = Yd[6 * r + m];
#pragma unroll
        for (int l = 0; l < 6; ++l) {
          double v = 0.0;
#pragma unroll
          for (int m = 0; m < 6; ++m) v += w6[m] * Vi[6 * m + l];
          y6[l] = v;
        }
#pragma unroll
        for (int l = 0; l < 6; ++l) Yd[6 * r + l] = y6[l];
      }
    }
    __syncthreads();
    double acc[36];
#pragma unroll
    for (int e = 0; e < 36; ++e) acc[e] = 0.0;
    if (rq.kind == COV_REQ_TIME_X) {
      // cov(t, x) = -sum_d Y_d' Sigma_{p_d, x}
      for (int d = lane; d < nd; d += 64) {
        const double* Sb = Sinv + (size_t)sn.dpos[d0 + d] * n + rq.b;
        const double* y = Yd + 36 * d;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double s6[6];
#pragma unroll
          for (int c = 0; c < 6; ++c) s6[c] = Sb[(size_t)r * n + c];
#pragma unroll
          for (int a = 0; a < 6; ++a) {
            const double ya = y[6 * r + a];
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[6 * a + c] -= ya * s6[c];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 36; ++e) acc[e] = WaveSum(acc[e]);
      if (lane == 0) {
        const int sa = time_sub(tb);
#pragma unroll
        for (int e = 0; e < 36; ++e) o[e] = kSub && ((sa >> (e / 6)) & 1) ? 0.0 : acc[e];
      }
      continue;
    }
    // ---- (t, t'): M = sum over the rows of t and their blocks of W' G, G = sum_d Sigma_{p, p_d} Y'_d
    const int ta = rq.a, ba = sn.tptr[ta], ka = sn.tptr[ta + 1] - ba, da = sn.dptr[ta];
    for (int q = lane; q < ka; q += 64) {
      auto side = [&](auto xc) {
        constexpr int x = decltype(xc)::value, xo = x == 0 ? 0 : 12;
        const int slot = sn.rslot[2 * (size_t)(ba + q) + x];
        if (slot < 0) return;
        const int p = sn.dpos[da + slot];
        double G[36];
#pragma unroll
        for (int e = 0; e < 36; ++e) G[e] = 0.0;
        for (int d = 0; d < nd; ++d) {
          const double* Sb = Sinv + (size_t)p * n + sn.dpos[d0 + d];
          const double* y = Yd + 36 * d;
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            double s6[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) s6[c] = Sb[(size_t)r * n + c];
#pragma unroll
            for (int l = 0; l < 6; ++l) {
              double v = 0.0;
#pragma unroll
              for (int c = 0; c < 6; ++c) v += s6[c] * y[6 * c + l];
              G[6 * r + l] += v;
            }
          }
        }
        corners(ba + q, [&](const double* J) {
#pragma unroll
          for (int rho = 0; rho < 2; ++rho) {
            double h6[6];
#pragma unroll
            for (int l = 0; l < 6; ++l) {
              double v = 0.0;
#pragma unroll
              for (int a = 0; a < 6; ++a) v += J[18 * rho + xo + a] * G[6 * a + l];
              h6[l] = v;
            }
#pragma unroll
            for (int m = 0; m < 6; ++m)
#pragma unroll
              for (int l = 0; l < 6; ++l) acc[6 * m + l] += J[18 * rho + 6 + m] * h6[l];
          }
        });
      };
      side(CovSide<0>{});
      side(CovSide<1>{});
    }
#pragma unroll
    for (int e = 0; e < 36; ++e) acc[e] = WaveSum(acc[e]);
    double Via[36];
    time_inverse(ta, Via);
    if (lane == 0) {
      double R[36];
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int l = 0; l < 6; ++l) {
          double v = ta == tb ? Via[6 * a + l] : 0.0;
#pragma unroll
          for (int m = 0; m < 6; ++m) v += Via[6 * a + m] * acc[6 * m + l];
          R[6 * a + l] = v;
        }
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int l = 0; l < 6; ++l) o[6 * a + l] = ta == tb && l < a ? R[6 * l + a] : R[6 * a + l];
      if constexpr (kSub) {
        const int sa = time_sub(ta), sb = time_sub(tb);
#pragma unroll
        for (int e = 0; e < 36; ++e) if (((sa >> (e / 6)) | (sb >> (e % 6))) & 1) o[e] = 0.0;
      }
    }
  }
}

// The point model's snapshot: camc, the column map and the COPY of the points that the compute took (the solver's point order).
struct CovPtSnap {
  const double* obs_u; const double* obs_v; const int* obs_cam; const int* pt_ptr;
  const double* camc; const double* pts; const int* cam_pos;
  double loss, rcond;
  int n;
};

// COV_REQ_CAM_POINT: a = the camera's position in S^-1, b = point j (the solver's order): out = cov(camera, j), 6 x 3 row-major.
// COV_REQ_POINT_POINT: a = point j, b = point k, j != k: out = cov(j, k), 3 x 3.  Lane a takes view a of each chunk of j; the
// Y of k's views are broadcast with __shfl.
__global__ void __launch_bounds__(256)
k_cov_pt_cross(int nreq, const CovReq* __restrict__ req, CovPtSnap sn, const double* __restrict__ Sinv, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6, n = sn.n;
  for (int i = blockIdx.x * nwave + wave; i < nreq; i += gridDim.x * nwave) {
    const CovReq rq = req[i];
    double* o = out + 36 * (size_t)rq.out;
    const int pk = rq.b, bk = sn.pt_ptr[pk], kk = sn.pt_ptr[pk + 1] - bk;
    const double Xk[3] = {sn.pts[3 * (size_t)pk], sn.pts[3 * (size_t)pk + 1], sn.pts[3 * (size_t)pk + 2]};
    double V[6], Vik[6];
    CovPointBlock(sn.camc, sn.obs_u, sn.obs_v, sn.obs_cam, bk, kk, Xk, sn.loss, lane, V);
    (void)CovPointInverse(V, sn.rcond, Vik);
    if (rq.kind == COV_REQ_CAM_POINT) {
      // -sum over the views of Sigma_{camera, c_q} Y_q
      double acc[18];
#pragma unroll
      for (int e = 0; e < 18; ++e) acc[e] = 0.0;
      for (int q = lane; q < kk; q += 64) {
        const int cam = sn.obs_cam[bk + q], pq = sn.cam_pos[cam];
        if (pq < 0) continue;
        double jc[12], jp[6], W[18], Y[18];
        CovObsJacobian(sn.camc, cam, Xk, sn.obs_u[bk + q], sn.obs_v[bk + q], sn.loss, jc, jp);
        CovWY(jc, jp, Vik, W, Y);
        const double* Sb = Sinv + (size_t)rq.a * n + pq;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double s6[6];
#pragma unroll
          for (int c = 0; c < 6; ++c) s6[c] = Sb[(size_t)r * n + c];
#pragma unroll
          for (int c3 = 0; c3 < 3; ++c3) {
            double v = 0.0;
#pragma unroll
            for (int c = 0; c < 6; ++c) v += s6[c] * Y[3 * c + c3];
            acc[3 * r + c3] -= v;
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 18; ++e) acc[e] = WaveSum(acc[e]);
      if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 18; ++e) o[e] = acc[e];
      }
      continue;
    }
    const int pj = rq.a, bj = sn.pt_ptr[pj], kj = sn.pt_ptr[pj + 1] - bj;
    const double Xj[3] = {sn.pts[3 * (size_t)pj], sn.pts[3 * (size_t)pj + 1], sn.pts[3 * (size_t)pj + 2]};
    double Vij[6];
    CovPointBlock(sn.camc, sn.obs_u, sn.obs_v, sn.obs_cam, bj, kj, Xj, sn.loss, lane, V);
    (void)CovPointInverse(V, sn.rcond, Vij);
    double acc[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) acc[e] = 0.0;
    for (int qa0 = 0; qa0 < kj; qa0 += 64) {
      const int qa = qa0 + lane;
      int pa = -1;
      double Ya[18];
#pragma unroll
      for (int e = 0; e < 18; ++e) Ya[e] = 0.0;
      if (qa < kj) {
        const int cam = sn.obs_cam[bj + qa];
        pa = sn.cam_pos[cam];
        double jc[12], jp[6], W[18];
        CovObsJacobian(sn.camc, cam, Xj, sn.obs_u[bj + qa], sn.obs_v[bj + qa], sn.loss, jc, jp);
        CovWY(jc, jp, Vij, W, Ya);
      }
      for (int qb0 = 0; qb0 < kk; qb0 += 64) {
        const int qb = qb0 + lane;
        int pb = -1;
        double Yb[18];
#pragma unroll
        for (int e = 0; e < 18; ++e) Yb[e] = 0.0;
        if (qb < kk) {
          const int cam = sn.obs_cam[bk + qb];
          pb = sn.cam_pos[cam];
          double jc[12], jp[6], W[18];
          CovObsJacobian(sn.camc, cam, Xk, sn.obs_u[bk + qb], sn.obs_v[bk + qb], sn.loss, jc, jp);
          CovWY(jc, jp, Vik, W, Yb);
        }
        const int nb = min(64, kk - qb0);
        for (int bb = 0; bb < nb; ++bb) {
          const int pbb = __shfl(pb, bb, 64);
          double y[18];
#pragma unroll
          for (int e = 0; e < 18; ++e) y[e] = __shfl(Yb[e], bb, 64);
          if (pa < 0 || pbb < 0) continue;
          const double* Sb = Sinv + (size_t)pa * n + pbb;
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            double s6[6], z[3];
#pragma unroll
            for (int c = 0; c < 6; ++c) s6[c] = Sb[(size_t)r * n + c];
#pragma unroll
            for (int c3 = 0; c3 < 3; ++c3) {
              double v = 0.0;
#pragma unroll
              for (int c = 0; c < 6; ++c) v += s6[c] * y[3 * c + c3];
              z[c3] = v;
            }
#pragma unroll
            for (int a3 = 0; a3 < 3; ++a3)
#pragma unroll
              for (int c3 = 0; c3 < 3; ++c3) acc[3 * a3 + c3] += Ya[3 * r + a3] * z[c3];
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) acc[e] = WaveSum(acc[e]);
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < 9; ++e) o[e] = acc[e];
    }
  }
}

}  // namespace rsba
