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
// One row of the marker-chain problem in time order: pose-block indices into [C | T | M] (-1: not a parameter of this row) and
// the camera whose intrinsics project it.
struct CovMcRow { int cam_block, time_block, marker_block, camera; };

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

// Normal matrix of the marker-chain problem into S (n x n, zeroed by the caller, upper blocks): one wavefront per time block,
// one lane per row (chunks of 64).  pos[block] = 6 x compact index or -1 (constant / unreferenced / eliminated).  elim[t] != 0:
// time block t is eliminated — S -= W_x V_t^-1 W_y' over the pairs of its rows' camera / marker blocks, W_x = sum J_x'J_t.
// kLoss: J of a row scaled by sqrt(rho'(s)) (loss: LossAndScale's signed parameter), s taken over its four corners first; wts
// (nullptr: none): the rows' weights a_q (ceres::ScaledLoss) in the rows' order, the factor sqrt(a_q) sqrt(rho').
template <bool kLoss>
__global__ void __launch_bounds__(64)
k_cov_mc_lin(int T, const int* __restrict__ tptr, const CovMcRow* __restrict__ rows, const double* __restrict__ obs8, const double* __restrict__ intr,
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
        MarkerCornerResidualJacobian(pcc, pc + (size_t)rw.time_block * CC_STRIDE, pcm, intr + 4 * rw.camera, cx[k], cy[k], o8[2 * k], o8[2 * k + 1], r, J);
        ss += r[0] * r[0] + r[1] * r[1];
      }
      (void)LossAndScale(loss, ss, &sq);
      if (wts != nullptr) sq *= sqrt(wts[q]);
    }
    for (int k = 0; k < 4; ++k) {
      double r[2], J[36];
      MarkerCornerResidualJacobian(pcc, pc + (size_t)rw.time_block * CC_STRIDE, pcm, intr + 4 * rw.camera, cx[k], cy[k], o8[2 * k], o8[2 * k + 1], r, J);
      if constexpr (kLoss) {
        for (int e = 0; e < 36; ++e) J[e] *= sq;
      }
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

}  // namespace rsba
