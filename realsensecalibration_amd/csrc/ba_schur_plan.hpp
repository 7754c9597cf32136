// Host-side planning of the point model's set-up: the observation layout (per-point CSR, balanced point order, sliced-ELL
// copy) and the static structure of the tiled Schur kernel (visibility masks, tiles, segments, reduction groups, reducers,
// stage arrivals, launch orders, sparse hit lists).  Plain C++: nothing here touches the GPU or reads the environment behind
// the caller's back, so the whole unit runs under the host sanitizers (tests/host_sanitize_driver.cpp).  ba_solver.hip
// allocates and copies what is planned here; the kernels of ba_schur_tiled.hpp read it.
//
// The constants and the work-list entry below are shared with the kernels and defined here only.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rsba {

#define RSBA_TG 16          // cameras per group
#define RSBA_MAX_STAGES 32        // camera groups a pipelined solve can gate on (512 cameras)
#ifndef RSBA_CHUNK
#define RSBA_CHUNK 512      // points per LDS chunk (-DRSBA_CHUNK=256 builds and runs: measured only together with three workgroups per CU, HISTORY.md round 5)
#endif
#define RSBA_CW (RSBA_CHUNK / 64)
#define RSBA_GRP 8          // segments per reduction group (more than 64 cameras)
#define RSBA_GRP_SMALL 4    // ... up to 64 cameras
#define RSBA_SELF_SETS 6      // reducers of a self tile: the sets of its 42 components that the K factors do not couple (ReducerSelfSet)
#define RSBA_DIRECT_GROUPS 4  // tiles with at most this many groups are finished by their last group, without reducers
#define RSBA_HIT_NONE 0xffffffffu   // an empty entry of a sparse hit list (PairSegmentSparse)
#define RSBA_CHOL_MAXN 384  // largest reduced system the one-launch factorisations take (64 cameras)
#define RSBA_PB 32          // panel width of the factorisations
#define RSBA_PLD (RSBA_PB + 1)   // ... and a panel's LDS leading dimension (bank-conflict padding)
#define RSBA_CT 64          // trailing-update tile of the multi-launch factorisation (ba_cholesky_large.hpp)
#define RSBA_BSM_BPG 3      // k_backsub_multi: blocks per workgroup (96 columns)
constexpr int kTileHandDoubles = 7168;   // doubles of one hand-over buffer of the tiled factorisation's diagonal chain (ba_cholesky_tiles.hpp)
// the reduced system's dimension padded to whole panels (constexpr: host and device)
constexpr int MultiCholPadded(int nc) { return (nc + RSBA_PB - 1) / RSBA_PB * RSBA_PB; }

// LDS doubles: (n+2) x 33 shared by the panel and the B strip, 32 x 33 tiles for T and the padded L11, 32 inverse
// pivots, scratch, the column scale, four 32 x 33 tiles for the look-ahead products of the next diagonal block.
inline size_t CholeskyLdsDoubles(int n) {
  const size_t fact = (size_t)(n + 2) * RSBA_PLD + 2 * RSBA_PB * RSBA_PLD + RSBA_PB + 64 + (size_t)n + 4 * RSBA_PB * RSBA_PLD;
  const size_t back = (size_t)((n + 63) & ~63) + 3 * RSBA_PB * RSBA_PLD + 64;
  return fact > back ? fact : back;
}

// Which tile the workgroup with index t works on.  With more tiles than CUs, the workgroups t and t + (number of CUs) end up
// on the same CU (measured: RSBA_MC_TRACE=1 lists the pairs), and a diagonal tile that shares its CU with a tile busy
// updating takes ~6 us longer per tile column: row by row, the first eleven diagonal tiles of 256 cameras were paired with
// tiles of the last three tile rows, busy from the first panel to the last.  So: the first `extra` indices go to tiles that
// retire early and are off the chain (I >= J + 2 of the first tile columns), their partners at the end of the launch are the
// tiles of the LAST tile columns (idle until late), everybody else — every early diagonal and sub-diagonal tile — has a CU alone.
inline std::vector<int> TileOrder(int nrt, int num_cus) {
  const int ntiles = nrt * (nrt + 1) / 2, extra = std::max(0, std::min(ntiles - num_cus, ntiles / 2));
  std::vector<int> order;
  order.reserve(ntiles);
  if (extra == 0 || nrt > 255) {
    for (int I = 0; I < nrt; ++I) for (int J = 0; J <= I; ++J) order.push_back(I << 8 | J);
    return order;
  }
  std::vector<char> taken((size_t)nrt * nrt, 0);
  std::vector<int> first, last;
  for (int J = 0; J < nrt && (int)first.size() < extra; ++J)
    for (int I = J + 2; I < nrt && (int)first.size() < extra; ++I) { first.push_back(I << 8 | J); taken[(size_t)I * nrt + J] = 1; }
  for (int J = nrt - 1; J >= 0 && (int)last.size() < (int)first.size(); --J)
    for (int I = nrt - 1; I >= J && (int)last.size() < (int)first.size(); --I)
      if (!taken[(size_t)I * nrt + J]) { last.push_back(I << 8 | J); taken[(size_t)I * nrt + J] = 1; }
  order = first;
  for (int I = 0; I < nrt; ++I) for (int J = 0; J <= I; ++J) if (!taken[(size_t)I * nrt + J]) order.push_back(I << 8 | J);
  order.insert(order.end(), last.begin(), last.end());
  return order;
}

// A segment is a range of 64-point mask words of one tile (not necessarily chunk-aligned: small problems get as many
// workgroups as they have words).
struct SchurSeg {
  int ga, gb, word_begin, word_end, self;
  // in-kernel reduction tree of the pair tiles: segment -> group of RSBA_GRP consecutive segments -> tile -> stage
  int tile, grp, grp_seg0, grp_nseg, tile_grp0, tile_ngrp, stage, stage_ntiles, nred, index, pad2;
  // index: the entry's own number (segs_ordered, the copy in launch order, is what the kernel reads: one load per ticket)
  // self: 0 pair segment, 1 self segment, 2 / 3 reducer of a pair / self tile (word_begin..word_end = its components)
};

// The six switches of the work partition (same answers, other launch geometry).  FromEnv() reads them once, when a solver
// is set up; the planning functions take them as an argument.
struct SchurPlanSwitches {
  static constexpr int kUnset = INT_MIN;
  int seg_per_cu = kUnset;      // RSBA_SEG_PER_CU: pair segments per CU over all pair tiles, exactly (no whole-chunk rounding)
  int seg_target = kUnset;      // RSBA_SEG_TARGET: the same number through the whole-chunk rounding; RSBA_SEG_PER_CU wins
  bool sparse_pairs = true;     // RSBA_SPARSE_PAIRS=0: the masked search above 64 cameras too
  int balance = 1;              // RSBA_BALANCE: 0 file order, 1 balanced, n > 1: n candidate units per point
  bool balance_parity = true;   // RSBA_BALANCE_PARITY=0: no even / odd word pass inside the units
  int red_delay = 250;          // RSBA_RED_DELAY: entries of the next stage that run ahead of a stage's reducers
  static SchurPlanSwitches FromEnv();
};

// The observations as the kernels read them.  SortObservations fills the per-point CSR (ptr, cam, u, v, order, max_views,
// duplicate); OrderAndSlice applies the balanced point order (when asked to) and lays out the sliced-ELL copy.  Two steps,
// because which schedule the partition is balanced for is known only once the device has been probed.
struct PointLayout {
  std::vector<int> ptr;          // [P + 1] observations of a point, sorted by camera (file order among equals)
  std::vector<int> cam;          // [N]
  std::vector<double> u, v;      // [N]
  std::vector<int64_t> order;    // [N] sorted position -> original observation index
  std::vector<int> pt_perm;      // device position of a point -> its index in the problem (empty: identity)
  int max_views = 0;
  bool duplicate = false;        // some camera observes the same point twice
  // sliced-ELL: slice = 64 consecutive points, as wide as its widest point; element e = (sl_ptr[slice] + view) * 64 + lane
  std::vector<int> sl_ptr;       // [ceil(P / 64) + 1]
  std::vector<int> sl_q;         // slot -> CSR position, -1 pads
  std::vector<int> sl_cam;       // slot -> camera, -1 pads
  std::vector<double> sl_uv;     // slot -> pixel
  size_t sl_elems = 0;           // slots (sl_cam and sl_uv are never empty: one / two pad elements without observations)
};

PointLayout SortObservations(int P, int64_t N, const int32_t* point_index, const int32_t* camera_index, const double* observations);
// max_threads: cap on the host threads of the point dealing (0: as many as the process may run on); the order does not depend on it
void OrderAndSlice(int C, int P, bool balance, bool staged, int cus, const SchurPlanSwitches& sw, PointLayout* layout, int max_threads = 0);

// Everything TiledSchur::Build uploads.
struct SchurPlan {
  int C = 0, P = 0;
  int ngroups = 0, nwords = 0, nchunks = 0, ntiles = 0, nstages = 0, ngrp = 0, nseg = 0, nseg_pair = 0;
  int nblocks = 0, nblocks_self = 0, nsync = 0, self_arrivals = 0, grid_pp = 0;
  std::vector<unsigned long long> mask;   // [ngroups * 16][nwords] visibility bits
  std::vector<int> prefix;                // [ngroups * 16][nwords] set bits of mask before each word
  std::vector<int> cptr;                  // [ngroups * 16 + 1] start of each camera's observations, camera-major
  std::vector<int> cmpos;                 // [N] CSR position -> camera-major position
  std::vector<double> u_cm, v_cm;         // [N] pixels in camera-major order
  std::vector<SchurSeg> sg;               // [nblocks] compute segments (pair tiles, then self tiles), then reducers
  std::vector<int> border, border_first, border_self;   // launch orders: every step, a run's first step (empty: none), self tiles only
  std::vector<int> cm_pos;                // sliced slot -> camera-major position (0 for pads)
  bool sparse = false;                    // the pair segments walk hit lists
  std::vector<unsigned> hits, hit_off;    // [hit_entries][3] (point, camera-major positions) | [nseg_pair][4] first entry of a wavefront
  std::vector<int> hit_trips;             // [nseg_pair][4] trips of a wavefront
  size_t hit_entries = 0, hit_count = 0;  // entries (0: no lists) and the hits among them
  double hit_seconds = 0.0;               // time it took to build them
};

SchurPlan BuildSchurPlan(int C, int P, const PointLayout& layout, bool staged, bool bordered, int cus, const SchurPlanSwitches& sw);

// One line on stderr: a 64-bit FNV-1a digest of every array above, and the scalars (RSBA_DEBUG; compares two builds' plans)
void PrintPlanDigests(const PointLayout& layout, const SchurPlan& plan);

}  // namespace rsba
