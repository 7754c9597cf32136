// Host-side planning of the marker chain's time elimination (ba_marker_schur.hpp, ba_marker_split.hpp): the index tables the kernels
// walk, the path a step takes and the byte counts of its launches.  Plain C++, header-only: nothing here touches the GPU, and the
// environment is read in one place (MarkerSwitches::FromEnv, at every Upload), so the whole unit runs under the host sanitizers
// (tests/marker_plan_driver.cpp).  MarkerSchurDevice allocates and copies what is planned here and launches from the plan.
//
// The constants, structs and LDS sizes below are shared with the kernels and defined here only.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "ba_common.hpp"       // RSBA_HD, CC_STRIDE
#include "ba_problem.hpp"
#include "ba_schur_plan.hpp"   // RSBA_CHOL_MAXN, RSBA_PB, RSBA_PLD, MultiCholPadded, kTileHandDoubles, CholeskyLdsDoubles, TileOrder

namespace rsba {

#define RSBA_MT_TILE 32        // residual blocks staged per tile (32 x 152 doubles of LDS)
#define RSBA_MT_MAXD 1020      // widest local system of one time: 170 camera + marker blocks
#define RSBA_MT_THREADS 1024
#define RSBA_MT_JLD 145        // LDS stride of a staged 8 x 18 Jacobian
#define RSBA_SP_STRIDE 64   // doubles of a (time, slot) record: W (time row x, slot column q at 6 x + q: 36) | g_s (6) | U_ss lower triangle (21) | pad
#define RSBA_SP_LDS 65      // its stride in LDS
#define RSBA_MRS_MAXP 5     // panels of k_marker_reduced_solve_lds (160 reduced columns)
#define RSBA_LDS_CAP ((size_t)156 * 1024)   // bytes of LDS a workgroup of these paths may ask for

// Per-observation wiring: offsets (in doubles) of the three blocks inside the FULL parameter array, or -1
// when the functor variant has no such block; and offsets inside the ACTIVE vector.
struct MarkerObs {
  int full_cam, full_time, full_marker;  // -1: block not part of this residual
  int act_cam, act_time, act_marker;
  int camera;                            // intrinsics index
  int pad;                               // constant components (ceres::SubsetParameterization): bit q of the 18 local columns camera | time | marker
};

// A workgroup's partial system: S as packed lower triangle (row i, column j <= i at i (i + 1) / 2 + j), then the vectors.
struct PartLayout {
  int nr;
  RSBA_HD size_t packed() const { return (size_t)nr * (nr + 1) / 2; }
  RSBA_HD size_t S() const { return 0; }
  RSBA_HD size_t gc() const { return packed(); }
  RSBA_HD size_t corr() const { return packed() + nr; }
  RSBA_HD size_t diagU() const { return packed() + 2 * (size_t)nr; }
  RSBA_HD size_t scal() const { return packed() + 3 * (size_t)nr; }
  RSBA_HD size_t size() const { return packed() + 3 * (size_t)nr + 8; }
};

struct TimeSlots {  // per residual block, in time order: where its camera / marker block sits
  int slot_cam, slot_marker;   // index in its time's slot list (-1: block not part of the residual; -2 - j: a constant block, the
                               // time's j-th pose-only slot, ConstSlotPose)
  int col_cam, col_marker;     // first column in the reduced system (-1)
  int camera, pad;             // camera index of the detection (its intrinsics), whether or not the camera pose is a parameter
};

// An entry of the split elimination's block lists as the kernels read it (an int4): x the residual block, y the pose of the other
// block (sb_blk) or of the time (xi_blk), z the detecting camera, w unused.
struct BlockRef { int x, y, z, w; };
static_assert(sizeof(BlockRef) == 16, "BlockRef is uploaded as int4");

// Free intrinsics on this path (with_intr): a residual block's THIRD slot — the intrinsics block of its detecting camera — in its
// time's slot list, and that block's first reduced column; -1 both: the camera has no block.  Beside TimeSlots, which stays as it is.
struct IntrSlots { int slot_intr, col_intr; };

inline size_t AccLdsBytes(int dmax, size_t s_doubles) {
  const int smax = dmax / 6;
  return (size_t)(2 * smax * RSBA_SP_LDS + 6 * dmax + 96 + s_doubles) * sizeof(double) + (size_t)2 * ((smax + 2) & ~1) * sizeof(int);
}
inline int AccMfmaTiles(int nr) { const int nt = (nr + 15) / 16; return nt * (nt + 1) / 2; }
inline size_t AccMfmaLdsBytes(int nr, int tb) {
  const int nrp = ((nr + 15) / 16) * 16;
  return (size_t)(3 * tb * 8 * nrp + 2 * tb * 48 + 2 * tb * 4 + 2 * tb * (nr / 6) * 21 + 2 * nr + (nr / 6) * 21) * sizeof(double);
}
inline size_t MarkerSolveLdsDoubles(int nr) {
  const int np = (nr + RSBA_PB - 1) / RSBA_PB, npad = RSBA_PB * np;
  size_t rows = 0;
  for (int p = 0; p < np; ++p) rows += (size_t)(npad + 1 - RSBA_PB * p);
  return rows * RSBA_PLD + 2 * RSBA_PB * RSBA_PLD + RSBA_PB + 2 * (size_t)npad;   // panels (>= 2048 doubles: the epilogue's scratch, once they are done with) | T | Lt | invd | scl | y, then x
}

// Every switch of the time-eliminating path.  "Set and atoi == 0" turns a path off; anything else leaves the rule to the structure.
struct MarkerSwitches {
  bool split = true;           // RSBA_MT_SPLIT=0: k_time_eliminate instead of the split elimination (not with a loss or subset masks)
  bool acc_mfma = true;        // RSBA_MT_ACC_MFMA=0: the VALU accumulation whatever the reduced width
  int chunks = 0;              // RSBA_MT_CHUNKS (>= 1 when set; 0: unset): chunks of times where the chunk sums live in LDS, instead of one per CU
  bool backsub_wg = true;      // RSBA_MT_BACKSUB_WG=0: k_time_backsub_terms where the split back-substitution is off
  bool split_backsub = true;   // RSBA_MT_SPLIT_BACKSUB=0: k_time_backsub_wg / _terms behind the split elimination (not with subset masks)
  bool fork = true;            // RSBA_MT_FORK=0: the product kernels one after the other on the solver's stream
  bool solve_lds = true;       // RSBA_MT_SOLVE_LDS=0: k_marker_reduced_solve up to 160 reduced columns too
  bool chol_tiles = true;      // RSBA_CHOL_TILES=0: the multi-launch factorisation above 384 reduced columns
  bool debug = false;          // RSBA_DEBUG: set-up notes on stderr

  static MarkerSwitches FromEnv() {
    MarkerSwitches w;
    auto not_zero = [](const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); };
    w.split = not_zero("RSBA_MT_SPLIT");
    w.acc_mfma = not_zero("RSBA_MT_ACC_MFMA");
    if (const char* e = getenv("RSBA_MT_CHUNKS")) w.chunks = std::max(1, atoi(e));
    w.backsub_wg = not_zero("RSBA_MT_BACKSUB_WG");
    w.split_backsub = not_zero("RSBA_MT_SPLIT_BACKSUB");
    w.fork = not_zero("RSBA_MT_FORK");
    w.solve_lds = not_zero("RSBA_MT_SOLVE_LDS");
    w.chol_tiles = not_zero("RSBA_CHOL_TILES");
    w.debug = getenv("RSBA_DEBUG") != nullptr;
    return w;
  }
};

// The host tables of a plan, as they are uploaded.  Residual blocks are in time order (`order`), times and slots in ascending order.
struct MarkerTables {
  std::vector<MarkerObs> hmo;     // [N]
  std::vector<TimeSlots> hts;     // [N]
  std::vector<double> hobs;       // [N][8]
  std::vector<int> tptr;          // [T + 1] residual blocks of each time
  std::vector<int> sptr, scol;    // [T + 1] free slots of each time | their first reduced columns, ascending inside a time
  std::vector<int> csptr, csfull; // [T + 1] pose-only slots of each time | the full offsets of their constant blocks, ascending (has_const)
  std::vector<int> tfull;         // [T] offset of the time block in the full parameter array
  std::vector<int> cf;            // [nr] reduced column -> index in the full parameter array
  std::vector<int> htc;           // [T] 1: a constant time (has_const)
  std::vector<int> htflags;       // [T] bit 0: a constant time; bits 8..13: the time's constant components (with_subset)
  std::vector<unsigned char> hrmask;   // [nr / 6] the reduced blocks' constant components (with_subset)
  std::vector<int> hcpose;        // [ncpose] full offsets of the constant camera / marker blocks some residual applies, by first use
  std::vector<int> cpf;           // [6 ncpose] k_pose_constants_reduced's layout of them: a pose's offset at every sixth entry
  std::vector<int> cptr;          // [G + 1] times of each chunk
  // the split elimination: a (time, slot)'s residual blocks, the thread order, the camera x marker items of every chunk
  std::vector<int> h_slot_time, h_sb_ptr, h_order, h_xi_ptr, h_xi_cc, h_xi_cm, h_xc_ptr, h_xorder;
  std::vector<BlockRef> h_sb_blk, h_xi_blk;
  std::vector<int> h_bt;          // [N] the time of a residual block (split_backsub)
  std::vector<int> pcols;         // per prior of the problem (ascending block) its first reduced column, -1: constant as a whole
  std::vector<int> tc_map;        // the tiled factorisation's placement of its workgroups (TileOrder; tc_tiles > 0)
  // free intrinsics (with_intr; all empty otherwise).  An intrinsics slot j = one (time, camera with a block):
  std::vector<IntrSlots> hti;     // [N] the residual blocks' third slot and column
  std::vector<int> h_is_slot;     // [nislots] its slot S (slot order: ascending time, ascending camera)
  std::vector<int> h_is_cam;      // [nislots] its camera
  std::vector<int> h_ib_ptr;      // [nislots + 1] its residual blocks ...
  std::vector<int> h_ib_blk;      // ... in block order (nib entries: every residual block of a camera with a block, once)
  // the pair items (camera pose x own intrinsics) and (marker x detecting camera's intrinsics) of every chunk lie behind the chunk's
  // camera x marker items in h_xi_cc (the column block: camera or marker) / h_xi_cm (the row block: intrinsics), with an empty list
  // in h_xi_ptr and no thread in h_xorder.  Each is the sum, in list order, of source records of 36 doubles: record j < nislots is
  // J_i' J_c of intrinsics slot j, record nislots + e is J_i' J_m of entry e of h_ib_blk.
  std::vector<int> h_xs_item;     // [nxs] the item
  std::vector<int> h_xs_ptr;      // [nxs + 1] its sources ...
  std::vector<int> h_xs_src;      // ... ascending (= time order)
};

struct MarkerPlan {
  int N = 0, T = 0, nr = 0, nfull = 0, G = 0, dmax = 0;
  int pmax = 0;           // widest pose cache of a time: its free slots and its pose-only (constant) slots
  int ncpose = 0;         // constant camera / marker poses some residual applies
  int widest = 0;         // residual blocks of the widest time
  int np = 0;             // 1: the problem carries priors (one more partial system, one more bp_time / drho_c entry)
  double half_side = 0;
  bool with_loss = false;    // a robust loss, observation weights or priors: the kLoss instances
  bool with_subset = false;  // some block in the program has a non-zero subset mask
  bool has_const = false;    // the kConst instances: a residual names a constant camera, marker or time block, or subset masks
  bool with_dist = false;    // the kDist instances: some distortion coefficient is not zero; no path rule reads it
  bool with_intr = false;    // free intrinsics ride on this plan: a third slot per residual block, the kDist instances always
  int nr_pose = 0;           // reduced columns of the pose blocks (= nr without free intrinsics; the intrinsics blocks lie behind)
  int nislots = 0, nib = 0, nxs = 0;   // (with_intr) intrinsics slots, entries of h_ib_blk, pair items summed from source records
  int nslots_pose = 0;       // (split) slots of pose blocks = threads of k_mc_slot_products (= nslots without free intrinsics)
  // ---- the path
  bool split = true;            // the split elimination (ba_marker_split.hpp); false: k_time_eliminate
  int acc_tiles = 0;            // > 0: k_mc_accumulate_mfma with that many tiles a wavefront
  int acc_tb = 2;               // ... and times per step (three tiles a wavefront; eight: one)
  bool lds_s = false;           // the chunk sums of S live in LDS
  bool solve_lds = false;       // k_marker_reduced_solve_lds (the whole triangle in LDS: up to 160 reduced columns)
  bool split_backsub = false;   // k_mc_time_step + k_mc_candidate instead of k_time_backsub_wg / _terms
  bool backsub_wg = false;      // k_time_backsub_wg instead of k_time_backsub_terms
  bool fork = false;            // the product kernels side by side on streams of their own
  bool debug = false;
  int nb_time = 0, ncand_wg = 0;   // entries of bp_time the back-substitution writes | workgroups of k_mc_candidate
  int nslots = 0, nx = 0, ncam_cols = 0, nx_threads = 0;   // (split) slots, items of k_mc_cross, columns of the free cameras, its threads
  int tc_np = 0, tc_nrt = 0, tc_tiles = 0;   // persistent tiled factorisation: panels, tile rows, tiles (0 tiles: the multi-launch path)
  // ---- bytes of dynamic LDS (k_time_eliminate, k_mc_accumulate*, k_time_backsub_wg, the one-workgroup solves, k_marker_chol_finish)
  size_t lds_elim = 0, lds_acc = 0, lds_bw = 0, lds_solve_lds = 0, lds_solve = 0, lds_finish = 0;
  size_t tc_flags = 0, tc_hand = 0;   // the tiled factorisation's flags (ints) and hand-over buffers (doubles)
  std::vector<int> order;    // device block -> the problem's observation
  MarkerTables tab;          // (a device drops them once they are uploaded)
};

// Constant blocks (block_constant, Ceres' SetParameterBlockConstant): a constant camera or marker has no reduced column; a time's
// constant cameras and markers are its pose-only slots, behind its free slots (ConstSlotPose).  The width rule: a time's pose cache —
// its distinct camera and marker blocks, free or constant — holds at most RSBA_MT_MAXD / 6 = 170 entries; the split accumulation's
// LDS bound counts the free ones (columns) only.  A constant time is eliminated with E = 0.  No free camera or marker at all (n_r = 0):
// every time is eliminated on its own and the reduced solve is skipped.
// loss: a robust loss is set, or the problem carries observation weights or priors (then possibly with huber_delta = 0: rho(s) = s).
// Its rows are formed by the split kernels only (k_time_eliminate and k_time_backsub_wg spread a residual block's corners over lanes
// and have no block-wide s): RSBA_MT_SPLIT=0 and RSBA_MT_BACKSUB_WG are not taken then, and a problem whose times are too wide for
// the split accumulation returns RSBA_ERR_UNSUPPORTED (the solver takes the dense path).  Subset masks: the same, and the split
// back-substitution whatever the switches say (the masks are applied to the split kernels' small products).
// cus: the chip's compute units (one chunk per CU where the chunk sums live in LDS; the resident tiles fit two per CU).
// intr: the caller wants the problem's free intrinsics (rsba_problem_set_intrinsics_free) in the plan; without a mask set it changes
// nothing.  One block of six reduced columns per camera with a mask, ascending camera, behind the markers' (the dense path's order
// without the time columns; the base camera and a camera with a constant pose may have one); column c of camera k is state value
// nfull + 6 k + c.  A time's slot list gains the blocks of the cameras that detect in it — last, their columns being the highest — and
// the width rules count them.  Held components (the complement of the mask) go into hrmask like a pose block's constant components.
// Such a plan always runs the split elimination and the split back-substitution: the other forms have no place for the third block.
inline int PlanMarkerChain(const rsba_problem& p, bool loss, int cus, const MarkerSwitches& sw, MarkerPlan* out, bool intr = false) {
  MarkerPlan& P = *out;
  P = MarkerPlan();
  MarkerTables& B = P.tab;
  P.with_loss = loss; P.debug = sw.debug; P.with_dist = p.has_distortion();
  P.N = (int)p.num_observations; P.nfull = (int)p.parameters.size(); P.half_side = p.marker_side / 2;
  const int N = P.N;
  if (N <= 0) return RSBA_ERR_ARG;
  const int C = p.num_cameras, Tn = p.num_times, M = p.num_markers;
  auto is_const = [&](int block) { return block < (int)p.block_constant.size() && p.block_constant[block] != 0; };
  // reduced blocks: the free cameras and markers some residual uses, cameras first
  std::vector<int> red_col(C + M, -1);
  std::vector<char> used(C + M, 0), tused(Tn, 0);
  for (int i = 0; i < N; ++i) {
    if (p.uses_camera(i)) used[p.camera_index[i]] = 1;
    if (p.uses_marker(i)) used[C + p.marker_index[i]] = 1;
    tused[p.time_index[i]] = 1;
  }
  int K = 0;
  for (int b = 0; b < C + M; ++b) if (used[b] && !is_const(b < C ? b : Tn + b)) {
    red_col[b] = 6 * K++;
    const int full = 6 * (b < C ? b : Tn + b);   // [C | T | M] x 6
    for (int q = 0; q < 6; ++q) B.cf.push_back(full + q);
  }
  P.nr_pose = 6 * K;
  std::vector<int> icol(C, -1);   // a camera's intrinsics block
  P.with_intr = intr && p.has_free_intrinsics();
  if (P.with_intr) {
    P.with_dist = true;
    std::vector<char> named(C, 0);
    for (int i = 0; i < N; ++i) named[p.camera_index[i]] = 1;
    for (int k = 0; k < C; ++k) if (p.intrinsics_free_mask(k) != 0) {
      if (!named[k]) return RSBA_ERR_UNSUPPORTED;   // (a mask on a camera no observation names: the dense path refuses it too)
      icol[k] = 6 * K++;
      for (int q = 0; q < 6; ++q) B.cf.push_back(P.nfull + 6 * k + q);
    }
  }
  const int nr = P.nr = 6 * K;   // (0: nothing but time blocks are free)
  // constant components: of the blocks in the program only (a constant, base or unreferenced block's mask is ignored)
  for (int b = 0; b < C + M; ++b) if (red_col[b] >= 0) B.hrmask.push_back((unsigned char)p.subset_mask(b < C ? b : Tn + b));
  for (int k = 0; k < C; ++k) if (icol[k] >= 0) B.hrmask.push_back((unsigned char)(~p.intrinsics_free_mask(k) & 0x3F));
  P.with_subset = std::find_if(B.hrmask.begin(), B.hrmask.end(), [](unsigned char v) { return v != 0; }) != B.hrmask.end();
  std::vector<int> tid_of(Tn, -1);
  int T = 0;
  for (int t = 0; t < Tn; ++t) if (tused[t]) {
    tid_of[t] = T++; B.tfull.push_back(6 * (C + t)); B.htc.push_back(is_const(C + t) ? 1 : 0);
    const int mask = is_const(C + t) ? 0 : p.subset_mask(C + t);
    P.with_subset = P.with_subset || mask != 0;
    B.htflags.push_back(B.htc.back() | (mask << 8));
  }
  P.T = T;
  // residual blocks in time order (stable)
  std::vector<int>& order = P.order;
  order.resize(N);
  for (int i = 0; i < N; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return p.time_index[x] < p.time_index[y]; });
  std::vector<int>&tptr = B.tptr, &sptr = B.sptr, &scol = B.scol, &csptr = B.csptr, &csfull = B.csfull, &hcpose = B.hcpose;
  std::vector<MarkerObs>& hmo = B.hmo;
  std::vector<TimeSlots>& hts = B.hts;
  tptr.assign(T + 1, 0); sptr.assign(T + 1, 0); csptr.assign(T + 1, 0);
  hmo.resize(N); hts.resize(N);
  if (P.with_intr) B.hti.resize(N);
  B.hobs.resize(8 * (size_t)N);
  for (int k = 0; k < N; ++k) tptr[tid_of[p.time_index[order[k]]] + 1]++;
  for (int t = 0; t < T; ++t) tptr[t + 1] += tptr[t];
  int dmax = 0, pmax = 0;
  std::vector<double> work(T);
  std::vector<char> cpose_seen(C + M, 0);
  for (int t = 0; t < T; ++t) {
    std::vector<int> cols, cfl;   // the time's free slots (reduced columns) and pose-only slots (full offsets of constant blocks)
    for (int k = tptr[t]; k < tptr[t + 1]; ++k) {
      const int i = order[k];
      if (p.uses_camera(i)) {
        const int b = p.camera_index[i];
        if (red_col[b] >= 0) cols.push_back(red_col[b]);
        else { cfl.push_back(6 * p.camera_block(i)); if (!cpose_seen[b]) { cpose_seen[b] = 1; hcpose.push_back(6 * p.camera_block(i)); } }
      }
      if (p.uses_marker(i)) {
        const int b = C + p.marker_index[i];
        if (red_col[b] >= 0) cols.push_back(red_col[b]);
        else { cfl.push_back(6 * p.marker_block(i)); if (!cpose_seen[b]) { cpose_seen[b] = 1; hcpose.push_back(6 * p.marker_block(i)); } }
      }
      if (icol[p.camera_index[i]] >= 0) cols.push_back(icol[p.camera_index[i]]);
    }
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    std::sort(cfl.begin(), cfl.end());
    cfl.erase(std::unique(cfl.begin(), cfl.end()), cfl.end());
    {
      // the kernel relies on one residual block per (time, camera, marker); the same detection listed twice goes to
      // the dense path
      std::vector<std::pair<int, int>> cm;
      for (int k = tptr[t]; k < tptr[t + 1]; ++k) cm.emplace_back(p.camera_index[order[k]], p.marker_index[order[k]]);
      std::sort(cm.begin(), cm.end());
      if (std::adjacent_find(cm.begin(), cm.end()) != cm.end()) return RSBA_ERR_UNSUPPORTED;
    }
    for (int k = tptr[t]; k < tptr[t + 1]; ++k) {
      const int i = order[k];
      MarkerObs& o = hmo[k];
      o.full_cam = p.uses_camera(i) ? 6 * p.camera_block(i) : -1; o.full_time = 6 * p.time_block(i);
      o.full_marker = p.uses_marker(i) ? 6 * p.marker_block(i) : -1;
      o.act_cam = o.act_time = o.act_marker = -1; o.camera = p.camera_index[i]; o.pad = 0;
      TimeSlots& s = hts[k];
      s.col_cam = p.uses_camera(i) ? red_col[p.camera_index[i]] : -1;
      s.col_marker = p.uses_marker(i) ? red_col[C + p.marker_index[i]] : -1;
      s.camera = p.camera_index[i]; s.pad = 0;
      auto const_slot = [&](int full) { return -2 - (int)(std::lower_bound(cfl.begin(), cfl.end(), full) - cfl.begin()); };
      s.slot_cam = s.col_cam >= 0 ? (int)(std::lower_bound(cols.begin(), cols.end(), s.col_cam) - cols.begin()) : (o.full_cam >= 0 ? const_slot(o.full_cam) : -1);
      s.slot_marker = s.col_marker >= 0 ? (int)(std::lower_bound(cols.begin(), cols.end(), s.col_marker) - cols.begin())
                                        : (o.full_marker >= 0 ? const_slot(o.full_marker) : -1);
      if (P.with_intr) {
        IntrSlots& u = B.hti[k];
        u.col_intr = icol[p.camera_index[i]];
        u.slot_intr = u.col_intr >= 0 ? (int)(std::lower_bound(cols.begin(), cols.end(), u.col_intr) - cols.begin()) : -1;
      }
      memcpy(&B.hobs[8 * (size_t)k], &p.observations[8 * (size_t)i], 8 * sizeof(double));
    }
    sptr[t + 1] = sptr[t] + (int)cols.size();
    scol.insert(scol.end(), cols.begin(), cols.end());
    csptr[t + 1] = csptr[t] + (int)cfl.size();
    csfull.insert(csfull.end(), cfl.begin(), cfl.end());
    const int d = 6 * (int)cols.size();
    dmax = std::max(dmax, d);
    pmax = std::max(pmax, (int)(cols.size() + cfl.size()));
    P.widest = std::max(P.widest, tptr[t + 1] - tptr[t]);
    work[t] = (double)d * d * (1.0 + 0.25 * (tptr[t + 1] - tptr[t])) + 2000.0;
  }
  P.dmax = dmax; P.pmax = pmax;
  if (6 * pmax > RSBA_MT_MAXD) return RSBA_ERR_UNSUPPORTED;
  P.ncpose = (int)hcpose.size();
  B.cpf.assign(6 * (size_t)P.ncpose, 0);
  for (int k = 0; k < P.ncpose; ++k) B.cpf[6 * (size_t)k] = hcpose[k];
  // (constant components ride on the kConst instances of the split kernels: the time's flags arrive where tconst does)
  P.has_const = P.with_subset || P.ncpose > 0 || std::find(B.htc.begin(), B.htc.end(), 1) != B.htc.end();
  const int npc = P.has_const ? pmax : dmax / 6;   // k_time_eliminate's pose cache holds the pose-only slots too; its other tables are the free columns'
  // chunks of consecutive times, balanced by work; the partial systems together stay below 2 GB
  const PartLayout PL{nr};
  const size_t s_doubles = PL.packed() + 3 * (size_t)nr;   // the chunk sums of S and its vectors
  P.lds_elim = (size_t)(13 * dmax + 96 + RSBA_MT_TILE * (RSBA_MT_JLD + 9) + (npc + 2) * CC_STRIDE) * sizeof(double) + (size_t)(2 * RSBA_MT_TILE + 3 * (dmax / 6 + 1) + 2) * sizeof(int);
  P.lds_s = P.lds_elim + s_doubles * sizeof(double) <= RSBA_LDS_CAP;
  if (P.lds_s) P.lds_elim += s_doubles * sizeof(double);
  const bool lds_s_elim = P.lds_s;   // (k_time_eliminate's own choice, should the split kernels not take the problem)
  P.split = P.with_loss || P.with_subset || P.with_intr || sw.split;
  if (P.split) {
    const int per_wave = (AccMfmaTiles(nr) + 15) / 16;
    P.acc_tiles = (per_wave <= 8 && sw.acc_mfma) ? (per_wave <= 3 ? 3 : 8) : 0;
    if (P.acc_tiles > 0) {
      P.lds_s = true;   // (the chunk's sums never touch memory before the end: one chunk per CU, as with the sums in LDS)
      if (P.acc_tiles == 8) P.acc_tb = 1;
      P.lds_acc = AccMfmaLdsBytes(nr, P.acc_tb);
    } else {
      P.lds_s = AccLdsBytes(dmax, s_doubles) <= RSBA_LDS_CAP;
      P.lds_acc = AccLdsBytes(dmax, P.lds_s ? s_doubles : 0);
    }
    if (P.lds_acc > RSBA_LDS_CAP) {
      // times that touch more blocks than the accumulation's double-buffered records hold in LDS (~110 of the 170 the model allows):
      // k_time_eliminate, which stages 32 residual blocks at a time whatever the width
      if (P.with_loss || P.with_subset || P.with_intr) return RSBA_ERR_UNSUPPORTED;
      P.split = false; P.acc_tiles = 0; P.lds_s = lds_s_elim;
    }
  }
  // Without the LDS accumulators every entry is a read-modify-write in the partial system: few enough workgroups that
  // their partial systems stay in the L2s (8 x 4 MB) then, as many as there are times otherwise (at most 1024).
  // With the sums in LDS a workgroup fills a CU: one chunk per CU (more chunks only add partial systems to write, to
  // zero and to reduce: 1024 chunks cost 11 % of the iteration on 5000 times)
  const size_t cap_lds = sw.chunks > 0 ? (size_t)sw.chunks : (size_t)cus;
  const size_t cap = P.lds_s ? cap_lds : std::min<size_t>(1024, std::max<size_t>(64, ((size_t)24 << 20) / (PL.size() * sizeof(double))));
  int G = (int)std::min<size_t>((size_t)T, cap);
  std::vector<int>& cptr = B.cptr;
  cptr.assign(G + 1, 0);
  {
    double total = 0; for (double w : work) total += w;
    double acc = 0; int g = 0;
    for (int t = 0; t < T; ++t) {
      acc += work[t];
      // close chunk g when it has its share and enough times remain for the others
      while (g < G - 1 && acc >= total * (g + 1) / G && T - (t + 1) >= G - 1 - g) cptr[++g] = t + 1;
    }
    while (g < G) cptr[++g] = T;
    // chunks may not be empty in the middle: compact
    std::vector<int> c2; c2.push_back(0);
    for (int k = 1; k <= G; ++k) if (cptr[k] > c2.back()) c2.push_back(cptr[k]);
    G = (int)c2.size() - 1; cptr = c2;
  }
  P.G = G;
  // the split elimination's tables: a (time, slot)'s residual blocks, the thread order, the camera-marker pairs of every chunk
  auto pose_of_full = [](int full) { return full >= 0 ? full / 6 : -1; };   // full offset -> pose in the parameter array
  const int kShareFrom = 10;   // an item of k_mc_cross with this many residual blocks or more runs on two neighbouring lanes
  if (P.split) {
    std::vector<int>&h_slot_time = B.h_slot_time, &h_sb_ptr = B.h_sb_ptr, &h_order = B.h_order, &h_xi_ptr = B.h_xi_ptr, &h_xi_cc = B.h_xi_cc, &h_xi_cm = B.h_xi_cm,
        &h_xc_ptr = B.h_xc_ptr, &h_xorder = B.h_xorder;
    std::vector<BlockRef>&h_sb_blk = B.h_sb_blk, &h_xi_blk = B.h_xi_blk;
    const int nslots = P.nslots = (int)scol.size();
    int ncam_cols = 0;
    for (int b = 0; b < C; ++b) if (red_col[b] >= 0) ncam_cols += 6;   // (the free cameras: the reduced columns below the markers')
    P.ncam_cols = ncam_cols;
    h_slot_time.resize(nslots);
    h_sb_ptr.assign(nslots + 1, 0);
    for (int t = 0; t < T; ++t) {
      for (int S = sptr[t]; S < sptr[t + 1]; ++S) h_slot_time[S] = t;
      for (int k = tptr[t]; k < tptr[t + 1]; ++k) {
        if (hts[k].slot_cam >= 0) h_sb_ptr[sptr[t] + hts[k].slot_cam + 1]++;
        if (hts[k].slot_marker >= 0) h_sb_ptr[sptr[t] + hts[k].slot_marker + 1]++;
      }
    }
    for (int S = 0; S < nslots; ++S) h_sb_ptr[S + 1] += h_sb_ptr[S];
    h_sb_blk.resize(h_sb_ptr[nslots]);
    {
      std::vector<int> fill(h_sb_ptr.begin(), h_sb_ptr.end() - 1);
      for (int t = 0; t < T; ++t)
        for (int k = tptr[t]; k < tptr[t + 1]; ++k) {
          // (the other block's pose whether it is free or constant)
          if (hts[k].slot_cam >= 0) h_sb_blk[fill[sptr[t] + hts[k].slot_cam]++] = BlockRef{k, pose_of_full(hmo[k].full_marker), hts[k].camera, 0};
          if (hts[k].slot_marker >= 0) h_sb_blk[fill[sptr[t] + hts[k].slot_marker]++] = BlockRef{k, pose_of_full(hmo[k].full_cam), hts[k].camera, 0};
        }
    }
    for (int S = 0; S < nslots; ++S) if (scol[S] < P.nr_pose) h_order.push_back(S);   // (an intrinsics slot has its own kernel)
    P.nslots_pose = (int)h_order.size();
    std::stable_sort(h_order.begin(), h_order.end(), [&](int x, int y) {
      const bool cx = scol[x] < ncam_cols, cy = scol[y] < ncam_cols;
      if (cx != cy) return cx;
      return h_sb_ptr[x + 1] - h_sb_ptr[x] > h_sb_ptr[y + 1] - h_sb_ptr[y];
    });
    h_xc_ptr.assign(G + 1, 0);
    h_xi_ptr.push_back(0);
    for (int g = 0; g < G; ++g) {
      std::vector<std::pair<std::pair<int, int>, int>> items;   // ((camera column, marker column), residual block)
      for (int t = cptr[g]; t < cptr[g + 1]; ++t)
        for (int k = tptr[t]; k < tptr[t + 1]; ++k)
          if (hts[k].col_cam >= 0 && hts[k].col_marker >= 0) items.push_back({{hts[k].col_cam, hts[k].col_marker}, k});
      std::stable_sort(items.begin(), items.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
      for (size_t i = 0; i < items.size(); ++i) {
        if (i == 0 || items[i].first != items[i - 1].first) {
          if (i != 0) h_xi_ptr.push_back((int)h_xi_blk.size());
          h_xi_cc.push_back(items[i].first.first); h_xi_cm.push_back(items[i].first.second);
        }
        h_xi_blk.push_back(BlockRef{items[i].second, hmo[items[i].second].full_time / 6, hts[items[i].second].camera, 0});
      }
      if (!items.empty()) h_xi_ptr.push_back((int)h_xi_blk.size());
      if (P.with_intr) {
        // the chunk's intrinsics slots and their residual blocks, then its items with an intrinsics row: ((row, column), source)
        // A (camera, own intrinsics) block is formed per intrinsics slot, by the thread that walks exactly those residual blocks, and
        // a (marker, intrinsics) block per residual block; an item sums its records in time order.  (A thread per item walking the
        // residual blocks, as k_mc_cross has it, would give a (camera, intrinsics) item every block of the camera in the chunk.)
        std::vector<std::pair<std::pair<int, int>, int>> xs;
        for (int t = cptr[g]; t < cptr[g + 1]; ++t) {
          for (int S = sptr[t]; S < sptr[t + 1]; ++S) if (scol[S] >= P.nr_pose) {
            const int j = (int)B.h_is_slot.size();
            B.h_is_slot.push_back(S);
            B.h_is_cam.push_back((int)(std::find(icol.begin(), icol.end(), scol[S]) - icol.begin()));
            B.h_ib_ptr.push_back((int)B.h_ib_blk.size());
            bool with_cam = false;
            int cam_col = -1;
            for (int k = tptr[t]; k < tptr[t + 1]; ++k) if (B.hti[k].col_intr == scol[S]) {
              if (hts[k].col_cam >= 0) { with_cam = true; cam_col = hts[k].col_cam; }
              if (hts[k].col_marker >= 0) xs.push_back({{scol[S], hts[k].col_marker}, -1 - (int)B.h_ib_blk.size()});   // (entry e as -1 - e: nislots is not known yet)
              B.h_ib_blk.push_back(k);
            }
            if (with_cam) xs.push_back({{scol[S], cam_col}, j});
          }
        }
        std::stable_sort(xs.begin(), xs.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
        for (size_t i = 0; i < xs.size(); ++i) {
          if (i == 0 || xs[i].first != xs[i - 1].first) {
            B.h_xs_item.push_back((int)h_xi_cc.size());
            B.h_xs_ptr.push_back((int)B.h_xs_src.size());
            h_xi_cm.push_back(xs[i].first.first); h_xi_cc.push_back(xs[i].first.second);
            h_xi_ptr.push_back((int)h_xi_blk.size());   // (no residual block of its own: k_mc_cross has no thread for it)
          }
          B.h_xs_src.push_back(xs[i].second);
        }
      }
      h_xc_ptr[g + 1] = (int)h_xi_cc.size();
    }
    if (P.with_intr) {
      P.nislots = (int)B.h_is_slot.size(); P.nib = (int)B.h_ib_blk.size(); P.nxs = (int)B.h_xs_item.size();
      B.h_ib_ptr.push_back(P.nib);
      B.h_xs_ptr.push_back((int)B.h_xs_src.size());
      for (int& src : B.h_xs_src) if (src < 0) src = P.nislots + (-1 - src);
    }
    const int nx = P.nx = (int)h_xi_cc.size();
    {
      std::vector<int> ord(nx);
      for (int it = 0; it < nx; ++it) ord[it] = it;
      auto len = [&](int it) { return h_xi_ptr[it + 1] - h_xi_ptr[it]; };
      std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return len(x) > len(y); });
      for (int it : ord) if (len(it) >= kShareFrom) { h_xorder.push_back(4 * it + 2); h_xorder.push_back(4 * it + 3); }
      for (int it : ord) if (len(it) < kShareFrom && len(it) > 0) h_xorder.push_back(4 * it);   // (an empty list: an item summed from source records)
      P.nx_threads = (int)h_xorder.size();
    }
    P.fork = sw.fork;
  }
  // (k_time_backsub_wg: a corner of a residual block per lane, two per lane at most; wider times take the wavefront-per-time kernel)
  P.backsub_wg = !P.with_loss && !P.with_subset && !P.with_intr && P.widest <= 128 /* 4 x 128 corners = 512 lanes */ && sw.backsub_wg;
  P.lds_bw = (size_t)(pmax + 1) * (CC_STRIDE + 12 + 6) * sizeof(double);   // the shot's tables (k_time_backsub_wg)
  P.nb_time = P.backsub_wg ? T : (T + 3) / 4;
  P.split_backsub = P.split && (P.with_subset || P.with_intr || sw.split_backsub);
  if (P.split_backsub) {
    P.ncand_wg = (N + 255) / 256; P.nb_time = T + P.ncand_wg;
    B.h_bt.resize(N);
    for (int t = 0; t < T; ++t) for (int k = tptr[t]; k < tptr[t + 1]; ++k) B.h_bt[k] = t;
  }
  P.np = p.block_priors.empty() ? 0 : 1;   // the priors' partial system and their entry behind the times'
  for (const auto& kv : p.block_priors) B.pcols.push_back(red_col[kv.first < C ? kv.first : kv.first - Tn]);
  // the reduced solve: nothing (n_r = 0), one workgroup up to 384 columns, the tiled or the multi-launch factorisation above
  if (nr > 0 && nr <= RSBA_CHOL_MAXN) {
    P.lds_solve = std::max((size_t)4 * 1024, CholeskyLdsDoubles(nr)) * sizeof(double);
    P.lds_solve_lds = MarkerSolveLdsDoubles(nr) * sizeof(double);
    P.solve_lds = nr <= RSBA_PB * RSBA_MRS_MAXP && P.lds_solve_lds <= RSBA_LDS_CAP && sw.solve_lds;
  } else if (nr > RSBA_CHOL_MAXN) {
    P.lds_finish = std::max((size_t)4 * 1024, (size_t)((nr + 63) & ~63) + 3 * RSBA_PB * RSBA_PLD + 64) * sizeof(double);
    // one resident workgroup per 64 x 64 tile, if they all fit on the chip at once (two per CU)
    const int m = MultiCholPadded(nr), nrt = (m + 1 + 63) / 64, ntiles = nrt * (nrt + 1) / 2;
    if (sw.chol_tiles && ntiles <= 2 * cus) {
      P.tc_np = m / RSBA_PB; P.tc_nrt = nrt; P.tc_tiles = ntiles;
      P.tc_flags = (size_t)P.tc_np * (nrt + 1) + 1;
      P.tc_hand = (size_t)2 * nrt * kTileHandDoubles;   // the diagonal chain's hand-overs
      B.tc_map = TileOrder(nrt, cus);
    }
  }
  return RSBA_OK;
}

}  // namespace rsba
