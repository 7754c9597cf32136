// Host-side planning of the covariance (ba_covariance.hpp): which blocks get columns in the system and where, the marker chain's rows
// in time order with what rides on them, the cross tables of the time-eliminating path, offset -> block resolution, and the plan of a
// pair query — which kernel serves a pair, in which orientation, and how its 36 outputs are unpacked.  Plain C++, header-only, vectors
// in and vectors out (the pattern of ba_marker_plan.hpp): nothing here touches the GPU, ba_solver.hip carves, copies and launches what
// is planned here, and tests/covariance_plan_driver.cpp holds the unit to the contracts the kernels rely on under the host sanitizers.
//
// The constant flags are ARGUMENTS everywhere: the computes pass the problem's flags as they are at the call, the constant points and
// the component masks are the solver's copies from create.  This unit does not choose between them.
//
// The request struct, its kinds and the block cap below are shared with the kernels and defined here only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "ba_evaluate_plan.hpp"   // EvalMarkerRow, EvalMarkerRowOf
#include "ba_problem.hpp"

namespace rsba {

#define RSBA_COV_MC_MAXBLK 170   // distinct camera / marker blocks with columns that one time touches: 170 x 36 doubles of LDS

// One request of a pair query: a wavefront writes the block into out's 36 doubles of the staging buffer.
//   COV_REQ_SINV         a, b: row and column of a 6 x 6 block of S^-1
//   COV_REQ_POINT        a: the point (the problem's order), its 3 x 3 marginal
//   COV_REQ_TIME_TIME    a = t, b = t', a <= b: cov(t, t'), 6 x 6
//   COV_REQ_TIME_X       a = t, b = x's position in S^-1: cov(t, x), 6 x 6
//   COV_REQ_CAM_POINT    a = the camera's position in S^-1, b = the point (device position): cov(camera, point), 6 x 3
//   COV_REQ_POINT_POINT  a, b: two points (device positions), the problem's indices ascending: cov(a, b), 3 x 3
struct CovReq { int a, b, kind, out; };
enum { COV_REQ_SINV = 0, COV_REQ_POINT = 1, COV_REQ_TIME_TIME = 2, COV_REQ_TIME_X = 3, COV_REQ_CAM_POINT = 4, COV_REQ_POINT_POINT = 5 };

// One row of the marker-chain problem: pose-block indices into [C | T | M] (-1: not a parameter of this row) and the camera whose
// intrinsics project it.  Evaluate reads them in the problem's order, the covariance in time order.
typedef EvalMarkerRow CovMcRow;

// One block of a pair: what it is in the result.
struct CovBlockRef {
  enum Kind { CONSTANT, REDUCED, TIME, POINT } kind = CONSTANT;
  int idx = 0;    // REDUCED: position in S^-1; TIME: the time; POINT: the point (the problem's index)
  int size = 6;
};
// What rsba_solver_covariance_block copies: nothing (zeros: a constant block), a 6 x 6 block of S^-1, or a point's marginal.
struct CovSingle {
  enum What { ZEROS, SINV, POINT } what = ZEROS;
  int a = 0, b = 0;   // SINV: row and column in S^-1; POINT: a = the point (the problem's index)
};

// The column map of one compute.  The parameter array is [C x 6 | P x 3] (point model) or [C | T | M] x 6 (marker chain); this struct
// is the only place that knows those steps.
struct CovLayout {
  int model = RSBA_MODEL_POINTS;
  int C = 0, T = 0, M = 0, P = 0;
  int I = 0;                         // marker chain under the extended layout (CovMarkerIntrColumns): C intrinsics blocks behind [C | T | M],
                                     // camera k's at block C + T + M + k, offset 6 (C + T + M + k); 0 otherwise
  int n = 0;                         // columns of the system: six per block with pos >= 0
  std::vector<uint8_t> ref;          // per camera (point model) / per block of [C | T | M] (| the I intrinsics blocks): some residual
                                     // references it (a sharded solver: on some rank)
  std::vector<uint8_t> ref_pt;       // point model: the same per point, this rank's
  std::vector<int> pos;              // per camera / per block: its first column, -1: constant, unreferenced or eliminated
  std::vector<unsigned char> elim;   // marker chain, per time: eliminated (free, referenced, time-eliminating path); max(T, 1) entries
  std::vector<uint8_t> const_pt;     // point model: constant points (may be shorter than P: the rest is free)
  std::vector<int> pt_dev;           // point model: a point's index in the problem -> its position on the device (empty: the same)

  bool points() const { return model == RSBA_MODEL_POINTS; }
  int blocks() const { return points() ? C : C + T + M; }   // the pose blocks
  int all_blocks() const { return blocks() + I; }           // ... and the intrinsics blocks behind them: the entries of ref and pos
  bool is_time(int b) const { return !points() && b >= C && b < C + T; }
  // a block whose rows are formed: with columns, or eliminated
  bool is_free(int b) const { return pos[b] >= 0 || (is_time(b) && elim[b - C]); }
  int dev(int j) const { return pt_dev.empty() ? j : pt_dev[j]; }
  void BuildPointDev(const std::vector<int>& pt_perm) {   // pt_perm: device position -> problem point
    pt_dev.resize(pt_perm.size());
    for (size_t jn = 0; jn < pt_perm.size(); ++jn) pt_dev[pt_perm[jn]] = (int)jn;
  }

  // Offset -> block: cameras and pose blocks step by 6, points by 3 behind the poses.  RSBA_ERR_ARG: the offset starts no block.
  int BlockOf(int64_t off, bool* point, int* idx) const {
    const int64_t pose_end = 6LL * all_blocks();
    if (off < 0) return RSBA_ERR_ARG;
    if (off < pose_end) {
      if (off % 6) return RSBA_ERR_ARG;
      *point = false; *idx = (int)(off / 6);
      return RSBA_OK;
    }
    if (!points() || off >= pose_end + 3LL * P || (off - pose_end) % 3) return RSBA_ERR_ARG;
    *point = true; *idx = (int)((off - pose_end) / 3);
    return RSBA_OK;
  }
  bool Referenced(bool point, int idx) const { return (point ? ref_pt[idx] : ref[idx]) != 0; }
  CovBlockRef Classify(bool point, int idx) const {
    CovBlockRef r;
    r.size = point ? 3 : 6;
    if (point) { r.kind = idx < (int)const_pt.size() && const_pt[idx] ? CovBlockRef::CONSTANT : CovBlockRef::POINT; r.idx = idx; }
    else if (pos[idx] >= 0) { r.kind = CovBlockRef::REDUCED; r.idx = pos[idx]; }
    else if (is_time(idx) && elim[idx - C]) { r.kind = CovBlockRef::TIME; r.idx = idx - C; }
    return r;
  }
  // RSBA_ERR_ARG: the offset starts no block, or names a block no residual references (the fixed base blocks included)
  int Resolve(int64_t off, CovBlockRef* r) const {
    bool point = false;
    int idx = 0;
    if (BlockOf(off, &point, &idx) != RSBA_OK || !Referenced(point, idx)) return RSBA_ERR_ARG;
    *r = Classify(point, idx);
    return RSBA_OK;
  }
  // rsba_solver_covariance_block's answer, in the order of its checks: a malformed offset (RSBA_ERR_ARG), then a time block in
  // either position (RSBA_ERR_UNSUPPORTED: not offered, eliminated on one path), then an unreferenced block (RSBA_ERR_ARG), then
  // camera x point and cross-point blocks (RSBA_ERR_UNSUPPORTED).
  int Single(int64_t off_a, int64_t off_b, CovSingle* q) const {
    const int64_t off[2] = {off_a, off_b};
    bool point[2] = {false, false};
    int idx[2] = {0, 0};
    for (int e = 0; e < 2; ++e) if (BlockOf(off[e], &point[e], &idx[e]) != RSBA_OK) return RSBA_ERR_ARG;
    for (int e = 0; e < 2; ++e) if (!point[e] && is_time(idx[e])) return RSBA_ERR_UNSUPPORTED;
    for (int e = 0; e < 2; ++e) if (!Referenced(point[e], idx[e])) return RSBA_ERR_ARG;
    *q = CovSingle();
    if (!point[0] && !point[1]) {
      if (pos[idx[0]] >= 0 && pos[idx[1]] >= 0) { q->what = CovSingle::SINV; q->a = pos[idx[0]]; q->b = pos[idx[1]]; }
      return RSBA_OK;
    }
    if (!point[0] || !point[1] || idx[0] != idx[1]) return RSBA_ERR_UNSUPPORTED;
    q->what = CovSingle::POINT; q->a = idx[0];   // (a constant point's marginal is written as zeros by k_cov_points)
    return RSBA_OK;
  }
};

// ---- the column map --------------------------------------------------------------------------------------------------------------
// Point model, first step: this rank's referenced flags.  const_pt: the constant points.  L->pt_dev is left as it is (the point
// order belongs to the solver, not to a compute).
inline void CovPointReferenced(int C, int P, int64_t N, const int32_t* camera_index, const int32_t* point_index, const std::vector<uint8_t>& const_pt,
                               std::vector<uint8_t>* ref_cam, CovLayout* L) {
  L->model = RSBA_MODEL_POINTS; L->C = C; L->T = 0; L->M = 0; L->P = P; L->I = 0;
  L->const_pt = const_pt;
  L->elim.clear();
  ref_cam->assign(C, 0);
  L->ref_pt.assign(P, 0);
  for (int64_t i = 0; i < N; ++i) { (*ref_cam)[camera_index[i]] = 1; L->ref_pt[point_index[i]] = 1; }
}
// ... second step: the columns of the free cameras that ref_cam names — this rank's flags, or on a sharded solver the all-ranks
// sum, so that every rank lays S out alike.
inline void CovPointColumns(const std::vector<uint8_t>& ref_cam, const std::vector<uint8_t>& camera_constant, CovLayout* L) {
  L->ref = ref_cam;
  L->pos.assign(L->C, -1);
  L->n = 0;
  for (int c = 0; c < L->C; ++c) {
    const bool constant = c < (int)camera_constant.size() && camera_constant[c];
    if (L->ref[c] && !constant) { L->pos[c] = L->n; L->n += 6; }
  }
}
// Marker chain: the free referenced blocks of [C | T | M] get columns in block order; on the time-eliminating path the free
// referenced times are eliminated instead.
inline void CovMarkerColumns(const rsba_problem& p, const std::vector<uint8_t>& block_constant, bool eliminate_times, CovLayout* L) {
  const int C = p.num_cameras, T = p.num_times, M = p.num_markers, nb = C + T + M;
  L->model = p.model; L->C = C; L->T = T; L->M = M; L->P = 0; L->I = 0;
  L->ref_pt.clear(); L->const_pt.clear();
  L->ref.assign(nb, 0);
  for (int64_t i = 0; i < p.num_observations; ++i) {
    if (p.uses_camera(i)) L->ref[p.camera_block(i)] = 1;
    L->ref[p.time_block(i)] = 1;
    if (p.uses_marker(i)) L->ref[p.marker_block(i)] = 1;
  }
  L->pos.assign(nb, -1);
  L->elim.assign(std::max(T, 1), 0);
  L->n = 0;
  for (int b = 0; b < nb; ++b) {
    if (!L->ref[b] || (b < (int)block_constant.size() && block_constant[b])) continue;
    if (eliminate_times && L->is_time(b)) { L->elim[b - C] = 1; continue; }
    L->pos[b] = L->n; L->n += 6;
  }
}

// ... a solver with free intrinsics under the extended layout, behind CovMarkerColumns: one more block per camera index.  A camera an
// observation names is referenced; one with a non-zero mask gets six columns behind the pose blocks', ascending camera index (a
// held component is a constant component of it: CovPlanMarkerIntrRows); mask 0: a constant block, zeros.  intr_mask may be shorter
// than C (missing entries: 0).
inline void CovMarkerIntrColumns(const rsba_problem& p, const std::vector<int>& intr_mask, CovLayout* L) {
  const int C = L->C, nb = L->blocks();
  L->I = C;
  L->ref.resize((size_t)nb + C, 0);
  L->pos.resize((size_t)nb + C, -1);
  for (int64_t i = 0; i < p.num_observations; ++i) L->ref[nb + p.camera_index[i]] = 1;
  for (int k = 0; k < C; ++k) {
    const int mask = k < (int)intr_mask.size() ? intr_mask[k] & 63 : 0;
    if (!L->ref[nb + k] || mask == 0) continue;
    L->pos[nb + k] = L->n; L->n += 6;
  }
}

// ---- the marker chain's rows -----------------------------------------------------------------------------------------------------
// Time order, stable: the problem's order within a time.  order[q]: the observation of row q; time t owns rows [tptr[t], tptr[t + 1]).
struct CovTimeOrder { std::vector<int> tptr, order; };
inline CovTimeOrder CovOrderByTime(const rsba_problem& p) {
  CovTimeOrder o;
  const int64_t N = p.num_observations;
  o.tptr.assign(p.num_times + 1, 0);
  for (int64_t i = 0; i < N; ++i) o.tptr[p.time_index[i] + 1]++;
  for (int t = 0; t < p.num_times; ++t) o.tptr[t + 1] += o.tptr[t];
  std::vector<int> fill(o.tptr.begin(), o.tptr.end() - 1);
  o.order.resize((size_t)N);
  for (int64_t i = 0; i < N; ++i) o.order[fill[p.time_index[i]]++] = (int)i;
  return o;
}

// The row tables of a compute, as they are uploaded (max(N, 1) rows: no empty upload).
struct CovMarkerRows {
  std::vector<int> tptr;             // [T + 1]
  std::vector<CovMcRow> rows;        // in time order
  std::vector<double> obs;           // their 8 observations each
  std::vector<double> wrow;          // their weights; empty: none applied
  bool with_sub = false;             // some free block has a non-zero mask: only then are the two below built
  std::vector<unsigned char> bsub;   // per block of [C | T | M]: its constant components, 0 for a block that is not free
  std::vector<int> sub18;            // per row: the masks of its camera | time | marker block in bits 0-5 | 6-11 | 12-17
};
// weights: per observation in the problem's order, nullptr: none applied.  subset: the blocks' 6-bit masks (may be shorter than the
// block array, or empty).
inline CovMarkerRows CovPlanMarkerRows(const rsba_problem& p, const CovLayout& L, const double* weights, const std::vector<uint8_t>& subset) {
  CovMarkerRows R;
  CovTimeOrder o = CovOrderByTime(p);
  const size_t N = o.order.size(), nrows = std::max<size_t>(N, 1);
  R.tptr.swap(o.tptr);
  R.rows.resize(nrows);
  R.obs.resize(8 * nrows);
  if (weights) R.wrow.assign(nrows, 1.0);
  for (size_t q = 0; q < N; ++q) {
    const size_t i = (size_t)o.order[q];
    R.rows[q] = EvalMarkerRowOf(p, (int64_t)i);
    std::copy(p.observations.begin() + 8 * i, p.observations.begin() + 8 * i + 8, R.obs.begin() + 8 * q);
    if (weights) R.wrow[q] = weights[i];
  }
  const int nb = L.blocks();
  std::vector<unsigned char> bsub(nb, 0);
  for (int b = 0; b < nb && b < (int)subset.size(); ++b) if (L.is_free(b)) { bsub[b] = subset[b]; R.with_sub = R.with_sub || bsub[b] != 0; }
  if (R.with_sub) {
    R.sub18.assign(nrows, 0);
    for (size_t q = 0; q < N; ++q) {
      const CovMcRow& rw = R.rows[q];
      R.sub18[q] = (rw.cam_block >= 0 ? bsub[rw.cam_block] : 0) | (bsub[rw.time_block] << 6) | (rw.marker_block >= 0 ? bsub[rw.marker_block] << 12 : 0);
    }
    R.bsub.swap(bsub);
  }
  return R;
}

// ... with intrinsics blocks (CovMarkerIntrColumns ran on L): the masks are always built.  bsub has all_blocks() entries, an intrinsics
// block with columns holding its CLEAR mask bits (the components the solve does not refine); sub18 carries a row's detecting
// camera's in bits 18-23 (all six where the camera has no columns: k_cov_mc_intr_lin forms no such column anyway).
inline CovMarkerRows CovPlanMarkerIntrRows(const rsba_problem& p, const CovLayout& L, const double* weights, const std::vector<uint8_t>& subset,
                                           const std::vector<int>& intr_mask) {
  CovMarkerRows R = CovPlanMarkerRows(p, L, weights, subset);
  const int nb = L.blocks();
  const size_t N = (size_t)p.num_observations;
  if (!R.with_sub) { R.bsub.assign(nb, 0); R.sub18.assign(R.rows.size(), 0); R.with_sub = true; }
  R.bsub.resize((size_t)nb + L.I, 0);
  for (int k = 0; k < L.I; ++k)
    if (L.pos[nb + k] >= 0) R.bsub[nb + k] = (unsigned char)(~(k < (int)intr_mask.size() ? intr_mask[k] : 0) & 63);
  for (size_t q = 0; q < N; ++q) {
    const int b = nb + R.rows[q].camera;
    R.sub18[q] |= (L.pos[b] >= 0 ? R.bsub[b] : 63) << 18;
  }
  return R;
}

// Time-eliminating path: per time the distinct camera / marker blocks with columns that its rows touch, in the order of their first
// appearance — dpos[dptr[t] .. dptr[t + 1]), their positions in S^-1 — and every row's two slots among them: rslot[2 q + x] for the
// camera (x = 0) / marker (x = 1) block of row q, -1: no columns.  Rows in the compute's order.
struct CovCrossTables { std::vector<int> dptr, dpos, rslot; };
// RSBA_ERR_UNSUPPORTED: a time touches more than RSBA_COV_MC_MAXBLK blocks (k_cov_mc_cross keeps one W per block in LDS)
inline int CovPlanCrossTables(const rsba_problem& p, const CovLayout& L, CovCrossTables* out) {
  const CovTimeOrder o = CovOrderByTime(p);
  const size_t N = o.order.size();
  CovCrossTables& X = *out;
  X.dptr.assign(p.num_times + 1, 0);
  X.dpos.clear();
  X.rslot.assign(2 * std::max<size_t>(N, 1), -1);
  std::vector<int> seen_in(L.n / 6 + 1, -1), slot_of(L.n / 6 + 1, -1);   // per block with columns: the last time that touched it, its slot there
  for (int t = 0; t < p.num_times; ++t) {
    const size_t d0 = X.dpos.size();
    for (size_t q = (size_t)o.tptr[t]; q < (size_t)o.tptr[t + 1]; ++q) {
      const EvalMarkerRow rw = EvalMarkerRowOf(p, o.order[q]);
      const int blk[2] = {rw.cam_block, rw.marker_block};
      for (int x = 0; x < 2; ++x) {
        const int pos = blk[x] >= 0 ? L.pos[blk[x]] : -1;
        if (pos < 0) continue;
        if (seen_in[pos / 6] != t) { seen_in[pos / 6] = t; slot_of[pos / 6] = (int)(X.dpos.size() - d0); X.dpos.push_back(pos); }
        X.rslot[2 * q + x] = slot_of[pos / 6];
      }
    }
    if (X.dpos.size() - d0 > RSBA_COV_MC_MAXBLK) return RSBA_ERR_UNSUPPORTED;
    X.dptr[t + 1] = (int)X.dpos.size();
  }
  if (X.dpos.empty()) X.dpos.push_back(0);   // (no empty upload)
  return RSBA_OK;
}

// ---- pair queries ----------------------------------------------------------------------------------------------------------------
// The requests of one query, by kernel: k_cov_gather, k_cov_mc_cross, k_cov_pt_cross.  They are uploaded as one list, in that order.
struct CovRequests {
  std::vector<CovReq> gather, marker, point;
  size_t size() const { return gather.size() + marker.size() + point.size(); }
  std::vector<CovReq> All() const {
    std::vector<CovReq> all;
    all.reserve(size());
    all.insert(all.end(), gather.begin(), gather.end());
    all.insert(all.end(), marker.begin(), marker.end());
    all.insert(all.end(), point.begin(), point.end());
    return all;
  }
};
struct CovPair { CovBlockRef a, b; };
// ONE orientation of every pair is computed, rows x cols in its staging slot; the other is its transpose on output.
struct CovPairPlan { bool zero, transposed; int rows, cols; };
struct CovQueryPlan {
  CovRequests rq;
  std::vector<CovPairPlan> pairs;
};

// Every pair is resolved before anything is planned: one bad offset refuses the whole call.
inline int CovResolvePairs(const CovLayout& L, int64_t num_pairs, const int64_t* offsets_a, const int64_t* offsets_b, std::vector<CovPair>* pairs) {
  pairs->assign((size_t)num_pairs, CovPair());
  for (int64_t i = 0; i < num_pairs; ++i) {
    int rc;
    if ((rc = L.Resolve(offsets_a[i], &(*pairs)[i].a)) != RSBA_OK || (rc = L.Resolve(offsets_b[i], &(*pairs)[i].b)) != RSBA_OK) return rc;
  }
  return RSBA_OK;
}
// Pair i's block goes to staging slot i.  (L.pt_dev is built by then where the solver has a point order.)
inline CovQueryPlan CovPlanPairs(const CovLayout& L, const std::vector<CovPair>& pairs) {
  CovQueryPlan Q;
  CovRequests& rq = Q.rq;
  Q.pairs.resize(pairs.size());
  for (size_t i = 0; i < pairs.size(); ++i) {
    const CovBlockRef &a = pairs[i].a, &b = pairs[i].b;
    CovPairPlan& pl = Q.pairs[i];
    pl = CovPairPlan{false, false, a.size, b.size};
    const int slot = (int)i;
    if (a.kind == CovBlockRef::CONSTANT || b.kind == CovBlockRef::CONSTANT) { pl.zero = true; continue; }
    if (a.kind == CovBlockRef::REDUCED && b.kind == CovBlockRef::REDUCED) { rq.gather.push_back(CovReq{a.idx, b.idx, COV_REQ_SINV, slot}); continue; }
    if (a.kind == CovBlockRef::POINT && b.kind == CovBlockRef::POINT) {
      if (a.idx == b.idx) { rq.gather.push_back(CovReq{a.idx, a.idx, COV_REQ_POINT, slot}); continue; }
      pl.transposed = a.idx > b.idx;
      rq.point.push_back(CovReq{L.dev(std::min(a.idx, b.idx)), L.dev(std::max(a.idx, b.idx)), COV_REQ_POINT_POINT, slot});
      continue;
    }
    if (a.kind == CovBlockRef::TIME && b.kind == CovBlockRef::TIME) {
      pl.transposed = a.idx > b.idx;
      rq.marker.push_back(CovReq{std::min(a.idx, b.idx), std::max(a.idx, b.idx), COV_REQ_TIME_TIME, slot});
      continue;
    }
    // a reduced block with an eliminated one: computed as (time, x) / (camera, point)
    const bool a_reduced = a.kind == CovBlockRef::REDUCED;
    const CovBlockRef &x = a_reduced ? a : b, &e = a_reduced ? b : a;
    if (e.kind == CovBlockRef::TIME) {
      pl.transposed = a_reduced; pl.rows = 6; pl.cols = 6;
      rq.marker.push_back(CovReq{e.idx, x.idx, COV_REQ_TIME_X, slot});
    } else {
      pl.transposed = !a_reduced; pl.rows = 6; pl.cols = 3;
      rq.point.push_back(CovReq{x.idx, L.dev(e.idx), COV_REQ_CAM_POINT, slot});
    }
  }
  return Q;
}
// A pair's 36 output doubles from its staging block g: the block row-major in the pair's own orientation, zeros behind it.
inline void CovUnpackPair(const CovPairPlan& pl, const double* g, double* o) {
  const int na = pl.transposed ? pl.cols : pl.rows, nb = pl.transposed ? pl.rows : pl.cols;
  for (int e = 0; e < 36; ++e) o[e] = 0.0;
  if (pl.zero) return;
  for (int r = 0; r < na; ++r)
    for (int c = 0; c < nb; ++c) o[r * nb + c] = pl.transposed ? g[c * pl.cols + r] : g[r * pl.cols + c];
}
inline void CovUnpackPairs(const CovQueryPlan& Q, const double* staging, double* out) {
  for (size_t i = 0; i < Q.pairs.size(); ++i) CovUnpackPair(Q.pairs[i], staging + 36 * i, out + 36 * i);
}

// rsba_solver_time_covariances: the marginal of every referenced free time into slot t — on the dense path a diagonal block of S^-1.
// (Constant and unreferenced times keep the zeros of the caller's buffer.)
inline CovRequests CovPlanTimes(const CovLayout& L) {
  CovRequests rq;
  for (int t = 0; t < L.T; ++t) {
    const int b = L.C + t;
    if (!L.ref[b]) continue;
    if (L.pos[b] >= 0) rq.gather.push_back(CovReq{L.pos[b], L.pos[b], COV_REQ_SINV, t});
    else if (L.elim[t]) rq.marker.push_back(CovReq{t, t, COV_REQ_TIME_TIME, t});
  }
  return rq;
}

}  // namespace rsba
