// Stand-alone driver of csrc/ba_covariance_plan.hpp (tests/test_covariance_plan_host.py builds it with -fsanitize=address,undefined and
// runs it as a child process): the covariance's column map, the marker chain's row and cross tables, offset resolution and the plan of
// a pair query, held to what the kernels rely on.  Every check starts from the problem alone (Truth below): nothing here reads the
// planner's intermediates.  The observations of every problem are their own indices, so a planned row names the observation it came from.
//   columns   pos is -1 exactly for constant, unreferenced and eliminated blocks, else 0, 6, 12, ... in block order; elim exactly for
//             the free referenced times of the eliminating path
//   rows      tptr, the problem's order within a time, every row's blocks, observations, weight and 18-bit mask
//   cross     dpos[dptr[t] + rslot] is the block's position, rslot = -1 exactly without a column, first-appearance order, the block cap
//   queries   the driver plays the kernels: for every planned request it writes the block of a known symmetric matrix in the orientation
//             the request kind defines, and every ordered pair of offsets must unpack to that matrix's (a, b) block; the return codes
//             of every offset, of the single-pair call and the request list of the time marginals beside it
// usage: covariance_plan_driver <tests/golden/hongo/correspondence.txt>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <set>
#include <string>

#include "ba_covariance_plan.hpp"

using namespace rsba;

static long g_checks = 0;
static std::string g_case;
#define CHECK(cond)                                                                                                        \
  do {                                                                                                                     \
    ++g_checks;                                                                                                            \
    if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_case.c_str()); exit(1); }       \
  } while (0)

struct Obs { int c, t, m; };
// variant 0: Main_Calibration's wiring (camera 0 and marker 0 are the base blocks), 1: Test2's (marker 0 free)
static rsba_problem MarkerProblem(int C, int T, int M, int variant, const std::vector<Obs>& obs) {
  rsba_problem p;
  p.model = variant == 1 ? RSBA_MODEL_MARKER_CHAIN_TEST2 : RSBA_MODEL_MARKER_CHAIN;
  p.num_cameras = C; p.num_times = T; p.num_markers = M; p.marker_side = 0.1;
  for (const Obs& o : obs) { p.camera_index.push_back(o.c); p.time_index.push_back(o.t); p.marker_index.push_back(o.m); }
  p.num_observations = (int64_t)obs.size();
  p.observations.resize(8 * obs.size());
  for (size_t i = 0; i < p.observations.size(); ++i) p.observations[i] = (double)i;
  p.parameters.assign(6 * (size_t)(C + T + M), 0.0);
  p.intrinsics.assign(4 * (size_t)C, 1.0);
  return p;
}
static bool Flag(const std::vector<uint8_t>& v, int i) { return i < (int)v.size() && v[i] != 0; }

// What the problem says, block by block.
struct Truth {
  std::vector<char> ref, constant, elim;   // per pose block (elim: per pose block too, set for eliminated times)
  std::vector<char> ref_pt, const_pt;
};
static Truth MarkerTruth(const rsba_problem& p, const std::vector<uint8_t>& constant, bool elim_path) {
  const int C = p.num_cameras, T = p.num_times, nb = C + T + p.num_markers;
  Truth t;
  t.ref.assign(nb, 0); t.constant.assign(nb, 0); t.elim.assign(nb, 0);
  for (int64_t i = 0; i < p.num_observations; ++i) {
    if (p.camera_index[i] != 0) t.ref[p.camera_index[i]] = 1;
    t.ref[C + p.time_index[i]] = 1;
    if (p.model == RSBA_MODEL_MARKER_CHAIN_TEST2 || p.marker_index[i] != 0) t.ref[C + T + p.marker_index[i]] = 1;
  }
  for (int b = 0; b < nb; ++b) {
    t.constant[b] = Flag(constant, b);
    t.elim[b] = elim_path && b >= C && b < C + T && t.ref[b] && !t.constant[b];
  }
  return t;
}

// ---- columns
static void CheckColumns(const CovLayout& L, const Truth& t, bool elim_path) {
  const int nb = (int)t.ref.size();
  CHECK(L.blocks() == nb && (int)L.pos.size() == nb && (int)L.ref.size() == nb);
  int next = 0;
  for (int b = 0; b < nb; ++b) {
    CHECK((L.ref[b] != 0) == (t.ref[b] != 0));
    const bool column = t.ref[b] && !t.constant[b] && !t.elim[b];
    CHECK(L.pos[b] == (column ? next : -1));
    if (column) next += 6;
    CHECK(L.is_free(b) == (t.ref[b] && !t.constant[b]));
  }
  CHECK(L.n == next);
  if (!L.points()) {
    CHECK((int)L.elim.size() == std::max(L.T, 1));
    for (int k = 0; k < L.T; ++k) { CHECK((L.elim[k] != 0) == (t.elim[L.C + k] != 0)); if (!elim_path) CHECK(L.elim[k] == 0); }
  }
}

// ---- rows: returns the observation of every row, read from the row's own observations
static std::vector<int> CheckRows(const rsba_problem& p, const CovLayout& L, const Truth& t, const double* weights, const std::vector<uint8_t>& subset,
                                  const CovMarkerRows& R) {
  const int T = p.num_times, N = (int)p.num_observations, C = p.num_cameras;
  const size_t nrows = (size_t)std::max(N, 1);
  CHECK((int)R.tptr.size() == T + 1 && R.tptr[0] == 0 && R.tptr[T] == N && R.rows.size() == nrows && R.obs.size() == 8 * nrows);
  CHECK(weights ? R.wrow.size() == nrows : R.wrow.empty());
  std::vector<int> count(T, 0);
  for (int i = 0; i < N; ++i) count[p.time_index[i]]++;
  bool any_mask = false;
  for (int b = 0; b < (int)t.ref.size(); ++b) any_mask = any_mask || (t.ref[b] && !t.constant[b] && Flag(subset, b));
  CHECK(R.with_sub == any_mask);
  if (any_mask) CHECK(R.sub18.size() == nrows && (int)R.bsub.size() == L.blocks()); else CHECK(R.sub18.empty() && R.bsub.empty());
  auto mask = [&](int b) { return b >= 0 && t.ref[b] && !t.constant[b] && b < (int)subset.size() ? (int)subset[b] : 0; };
  for (int b = 0; any_mask && b < L.blocks(); ++b) CHECK(R.bsub[b] == mask(b));
  std::vector<int> row_obs(N, -1);
  std::vector<char> seen(N, 0);
  for (int k = 0; k < T; ++k) {
    CHECK(R.tptr[k + 1] - R.tptr[k] == count[k]);
    for (int q = R.tptr[k]; q < R.tptr[k + 1]; ++q) {
      const int i = (int)(R.obs[8 * (size_t)q] / 8);
      CHECK(i >= 0 && i < N && !seen[i] && p.time_index[i] == k);
      seen[i] = 1; row_obs[q] = i;
      if (q > R.tptr[k]) CHECK(row_obs[q - 1] < i);   // the problem's order within a time
      for (int e = 0; e < 8; ++e) CHECK(R.obs[8 * (size_t)q + e] == p.observations[8 * (size_t)i + e]);
      const CovMcRow& rw = R.rows[q];
      const bool uses_m = p.model == RSBA_MODEL_MARKER_CHAIN_TEST2 || p.marker_index[i] != 0;
      CHECK(rw.cam_block == (p.camera_index[i] != 0 ? p.camera_index[i] : -1) && rw.time_block == C + k);
      CHECK(rw.marker_block == (uses_m ? C + T + p.marker_index[i] : -1) && rw.camera == p.camera_index[i]);
      if (weights) CHECK(R.wrow[q] == weights[i]);
      if (any_mask) CHECK(R.sub18[q] == (mask(rw.cam_block) | (mask(rw.time_block) << 6) | (mask(rw.marker_block) << 12)));
    }
  }
  return row_obs;
}

// ---- cross tables
static void CheckCross(const rsba_problem& p, const CovLayout& L, const std::vector<int>& tptr, const std::vector<int>& row_obs, const CovCrossTables& X) {
  const int T = p.num_times, N = (int)p.num_observations, C = p.num_cameras;
  CHECK((int)X.dptr.size() == T + 1 && X.dptr[0] == 0 && X.rslot.size() == 2 * (size_t)std::max(N, 1) && !X.dpos.empty());
  for (int k = 0; k < T; ++k) {
    std::vector<int> first;   // the positions of the time's blocks with columns, by first appearance
    for (int q = tptr[k]; q < tptr[k + 1]; ++q) {
      const int i = row_obs[q];
      const bool uses_m = p.model == RSBA_MODEL_MARKER_CHAIN_TEST2 || p.marker_index[i] != 0;
      const int blk[2] = {p.camera_index[i] != 0 ? p.camera_index[i] : -1, uses_m ? C + T + p.marker_index[i] : -1};
      for (int x = 0; x < 2; ++x) {
        const int pos = blk[x] >= 0 ? L.pos[blk[x]] : -1, slot = X.rslot[2 * (size_t)q + x];
        CHECK((slot == -1) == (pos < 0));
        if (pos < 0) continue;
        if (std::find(first.begin(), first.end(), pos) == first.end()) first.push_back(pos);
        CHECK(slot >= 0 && X.dptr[k] + slot < X.dptr[k + 1] && X.dpos[X.dptr[k] + slot] == pos);
      }
    }
    CHECK(X.dptr[k + 1] - X.dptr[k] == (int)first.size() && first.size() <= RSBA_COV_MC_MAXBLK);
    for (size_t d = 0; d < first.size(); ++d) CHECK(X.dpos[X.dptr[k] + d] == first[d]);
  }
  if (N == 0) CHECK(X.rslot[0] == -1 && X.rslot[1] == -1);
}

// ---- resolve, the pair plan and its unpacking, end to end
static double Sigma(int64_t i, int64_t j) { return (double)(std::min(i, j) * 8192 + std::max(i, j) + 1); }   // symmetric, every entry its own

struct Blocks {   // the parameter array of a layout, from the truth: offsets, sizes and what each block is
  std::vector<int64_t> off;
  std::vector<int> size;
  std::vector<char> ok, constant, time;   // ok: referenced
  int64_t end = 0;
};
static Blocks AllBlocks(const CovLayout& L, const Truth& t) {
  Blocks B;
  const int nb = (int)t.ref.size();
  for (int b = 0; b < nb; ++b) {
    B.off.push_back(6LL * b); B.size.push_back(6); B.ok.push_back(t.ref[b]); B.constant.push_back(t.constant[b]);
    B.time.push_back(!L.points() && b >= L.C && b < L.C + L.T);
  }
  for (int j = 0; j < (int)t.ref_pt.size(); ++j) {
    B.off.push_back(6LL * nb + 3LL * j); B.size.push_back(3); B.ok.push_back(t.ref_pt[j]); B.constant.push_back(t.const_pt[j]); B.time.push_back(0);
  }
  B.end = 6LL * nb + 3LL * (int64_t)t.ref_pt.size();
  return B;
}

// The kernels' side of a query: every request's block of Sigma into its staging slot, in the orientation its kind defines.
static void PlayKernels(const CovLayout& L, const std::vector<int>& pt_perm, const CovRequests& rq, std::vector<double>* staging) {
  const int nb = L.blocks();
  std::vector<int> block_at(L.n / 6 + 1, -1);
  for (int b = 0; b < nb; ++b) if (L.pos[b] >= 0) block_at[L.pos[b] / 6] = b;
  auto pose_at = [&](int pos) { CHECK(pos >= 0 && pos % 6 == 0 && pos < L.n && block_at[pos / 6] >= 0); return 6LL * block_at[pos / 6]; };
  auto time_at = [&](int k) { CHECK(k >= 0 && k < L.T && L.elim[k]); return 6LL * (L.C + k); };
  auto point_at = [&](int j) { CHECK(j >= 0 && j < L.P); return 6LL * nb + 3LL * j; };
  auto problem_point = [&](int dev) { CHECK(dev >= 0 && dev < L.P); return pt_perm.empty() ? dev : pt_perm[dev]; };
  const std::vector<CovReq> all = rq.All();
  CHECK(all.size() == rq.size());
  std::set<int> slots;
  for (size_t k = 0; k < all.size(); ++k) {
    const CovReq& r = all[k];
    const int list = k < rq.gather.size() ? 0 : k < rq.gather.size() + rq.marker.size() ? 1 : 2;   // gather | marker | point
    const CovReq& same = list == 0 ? rq.gather[k] : list == 1 ? rq.marker[k - rq.gather.size()] : rq.point[k - rq.gather.size() - rq.marker.size()];
    CHECK(r.a == same.a && r.b == same.b && r.kind == same.kind && r.out == same.out);
    CHECK(r.out >= 0 && 36 * (size_t)r.out + 36 <= staging->size() && slots.insert(r.out).second);
    int64_t ra = 0, cb = 0;
    int rows = 6, cols = 6;
    switch (r.kind) {
      case COV_REQ_SINV: CHECK(list == 0); ra = pose_at(r.a); cb = pose_at(r.b); break;
      case COV_REQ_POINT: CHECK(list == 0 && r.a == r.b); ra = cb = point_at(r.a); rows = cols = 3; break;
      case COV_REQ_TIME_TIME: CHECK(list == 1 && r.a <= r.b); ra = time_at(r.a); cb = time_at(r.b); break;
      case COV_REQ_TIME_X: CHECK(list == 1); ra = time_at(r.a); cb = pose_at(r.b); break;
      case COV_REQ_CAM_POINT: CHECK(list == 2); ra = pose_at(r.a); cb = point_at(problem_point(r.b)); cols = 3; break;
      case COV_REQ_POINT_POINT:
        CHECK(list == 2 && problem_point(r.a) < problem_point(r.b));
        ra = point_at(problem_point(r.a)); cb = point_at(problem_point(r.b)); rows = cols = 3;
        break;
      default: CHECK(false);
    }
    for (int i = 0; i < rows; ++i) for (int j = 0; j < cols; ++j) (*staging)[36 * (size_t)r.out + (size_t)i * cols + j] = Sigma(ra + i, cb + j);
  }
}

static void CheckQueries(CovLayout& L, const Truth& t, const std::vector<int>& pt_perm) {
  const Blocks B = AllBlocks(L, t);
  const int nblk = (int)B.off.size();
  // every offset: OK exactly for the start of a referenced block
  std::vector<int> good;
  for (int64_t off = -2; off <= B.end + 7; ++off) {
    int b = 0;
    while (b < nblk && B.off[b] != off) ++b;
    CovBlockRef r;
    const int rc = L.Resolve(off, &r);
    CHECK(rc == (b < nblk && B.ok[b] ? RSBA_OK : RSBA_ERR_ARG));
    if (rc == RSBA_OK) { good.push_back(b); CHECK(r.size == B.size[b] && (r.kind == CovBlockRef::CONSTANT) == (B.constant[b] != 0)); }
  }
  // every ordered pair of them in one call
  std::vector<int64_t> oa, ob;
  for (int a : good) for (int b : good) { oa.push_back(B.off[a]); ob.push_back(B.off[b]); }
  std::vector<CovPair> pairs;
  CHECK(CovResolvePairs(L, (int64_t)oa.size(), oa.data(), ob.data(), &pairs) == RSBA_OK && pairs.size() == oa.size());
  if (L.points() && L.pt_dev.empty() && !pt_perm.empty()) L.BuildPointDev(pt_perm);
  const CovQueryPlan Q = CovPlanPairs(L, pairs);
  CHECK(Q.pairs.size() == oa.size());
  std::vector<double> staging(36 * oa.size() + 1, NAN), out(36 * oa.size() + 1, NAN);
  PlayKernels(L, pt_perm, Q.rq, &staging);
  CovUnpackPairs(Q, staging.data(), out.data());
  size_t i = 0;
  for (int a : good) for (int b : good) {
    const CovPairPlan& pl = Q.pairs[i];
    const bool zero = B.constant[a] || B.constant[b];
    CHECK(pl.zero == zero && (pl.transposed ? pl.cols : pl.rows) == B.size[a] && (pl.transposed ? pl.rows : pl.cols) == B.size[b]);
    const double* o = &out[36 * i];
    const double* mirror = &out[36 * ((i % good.size()) * good.size() + i / good.size())];   // the pair (b, a)
    for (int e = 0; e < 36; ++e) {
      const int r = e / B.size[b], c = e % B.size[b];
      const bool inside = e < B.size[a] * B.size[b];
      CHECK(o[e] == (inside && !zero ? Sigma(B.off[a] + r, B.off[b] + c) : 0.0));
      if (inside) CHECK(o[e] == mirror[c * B.size[a] + r]);
    }
    ++i;
  }
  // one bad offset refuses the whole call
  if (!oa.empty()) { oa.back() = B.end; CHECK(CovResolvePairs(L, (int64_t)oa.size(), oa.data(), ob.data(), &pairs) == RSBA_ERR_ARG); }
  // the single-pair call: its return codes, in the order of its checks, and what it copies
  std::vector<int> start_of((size_t)B.end + 1, -1);
  for (int b = 0; b < nblk; ++b) start_of[B.off[b]] = b;
  auto start = [&](int64_t off) { return off >= 0 && off < B.end ? start_of[off] : -1; };
  for (int64_t offa = -1; offa <= B.end + 1; ++offa) for (int64_t offb = -1; offb <= B.end + 1; ++offb) {
    const int a = start(offa), b = start(offb);
    CovSingle q;
    const int rc = L.Single(offa, offb, &q);
    int want = RSBA_OK;
    if (a < 0 || b < 0) want = RSBA_ERR_ARG;
    else if (B.time[a] || B.time[b]) want = RSBA_ERR_UNSUPPORTED;
    else if (!B.ok[a] || !B.ok[b]) want = RSBA_ERR_ARG;
    else if ((B.size[a] == 3 || B.size[b] == 3) && a != b) want = RSBA_ERR_UNSUPPORTED;
    CHECK(rc == want);
    if (rc != RSBA_OK) continue;
    if (B.size[a] == 3) CHECK(q.what == CovSingle::POINT && 6LL * L.blocks() + 3LL * q.a == offa);
    else if (B.constant[a] || B.constant[b]) CHECK(q.what == CovSingle::ZEROS);
    else CHECK(q.what == CovSingle::SINV && q.a == L.pos[a] && q.b == L.pos[b] && q.a >= 0 && q.b >= 0);
  }
  // the time marginals: every referenced free time once, into slot t
  if (!L.points()) {
    const CovRequests rq = CovPlanTimes(L);
    CHECK(rq.point.empty());
    size_t g = 0, m = 0;
    for (int k = 0; k < L.T; ++k) {
      const int b = L.C + k;
      if (!t.ref[b] || t.constant[b]) continue;
      if (t.elim[b]) { CHECK(m < rq.marker.size()); const CovReq& r = rq.marker[m++]; CHECK(r.a == k && r.b == k && r.kind == COV_REQ_TIME_TIME && r.out == k); }
      else { CHECK(g < rq.gather.size()); const CovReq& r = rq.gather[g++]; CHECK(r.a == L.pos[b] && r.b == r.a && r.a >= 0 && r.kind == COV_REQ_SINV && r.out == k); }
    }
    CHECK(g == rq.gather.size() && m == rq.marker.size());
  }
}

// One marker-chain problem through everything, on one path
static void CheckMarker(const std::string& name, rsba_problem p, const std::vector<uint8_t>& constant, const std::vector<uint8_t>& subset,
                        const std::vector<double>& weights, bool elim_path) {
  g_case = name + (elim_path ? " (eliminating)" : " (dense)");
  p.block_constant = constant;
  const Truth t = MarkerTruth(p, constant, elim_path);
  CovLayout L;
  CovMarkerColumns(p, p.block_constant, elim_path, &L);
  CHECK(L.model == p.model && L.C == p.num_cameras && L.T == p.num_times && L.M == p.num_markers && L.P == 0);
  CheckColumns(L, t, elim_path);
  const double* w = weights.empty() ? nullptr : weights.data();
  const CovMarkerRows R = CovPlanMarkerRows(p, L, w, subset);
  const std::vector<int> row_obs = CheckRows(p, L, t, w, subset, R);
  CovCrossTables X;
  CHECK(CovPlanCrossTables(p, L, &X) == RSBA_OK);
  CheckCross(p, L, R.tptr, row_obs, X);
  CheckQueries(L, t, {});
}

// One point-model problem: this rank's flags, and the all-ranks flags `summed` (empty: one rank)
static void CheckPoints(const std::string& name, int C, int P, const std::vector<int32_t>& cam, const std::vector<int32_t>& pt, const std::vector<uint8_t>& cconst,
                        const std::vector<uint8_t>& pconst, const std::vector<int>& pt_perm, const std::vector<uint8_t>& other_rank) {
  g_case = name;
  Truth t;
  t.ref.assign(C, 0); t.constant.assign(C, 0); t.elim.assign(C, 0); t.ref_pt.assign(P, 0); t.const_pt.assign(P, 0);
  for (size_t i = 0; i < cam.size(); ++i) { t.ref[cam[i]] = 1; t.ref_pt[pt[i]] = 1; }
  for (int c = 0; c < C; ++c) t.constant[c] = Flag(cconst, c);
  for (int j = 0; j < P; ++j) t.const_pt[j] = Flag(pconst, j);
  CovLayout L;
  L.pt_dev.assign(3, 7);   // (a compute leaves the point order's inverse alone)
  std::vector<uint8_t> ref_cam;
  CovPointReferenced(C, P, (int64_t)cam.size(), cam.data(), pt.data(), pconst, &ref_cam, &L);
  CHECK((int)ref_cam.size() == C && (int)L.ref_pt.size() == P && L.pt_dev.size() == 3);
  for (int c = 0; c < C; ++c) CHECK((ref_cam[c] != 0) == (t.ref[c] != 0));
  for (int j = 0; j < P; ++j) CHECK((L.ref_pt[j] != 0) == (t.ref_pt[j] != 0));
  L.pt_dev.clear();
  for (int c = 0; c < C && !other_rank.empty(); ++c) if (other_rank[c]) { ref_cam[c] = 1; t.ref[c] = 1; }   // the all-ranks sum
  CovPointColumns(ref_cam, cconst, &L);
  CHECK(L.points() && L.C == C && L.P == P);
  CheckColumns(L, t, false);
  for (int c = 0; c < C && !other_rank.empty(); ++c) if (other_rank[c] && !t.constant[c]) CHECK(L.pos[c] >= 0);   // a column for another rank's camera
  CheckQueries(L, t, pt_perm);
  if (!pt_perm.empty()) for (int jn = 0; jn < P; ++jn) CHECK(L.dev(pt_perm[jn]) == jn);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s correspondence.txt\n", argv[0]); return 2; }
  {
    // the hongo wiring, as RSBA_MODEL_MARKER_CHAIN and as _TEST2, on both paths
    std::ifstream f(argv[1]);
    int T = 0, C = 0, M = 0, N = 0;
    f >> T >> C >> M >> N;
    CHECK(f.good() && T > 0 && C > 0 && M > 0 && N > 0);
    double skip;
    for (int i = 0; i < T * (1 + C); ++i) f >> skip;
    std::vector<Obs> obs(N);
    for (int i = 0; i < N; ++i) { f >> obs[i].t >> obs[i].c >> obs[i].m; for (int e = 0; e < 8; ++e) f >> skip; }
    CHECK(f.good());
    for (int variant = 0; variant < 2; ++variant) for (int elim = 0; elim < 2; ++elim)
      CheckMarker(variant ? "hongo test2" : "hongo", MarkerProblem(C, T, M, variant, obs), {}, {}, {}, elim != 0);
    printf("hongo: %d observations checked\n", N);
  }
  {
    // a rig, its times interleaved (the time order has work to do): camera 4 and marker 3 unreferenced, time 2 without rows, a constant
    // camera, a constant time and a constant marker (the flags shorter than the block array), subset masks on free, constant and
    // unreferenced blocks, weights
    const int C = 5, T = 6, M = 4;
    std::vector<Obs> obs;
    for (int c = 0; c < 4; ++c) for (int t = 0; t < T; ++t) for (int m = 0; m < 3; ++m) if (t != 2 && (c + t + m) % 4 != 0) obs.push_back(Obs{c, t, m});
    std::vector<uint8_t> constant(C + T + 2, 0), subset(C + T + M, 0);
    constant[2] = 1; constant[C + 4] = 1; constant[C + T + 1] = 1;
    subset[1] = 0b000101; subset[2] = 0b111000; subset[4] = 0b000001; subset[C + 1] = 0b100000; subset[C + 4] = 0b000011; subset[C + T + 2] = 0b010010;
    std::vector<double> weights(obs.size());
    for (size_t i = 0; i < weights.size(); ++i) weights[i] = 0.25 * (double)(i % 9);
    for (int variant = 0; variant < 2; ++variant) for (int elim = 0; elim < 2; ++elim) {
      const rsba_problem p = MarkerProblem(C, T, M, variant, obs);
      CheckMarker("rig", p, constant, subset, weights, elim != 0);
      CheckMarker("rig, no flags", p, {}, {}, {}, elim != 0);
      CheckMarker("rig, masks on constant blocks only", p, constant, {0, 0, 0b000111}, weights, elim != 0);
    }
    printf("rig: %zu observations checked\n", obs.size());
  }
  {
    // a time that touches exactly RSBA_COV_MC_MAXBLK blocks with columns plans; one more is refused
    const int K = RSBA_COV_MC_MAXBLK / 2;
    std::vector<Obs> obs;
    for (int k = 0; k < K; ++k) obs.push_back(Obs{k + 1, 0, k});
    rsba_problem p = MarkerProblem(K + 1, 1, K + 1, 1, obs);
    CheckMarker("a full time", p, {}, {}, {}, true);
    obs.push_back(Obs{1, 0, K});
    p = MarkerProblem(K + 1, 1, K + 1, 1, obs);
    g_case = "a time too wide";
    CovLayout L;
    CovMarkerColumns(p, {}, true, &L);
    CovCrossTables X;
    CHECK(CovPlanCrossTables(p, L, &X) == RSBA_ERR_UNSUPPORTED);
    CovMarkerColumns(p, {}, false, &L);   // (the dense path has columns for everything; the tables are not built there, the cap is the same)
    CHECK(CovPlanCrossTables(p, L, &X) == RSBA_ERR_UNSUPPORTED);
    std::vector<uint8_t> constant(K + 1 + 1 + K + 1, 0);
    constant[K + 1 + 1 + K] = 1;   // ... and a constant block does not count
    CheckMarker("a full time and a constant block", p, constant, {}, {}, true);
    printf("block cap checked\n");
  }
  {
    // point model: camera 3 and point 5 unreferenced, a constant camera, constant points (one of them unreferenced), the flags shorter
    // than the arrays, a point order that is not the identity, and a second rank that references cameras 3 and 0
    const int C = 6, P = 9;
    std::vector<int32_t> cam, pt;
    for (int j = 0; j < P; ++j) for (int c = 0; c < C; ++c) if (j != 5 && c != 3 && (c + 2 * j) % 3 != 0) { cam.push_back(c); pt.push_back(j); }
    const std::vector<int> perm = {4, 0, 8, 2, 6, 1, 7, 3, 5};
    CheckPoints("points", C, P, cam, pt, {}, {}, {}, {});
    CheckPoints("points, constants and a point order", C, P, cam, pt, {0, 1}, {0, 0, 1, 0, 0, 1, 1}, perm, {});
    CheckPoints("points, two ranks", C, P, cam, pt, {1}, {0, 0, 0, 1}, perm, {1, 0, 0, 1, 0, 0});
    printf("point model: %zu observations checked\n", cam.size());
  }
  {
    // the empty problem and one observation
    for (int elim = 0; elim < 2; ++elim) {
      CheckMarker("empty", MarkerProblem(2, 2, 2, 0, {}), {}, {}, {}, elim != 0);
      CheckMarker("empty, no blocks", MarkerProblem(0, 0, 0, 0, {}), {}, {}, {}, elim != 0);
      CheckMarker("one observation", MarkerProblem(2, 2, 2, 0, {Obs{1, 1, 1}}), {}, {0, 0b000001}, {2.0}, elim != 0);
      CheckMarker("one observation of the base blocks", MarkerProblem(2, 2, 2, 0, {Obs{0, 0, 0}}), {}, {}, {}, elim != 0);
    }
    CheckPoints("empty points", 2, 3, {}, {}, {}, {}, {}, {});
    CheckPoints("no points at all", 0, 0, {}, {}, {}, {}, {}, {});
    CheckPoints("one point observation", 2, 3, {1}, {2}, {}, {}, {2, 0, 1}, {});
    printf("empty and single-observation problems checked\n");
  }
  printf("covariance plan driver: ok (%ld checks)\n", g_checks);
  return 0;
}
