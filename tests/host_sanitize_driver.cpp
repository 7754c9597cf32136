// AddressSanitizer / UBSan exercise of the HOST side of librsba (file readers, problem container, writers, the front
// end's initial-guess math, and the planning of the point model's set-up, ba_schur_plan.cpp): the host translation units
// are compiled with -fsanitize=address,undefined together with this driver and run by tests/test_host_sanitize.py; a
// second build with -fsanitize=thread runs the planning section alone (its point dealing writes one counter array from up
// to eight threads).  The kernels (ba_solver.hip) are not part of the build: rsba::DeviceCount is stubbed to 0, and no solve
// entry point is called.  Test infrastructure only.
//   usage: host_sanitize_driver <tests/golden> <scratch dir>     everything
//          host_sanitize_driver --plans                          the planning section only
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "ba_schur_plan.hpp"
#include "rsba.h"

namespace rsba { int DeviceCount() { return 0; } }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); exit(2); } } while (0)

static void WriteFile(const std::string& path, const std::string& text) {
  FILE* f = fopen(path.c_str(), "w");
  CHECK(f != nullptr);
  fputs(text.c_str(), f);
  fclose(f);
}

// ------------------------------------------------------------------------------------------------
// The planning of the point model's set-up (ba_schur_plan.cpp): plans for synthetic visibilities, checked against the
// contracts the kernels of ba_schur_tiled.hpp rely on.
// ------------------------------------------------------------------------------------------------
namespace {
using rsba::PointLayout;
using rsba::SchurPlan;
using rsba::SchurPlanSwitches;
using rsba::SchurSeg;

struct Lcg {
  uint64_t st;
  uint32_t next() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 33); }
};

// a point problem: every point seen by `views` distinct cameras (all of them when dense), observations in shuffled order
struct Visibility {
  int C = 0, P = 0;
  std::vector<int32_t> cam, pt;
  std::vector<double> uv;
  int64_t N() const { return (int64_t)cam.size(); }
};
Visibility MakeVisibility(int C, int P, bool dense, uint64_t seed) {
  Visibility vis; vis.C = C; vis.P = P;
  Lcg r{seed};
  std::vector<int> cams(C);
  for (int j = 0; j < P; ++j) {
    for (int c = 0; c < C; ++c) cams[c] = c;
    const int k = dense ? C : std::min(C, 2 + (int)(r.next() % 9));
    for (int i = 0; i < k; ++i) { std::swap(cams[i], cams[i + r.next() % (C - i)]); vis.cam.push_back(cams[i]); vis.pt.push_back(j); }
  }
  for (int64_t i = vis.N() - 1; i > 0; --i) { const int64_t o = r.next() % (i + 1); std::swap(vis.cam[i], vis.cam[o]); std::swap(vis.pt[i], vis.pt[o]); }
  for (int64_t i = 0; i < vis.N(); ++i) { vis.uv.push_back(vis.pt[i] + 0.25); vis.uv.push_back(vis.cam[i] + 0.5); }
  return vis;
}

bool IsPermutation(const std::vector<int>& v, size_t n) {
  if (v.size() != n) return false;
  std::vector<char> seen(n, 0);
  for (int x : v) { if (x < 0 || (size_t)x >= n || seen[x]) return false; seen[x] = 1; }
  return true;
}

void CheckLayout(const Visibility& vis, const PointLayout& lay) {
  const int P = vis.P; const int64_t N = vis.N();
  // point order: empty or a permutation; the CSR is the problem's observations, by (device point, camera)
  CHECK(lay.pt_perm.empty() || IsPermutation(lay.pt_perm, P));
  CHECK((int)lay.ptr.size() == P + 1 && lay.ptr[0] == 0 && lay.ptr[P] == N);
  CHECK((int64_t)lay.cam.size() == N && (int64_t)lay.u.size() == N && (int64_t)lay.v.size() == N && (int64_t)lay.order.size() == N);
  std::vector<char> seen(N, 0);
  int maxk = 0;
  for (int j = 0; j < P; ++j) {
    CHECK(lay.ptr[j + 1] >= lay.ptr[j]);
    maxk = std::max(maxk, lay.ptr[j + 1] - lay.ptr[j]);
    for (int q = lay.ptr[j]; q < lay.ptr[j + 1]; ++q) {
      const int64_t i = lay.order[q];
      CHECK(i >= 0 && i < N && !seen[i]);
      seen[i] = 1;
      CHECK(vis.pt[i] == (lay.pt_perm.empty() ? j : lay.pt_perm[j]) && vis.cam[i] == lay.cam[q]);
      CHECK(lay.u[q] == vis.uv[2 * i] && lay.v[q] == vis.uv[2 * i + 1]);
      CHECK(q == lay.ptr[j] || lay.cam[q - 1] < lay.cam[q]);
    }
  }
  CHECK(maxk == lay.max_views && !lay.duplicate);
  // sliced layout: every CSR position exactly once, pads are -1
  const int nslices = (P + 63) / 64;
  CHECK((int)lay.sl_ptr.size() == nslices + 1 && lay.sl_ptr[0] == 0);
  CHECK(lay.sl_elems == (size_t)lay.sl_ptr[nslices] * 64 && lay.sl_q.size() == lay.sl_elems);
  CHECK(lay.sl_cam.size() == std::max<size_t>(lay.sl_elems, 1) && lay.sl_uv.size() == std::max<size_t>(2 * lay.sl_elems, 2));
  std::vector<char> placed(N, 0);
  for (int sl = 0; sl < nslices; ++sl) {
    int w = 0;
    for (int j = 64 * sl; j < std::min(P, 64 * sl + 64); ++j) w = std::max(w, lay.ptr[j + 1] - lay.ptr[j]);
    CHECK(lay.sl_ptr[sl + 1] - lay.sl_ptr[sl] == w);
    for (int row = 0; row < w; ++row)
      for (int lane = 0; lane < 64; ++lane) {
        const size_t e = ((size_t)lay.sl_ptr[sl] + row) * 64 + lane;
        const int j = 64 * sl + lane;
        if (j < P && row < lay.ptr[j + 1] - lay.ptr[j]) {
          const int q = lay.ptr[j] + row;
          CHECK(lay.sl_q[e] == q && !placed[q] && lay.sl_cam[e] == lay.cam[q] && lay.sl_uv[2 * e] == lay.u[q] && lay.sl_uv[2 * e + 1] == lay.v[q]);
          placed[q] = 1;
        } else {
          CHECK(lay.sl_q[e] == -1 && lay.sl_cam[e] == -1);
        }
      }
  }
  for (int64_t q = 0; q < N; ++q) CHECK(placed[q]);
}

// the tiles of a plan as its segment table tells them: compute segments [s0, s1) and the reducer entries
struct TileView { int s0 = 0, s1 = 0, ga = 0, gb = 0; bool self = false; std::vector<int> red; };

std::vector<TileView> CheckSegments(const SchurPlan& pl, bool staged) {
  const std::vector<SchurSeg>& sg = pl.sg;
  const int nW = (pl.P + 63) / 64;
  CHECK(pl.ngroups == (pl.C + RSBA_TG - 1) / RSBA_TG && pl.nwords % RSBA_CW == 0 && pl.nwords >= nW && pl.nwords - nW < RSBA_CW && pl.nchunks * RSBA_CW == pl.nwords);
  CHECK((int)sg.size() == pl.nblocks && pl.nseg <= pl.nblocks && pl.nseg_pair <= pl.nseg);
  CHECK(pl.nsync == pl.ngrp + 2 * pl.ntiles + RSBA_MAX_STAGES + 2);
  CHECK(!staged || pl.nstages <= RSBA_MAX_STAGES);
  std::vector<TileView> tiles;
  int ngrp = 0, pair_segs = -1;
  for (int q = 0; q < pl.nseg;) {
    // segments: the tile's word ranges tile [0, nW) in order
    TileView tv; tv.s0 = q; tv.ga = sg[q].ga; tv.gb = sg[q].gb; tv.self = sg[q].self == 1;
    const int t = (int)tiles.size();
    CHECK(sg[q].word_begin == 0);
    int grp_left = 0, grp_first = 0, grp = sg[q].tile_grp0 - 1, groups = 0;
    CHECK(sg[q].tile_grp0 == ngrp);
    for (; q < pl.nseg && sg[q].tile == t; ++q) {
      const SchurSeg& e = sg[q];
      CHECK(e.index == q && e.ga == tv.ga && e.gb == tv.gb && (e.self == 1) == tv.self && (e.self == 0 || e.self == 1) && (e.self == 0) == (q < pl.nseg_pair));
      CHECK(tv.self ? e.ga == e.gb : e.ga <= e.gb);
      CHECK(e.ga >= 0 && e.gb < pl.ngroups);
      CHECK(q == tv.s0 || e.word_begin == sg[q - 1].word_end);
      CHECK(e.word_end > e.word_begin || nW == 0);
      // groups: consecutive segments, consecutive numbers
      if (grp_left == 0) { grp_first = q; grp_left = e.grp_nseg; ++grp; ++groups; CHECK(e.grp_nseg >= 1); }
      CHECK(e.grp == grp && e.grp_seg0 == grp_first && e.grp_nseg == sg[grp_first].grp_nseg);
      --grp_left;
      CHECK(e.tile_grp0 == ngrp && e.tile_ngrp == sg[tv.s0].tile_ngrp && e.nred == sg[tv.s0].nred);
      CHECK(e.stage >= 0 && e.stage < pl.nstages && e.stage == sg[tv.s0].stage);
    }
    tv.s1 = q;
    CHECK(grp_left == 0 && sg[q - 1].word_end == nW && groups == sg[tv.s0].tile_ngrp);
    ngrp += groups;
    const int nred = sg[tv.s0].nred;
    CHECK((nred == 0) == (groups <= RSBA_DIRECT_GROUPS) && (nred == 0 || nred == (tv.self ? RSBA_SELF_SETS : 4)));
    if (!tv.self) { CHECK(pair_segs < 0 || pair_segs == tv.s1 - tv.s0); pair_segs = tv.s1 - tv.s0; }
    tiles.push_back(tv);
  }
  CHECK((int)tiles.size() == pl.ntiles && ngrp == pl.ngrp);
  // the tiles: every pair of groups that has an off-diagonal pair once, every group's self tile once
  {
    std::vector<int> pair_seen(pl.ngroups * pl.ngroups, 0), self_seen(pl.ngroups, 0);
    for (const TileView& tv : tiles) { if (tv.self) ++self_seen[tv.ga]; else ++pair_seen[tv.ga * pl.ngroups + tv.gb]; }
    for (int ga = 0; ga < pl.ngroups; ++ga) {
      CHECK(self_seen[ga] == 1);
      for (int gb = ga; gb < pl.ngroups; ++gb) CHECK(pair_seen[ga * pl.ngroups + gb] == ((ga == gb && std::min(RSBA_TG, pl.C - RSBA_TG * ga) < 2) ? 0 : 1));
    }
  }
  // reducers: behind the compute segments, nred per tile, each a copy of its tile's numbers
  for (int q = pl.nseg; q < pl.nblocks; ++q) {
    const SchurSeg& e = sg[q];
    CHECK(e.index == q && e.tile >= 0 && e.tile < pl.ntiles);
    TileView& tv = tiles[e.tile];
    const SchurSeg& f = sg[tv.s0];
    CHECK(e.self == (tv.self ? 3 : 2) && e.nred == f.nred && e.stage == f.stage && e.tile_grp0 == f.tile_grp0 && e.tile_ngrp == f.tile_ngrp && e.ga == f.ga && e.gb == f.gb);
    CHECK(e.word_begin == (int)tv.red.size() && e.word_end > e.word_begin);
    tv.red.push_back(q);
  }
  // stages: the arrivals at a stage's counter — per tile its reducers, or its one finisher
  std::vector<int> arrivals(pl.nstages, 0);
  int self_arrivals = 0;
  for (const TileView& tv : tiles) {
    const SchurSeg& f = sg[tv.s0];
    CHECK((int)tv.red.size() == f.nred);
    const int n = f.nred ? f.nred : 1;
    arrivals[f.stage] += n;
    if (tv.self) self_arrivals += n;
  }
  for (const SchurSeg& e : sg) CHECK(e.stage_ntiles == arrivals[e.stage]);
  CHECK(self_arrivals == pl.self_arrivals);
  return tiles;
}

// every reducer entry of `order` comes after every compute segment of its tile (no deadlock: a reducer holds a workgroup slot
// while it waits, and tickets are drawn in this order)
void CheckReducersLast(const SchurPlan& pl, const std::vector<TileView>& tiles, const std::vector<int>& order) {
  std::vector<int> pos(pl.nblocks, -1);
  for (size_t b = 0; b < order.size(); ++b) pos[order[b]] = (int)b;
  for (const TileView& tv : tiles)
    for (int r : tv.red) {
      if (pos[r] < 0) continue;
      for (int q = tv.s0; q < tv.s1; ++q) CHECK(pos[q] >= 0 && pos[q] < pos[r]);
    }
}

void CheckOrders(const SchurPlan& pl, const std::vector<TileView>& tiles, bool staged) {
  CHECK(IsPermutation(pl.border, pl.nblocks));
  CHECK(pl.border_first.empty() || IsPermutation(pl.border_first, pl.nblocks));
  CHECK(!staged || !pl.border_first.empty());
  std::vector<int> self_entries;
  for (const TileView& tv : tiles) if (tv.self) { for (int q = tv.s0; q < tv.s1; ++q) self_entries.push_back(q); for (int r : tv.red) self_entries.push_back(r); }
  std::vector<int> got(pl.border_self);
  std::sort(got.begin(), got.end()); std::sort(self_entries.begin(), self_entries.end());
  CHECK(got == self_entries && (int)got.size() == pl.nblocks_self);
  CheckReducersLast(pl, tiles, pl.border);
  CheckReducersLast(pl, tiles, pl.border_first);
  CheckReducersLast(pl, tiles, pl.border_self);
}

void CheckMasks(const PointLayout& lay, const SchurPlan& pl) {
  const int P = pl.P, ncam = pl.ngroups * RSBA_TG, nwords = pl.nwords;
  const int64_t N = lay.ptr[P];
  CHECK(pl.mask.size() == (size_t)ncam * nwords && pl.prefix.size() == pl.mask.size() && (int)pl.cptr.size() == ncam + 1);
  std::vector<int> nobs(ncam, 0);
  size_t bits = 0;
  for (int j = 0; j < P; ++j) for (int q = lay.ptr[j]; q < lay.ptr[j + 1]; ++q) { ++nobs[lay.cam[q]]; CHECK((pl.mask[(size_t)lay.cam[q] * nwords + (j >> 6)] >> (j & 63)) & 1ull); }
  CHECK(pl.cptr[0] == 0);
  for (int c = 0; c < ncam; ++c) {
    int run = 0;
    for (int w = 0; w < nwords; ++w) { CHECK(pl.prefix[(size_t)c * nwords + w] == run); run += __builtin_popcountll(pl.mask[(size_t)c * nwords + w]); }
    CHECK(run == nobs[c] && pl.cptr[c + 1] - pl.cptr[c] == nobs[c]);
    bits += run;
  }
  CHECK((int64_t)bits == N && pl.cptr[ncam] == N);
  CHECK(pl.cmpos.size() == (size_t)std::max<int64_t>(N, 1) && pl.u_cm.size() == pl.cmpos.size() && pl.v_cm.size() == pl.cmpos.size());
  std::vector<char> seen(std::max<int64_t>(N, 1), 0);
  for (int64_t q = 0; q < N; ++q) {
    const int m = pl.cmpos[q];
    CHECK(m >= pl.cptr[lay.cam[q]] && m < pl.cptr[lay.cam[q] + 1] && !seen[m]);
    seen[m] = 1;
    CHECK(pl.u_cm[m] == lay.u[q] && pl.v_cm[m] == lay.v[q]);
  }
  CHECK(pl.cm_pos.size() == std::max<size_t>(lay.sl_q.size(), 1));
  for (size_t e = 0; e < lay.sl_q.size(); ++e) CHECK(pl.cm_pos[e] == (lay.sl_q[e] >= 0 ? pl.cmpos[lay.sl_q[e]] : 0));
}

void CheckHitLists(const PointLayout& lay, const SchurPlan& pl, const std::vector<TileView>& tiles) {
  if (!pl.sparse || pl.nseg_pair == 0) { CHECK(pl.hits.empty() && pl.hit_off.empty() && pl.hit_trips.empty() && pl.hit_entries == 0); return; }
  const int P = pl.P;
  const int64_t N = lay.ptr[P];
  CHECK(pl.hits.size() == 3 * std::max<size_t>(pl.hit_entries, 1) && pl.hit_off.size() == (size_t)pl.nseg_pair * 4 && pl.hit_trips.size() == pl.hit_off.size());
  std::vector<int> csr_of(std::max<int64_t>(N, 1), 0), point_of(std::max<int64_t>(N, 1), 0);   // camera-major position -> CSR position; CSR position -> point
  for (int j = 0; j < P; ++j) for (int q = lay.ptr[j]; q < lay.ptr[j + 1]; ++q) { csr_of[pl.cmpos[q]] = q; point_of[q] = j; }
  std::vector<int> tile_of_seg(pl.nseg, 0);
  for (size_t t = 0; t < tiles.size(); ++t) for (int q = tiles[t].s0; q < tiles[t].s1; ++q) tile_of_seg[q] = (int)t;
  std::vector<uint64_t> pairs;
  size_t entries = 0;
  for (int q = 0; q < pl.nseg_pair; ++q)
    for (int wv = 0; wv < 4; ++wv) {
      CHECK(pl.hit_off[(size_t)q * 4 + wv] == entries && pl.hit_trips[(size_t)q * 4 + wv] >= 0);
      const int trips = pl.hit_trips[(size_t)q * 4 + wv];
      const SchurSeg& sgq = pl.sg[q];
      bool any_full_row = trips == 0;
      for (int l = 0; l < 64; ++l) {
        bool ended = false;
        for (int n = 0; n < trips; ++n) {
          const size_t e = entries + (size_t)n * 64 + l;
          const unsigned j = pl.hits[3 * e], ma = pl.hits[3 * e + 1], mb = pl.hits[3 * e + 2];
          if (j == RSBA_HIT_NONE) { CHECK(ma == RSBA_HIT_NONE && mb == RSBA_HIT_NONE); ended = true; continue; }
          CHECK(!ended);   // a lane's hits are dense from trip 0
          if (n == trips - 1) any_full_row = true;
          CHECK((int)j < P && (int64_t)ma < N && (int64_t)mb < N);
          const int qa = csr_of[ma], qb = csr_of[mb];
          CHECK(point_of[qa] == (int)j && point_of[qb] == (int)j && qa < qb);
          const int w = (int)j >> 6;
          CHECK(w >= sgq.word_begin && w < sgq.word_end);
          const int a = lay.cam[qa], b = lay.cam[qb], ga = a / RSBA_TG, gb = b / RSBA_TG, ia = a % RSBA_TG, ib = b % RSBA_TG;
          CHECK(ga == sgq.ga && gb == sgq.gb);
          // the lane PairSegmentSparse reads the pair on: pair (ia, ib) of an off-diagonal tile; of a diagonal tile its number among
          // the 120 pairs ia < ib, in the half of the workgroup that walks the word's parity
          int tid;
          if (ga != gb) tid = ia * RSBA_TG + ib;
          else { int dt = 0; for (int x = 0; x < ia; ++x) dt += RSBA_TG - 1 - x; dt += ib - ia - 1; tid = ((w - sgq.word_begin) & 1) * 128 + dt; }
          CHECK(tid == wv * 64 + l);
          pairs.push_back((uint64_t)qa << 32 | (uint32_t)qb);
        }
      }
      CHECK(any_full_row);   // trips is the longest lane's count, not more
      entries += (size_t)trips * 64;
    }
  CHECK(entries == pl.hit_entries);
  // every unordered pair of a point's observations exactly once: sum k (k - 1) / 2 of them, no two alike
  size_t want = 0;
  for (int j = 0; j < P; ++j) { const size_t k = lay.ptr[j + 1] - lay.ptr[j]; want += k * (k - 1) / 2; }
  CHECK(pairs.size() == want && pl.hit_count == want);
  std::sort(pairs.begin(), pairs.end());
  CHECK(std::adjacent_find(pairs.begin(), pairs.end()) == pairs.end());
}

bool SameLayout(const PointLayout& a, const PointLayout& b) {
  return a.ptr == b.ptr && a.cam == b.cam && a.u == b.u && a.v == b.v && a.order == b.order && a.pt_perm == b.pt_perm && a.max_views == b.max_views &&
         a.sl_ptr == b.sl_ptr && a.sl_q == b.sl_q && a.sl_cam == b.sl_cam && a.sl_uv == b.sl_uv;
}

// layout and plan of one problem as UploadPoints makes them, with every contract checked; returns the number of plans
int CheckProblem(const Visibility& vis, int cus, const SchurPlanSwitches& sw) {
  const int C = vis.C, P = vis.P;
  // the combinations UploadPoints can produce: the pipelined (staged) schedule with 17 .. 64 cameras, the last camera group
  // as a border with three camera groups or more up to 64 cameras, in either schedule
  const bool can_stage = C > RSBA_TG && 6 * C <= RSBA_CHOL_MAXN, can_border = C > 2 * RSBA_TG && 6 * C <= RSBA_CHOL_MAXN;
  int plans = 0;
  for (int staged = 0; staged <= (can_stage ? 1 : 0); ++staged) {
    const PointLayout sorted = rsba::SortObservations(P, vis.N(), vis.pt.data(), vis.cam.data(), vis.uv.data());
    PointLayout lay = sorted, lay1 = sorted;
    rsba::OrderAndSlice(C, P, true, staged != 0, cus, sw, &lay, 8);
    rsba::OrderAndSlice(C, P, true, staged != 0, cus, sw, &lay1, 1);
    CHECK(SameLayout(lay, lay1));   // the order does not depend on the threads that deal it
    CheckLayout(vis, lay);
    if (sw.balance == 0 || C < 2 || P < 4 * RSBA_CHUNK) CHECK(lay.pt_perm.empty());
    else if (6 * C <= RSBA_CHOL_MAXN) CHECK(!lay.pt_perm.empty());
    for (int bordered = 0; bordered <= (can_border ? 1 : 0); ++bordered) {
      const SchurPlan pl = rsba::BuildSchurPlan(C, P, lay, staged != 0, bordered != 0, cus, sw);
      CHECK(pl.C == C && pl.P == P && pl.sparse == (sw.sparse_pairs && 6 * C > RSBA_CHOL_MAXN));
      CHECK(pl.nstages == (bordered ? 2 * (pl.ngroups - 1) + 1 : pl.ngroups) && pl.grid_pp == std::max(1, std::min((P + 255) / 256, 2048)));
      const std::vector<TileView> tiles = CheckSegments(pl, staged != 0);
      if (sw.seg_per_cu != SchurPlanSwitches::kUnset && pl.nseg_pair > 0) {
        // RSBA_SEG_PER_CU is taken as it is: no rounding to whole chunks
        const int npair = pl.ntiles - pl.ngroups, nW = (P + 63) / 64;
        CHECK(pl.nseg_pair == npair * std::max(1, std::min((int)std::lround((double)sw.seg_per_cu * cus / npair), nW)));
      }
      CheckOrders(pl, tiles, staged != 0);
      CheckMasks(lay, pl);
      CheckHitLists(lay, pl, tiles);
      ++plans;
    }
  }
  return plans;
}

void CheckPlans() {
  // the switches: defaults without the environment, every one of them from it
  for (const char* n : {"RSBA_SEG_PER_CU", "RSBA_SEG_TARGET", "RSBA_SPARSE_PAIRS", "RSBA_BALANCE", "RSBA_BALANCE_PARITY", "RSBA_RED_DELAY"}) unsetenv(n);
  const SchurPlanSwitches def = SchurPlanSwitches::FromEnv();
  CHECK(def.seg_per_cu == SchurPlanSwitches::kUnset && def.seg_target == SchurPlanSwitches::kUnset && def.sparse_pairs && def.balance == 1 && def.balance_parity && def.red_delay == 250);
  setenv("RSBA_SEG_PER_CU", "4", 1); setenv("RSBA_SEG_TARGET", "6", 1); setenv("RSBA_SPARSE_PAIRS", "0", 1); setenv("RSBA_BALANCE", "0", 1);
  setenv("RSBA_BALANCE_PARITY", "0", 1); setenv("RSBA_RED_DELAY", "0", 1);
  const SchurPlanSwitches env = SchurPlanSwitches::FromEnv();
  CHECK(env.seg_per_cu == 4 && env.seg_target == 6 && !env.sparse_pairs && env.balance == 0 && !env.balance_parity && env.red_delay == 0);
  for (const char* n : {"RSBA_SEG_PER_CU", "RSBA_SEG_TARGET", "RSBA_SPARSE_PAIRS", "RSBA_BALANCE", "RSBA_BALANCE_PARITY", "RSBA_RED_DELAY"}) unsetenv(n);

  int plans = 0;
  // every camera count with small and ragged point counts (P % 64 != 0, P < 4 RSBA_CHUNK: no balancing), 256 CUs and 8
  const int cams[] = {1, 2, 8, 17, 33, 40, 64, 70, 130};
  const int points[] = {3, 64, 100, 1000, 4 * RSBA_CHUNK - 1, 4 * RSBA_CHUNK, 5003};
  for (int C : cams)
    for (int P : points) {
      const Visibility vis = MakeVisibility(C, P, C <= 8, 1000003ull * C + P);
      for (int cus : {256, 8}) plans += CheckProblem(vis, cus, def);
    }
  // eight streams of the point dealing (P >= 16384), up to 60000 points
  const std::pair<int, int> large[] = {{8, 60000}, {17, 16384}, {40, 20011}, {64, 16421}, {64, 60000}, {70, 16421}, {130, 30000}};
  for (const auto& cp : large) {
    const Visibility vis = MakeVisibility(cp.first, cp.second, cp.first <= 8, 77ull * cp.first + cp.second);
    plans += CheckProblem(vis, 256, def);
    if (cp.second < 60000) plans += CheckProblem(vis, 8, def);
  }
  // every switch away from its default
  std::vector<SchurPlanSwitches> variants;
  for (int spc : {1, 4, 8}) { SchurPlanSwitches s; s.seg_per_cu = spc; variants.push_back(s); }
  { SchurPlanSwitches s; s.seg_target = 6; variants.push_back(s); }
  { SchurPlanSwitches s; s.seg_per_cu = 4; s.seg_target = 6; variants.push_back(s); }   // RSBA_SEG_PER_CU wins
  { SchurPlanSwitches s; s.sparse_pairs = false; variants.push_back(s); }
  { SchurPlanSwitches s; s.balance = 0; variants.push_back(s); }
  { SchurPlanSwitches s; s.balance = 5; variants.push_back(s); }
  { SchurPlanSwitches s; s.balance_parity = false; variants.push_back(s); }
  { SchurPlanSwitches s; s.red_delay = 0; variants.push_back(s); }
  { SchurPlanSwitches s; s.red_delay = 7; variants.push_back(s); }
  const std::pair<int, int> switched[] = {{40, 5003}, {64, 16421}, {70, 5003}, {130, 16421}};
  for (const auto& cp : switched) {
    const Visibility vis = MakeVisibility(cp.first, cp.second, false, 31ull * cp.first + cp.second);
    for (const SchurPlanSwitches& s : variants) plans += CheckProblem(vis, 256, s);
  }
  printf("schur plans checked: %d\n", plans);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "--plans") == 0) {
    CheckPlans();
    printf("host sanitize driver: ok\n");
    return 0;
  }
  CHECK(argc == 3);
  const std::string G = argv[1], T = argv[2];
  CHECK(rsba_version() == RSBA_VERSION && rsba_device_count() == 0);
  for (int c = -1; c < 10; ++c) CHECK(rsba_error_string(c) != nullptr);

  // ---- intrinsics XML (my_io.cpp:5-31) + correspondence.txt (bundle_adjustment.cpp:132-187)
  const char* serials[4] = {"821312061029", "816612062327", "821212062536", "821212061326"};
  double intr[16];
  for (int i = 0; i < 4; ++i) CHECK(rsba_read_intrinsics_xml((G + "/intrinsics/" + serials[i] + ".xml").c_str(), intr + 4 * i) == RSBA_OK);
  CHECK(rsba_read_intrinsics_xml((G + "/intrinsics/none.xml").c_str(), intr) == RSBA_ERR_IO);
  rsba_problem* p = nullptr;
  CHECK(rsba_problem_load_correspondence((G + "/hongo/correspondence.txt").c_str(), RSBA_MODEL_MARKER_CHAIN, 0.0148, intr, &p) == RSBA_OK);
  CHECK(rsba_problem_num_times(p) == 6 && rsba_problem_num_cameras(p) == 4 && rsba_problem_num_markers(p) == 11);
  CHECK(rsba_problem_num_observations(p) == 68 && rsba_problem_num_parameters(p) == 126 && rsba_problem_num_points(p) == 0);
  for (int64_t i = -1; i <= 68; ++i) {   // one past either end: accessors must refuse, not read
    (void)rsba_problem_camera_idx(p, i); (void)rsba_problem_time_idx(p, i); (void)rsba_problem_marker_idx(p, i); (void)rsba_problem_point_idx(p, i);
  }
  for (int t = -1; t <= 6; ++t) for (int c = -1; c <= 4; ++c) (void)rsba_problem_num_observations_per_time_camera(p, t, c);
  CHECK(rsba_problem_camera_parameters(p, 4) == nullptr && rsba_problem_camera_parameters(p, 3) != nullptr);
  CHECK(rsba_problem_marker_transform(p, 11) == nullptr && rsba_problem_marker_transform(p, -1) == nullptr);
  std::vector<double> corners(12 * 68);
  CHECK(rsba_problem_point3d_coordinates(p, corners.data()) == RSBA_OK);
  // writers (bundle_adjustment_manager.cpp:98-175)
  CHECK(rsba_write_outputs(p, (T + "/Camera_Transform.xml").c_str(), T.c_str(), (T + "/point3d.txt").c_str()) == RSBA_OK);
  CHECK(rsba_write_outputs(p, nullptr, nullptr, nullptr) == RSBA_OK);
  CHECK(rsba_write_outputs(p, (T + "/no/such/dir/x.xml").c_str(), nullptr, nullptr) == RSBA_ERR_IO);
  // Correspondencer::CalculateTransforms on the loaded problem (EPnP per camera)
  CHECK(rsba_problem_initial_camera_poses(p) == RSBA_OK);
  rsba_problem_free(p);
  p = nullptr;
  CHECK(rsba_problem_load_correspondence((G + "/test2/correspondence_test.txt").c_str(), RSBA_MODEL_MARKER_CHAIN_TEST2, 0.048, intr, &p) == RSBA_OK);
  CHECK(rsba_write_outputs(p, (T + "/Camera_Transform2.xml").c_str(), nullptr, (T + "/point3d2.txt").c_str()) == RSBA_OK);
  rsba_problem_free(p);
  p = nullptr;

  // ---- malformed / short inputs: return codes, no reads past the end
  CHECK(rsba_problem_load_correspondence((G + "/hongo/nope.txt").c_str(), RSBA_MODEL_MARKER_CHAIN, 0.0148, intr, &p) == RSBA_ERR_IO);
  WriteFile(T + "/short.txt", "2 2 1 3\n0 1 1\n1 1 0\n0 0 0 1 2 3 4 5 6 7 8\n0 1 0 1 2 3");
  CHECK(rsba_problem_load_correspondence((T + "/short.txt").c_str(), RSBA_MODEL_MARKER_CHAIN, 0.0148, intr, &p) == RSBA_ERR_FORMAT);
  WriteFile(T + "/badidx.txt", "1 1 1 1\n0 1\n0 7 0 1 2 3 4 5 6 7 8\n0 0 0 0 0 0\n0 0 0 0 0 0\n0 0 0 0 0 0\n");
  CHECK(rsba_problem_load_correspondence((T + "/badidx.txt").c_str(), RSBA_MODEL_MARKER_CHAIN, 0.0148, intr, &p) != RSBA_OK);
  WriteFile(T + "/neg.txt", "-1 4 2 5\n");
  CHECK(rsba_problem_load_correspondence((T + "/neg.txt").c_str(), RSBA_MODEL_MARKER_CHAIN, 0.0148, intr, &p) != RSBA_OK);
  WriteFile(T + "/empty.txt", "");
  CHECK(rsba_problem_load_correspondence((T + "/empty.txt").c_str(), RSBA_MODEL_MARKER_CHAIN, 0.0148, intr, &p) == RSBA_ERR_FORMAT);
  CHECK(rsba_problem_load_points_file((T + "/empty.txt").c_str(), intr, &p) == RSBA_ERR_FORMAT);

  // ---- Test1 point file (bundle_adjustmenter.cpp:55-85), both header forms
  CHECK(rsba_problem_load_points_file((G + "/two_cam_data.txt").c_str(), intr, &p) == RSBA_OK);
  CHECK(rsba_problem_model(p) == RSBA_MODEL_POINTS && rsba_problem_num_cameras(p) == 1);   // the committed file holds one camera
  const int64_t n1 = rsba_problem_num_observations(p);
  CHECK(n1 == rsba_problem_num_points(p));
  for (int64_t i = -1; i <= n1; ++i) { (void)rsba_problem_point_idx(p, i); (void)rsba_problem_camera_idx(p, i); }
  CHECK(rsba_problem_set_camera_constant(p, 0, 1) == RSBA_OK && rsba_problem_set_camera_constant(p, 1, 1) == RSBA_ERR_ARG);
  rsba_problem_free(p);
  p = nullptr;
  WriteFile(T + "/pts3.txt", "2 2 3\n0 0 1.5 2.5\n1 0 3.5 4.5\n1 1 5.5 6.5\n0 0 0\n0 0 1\n0 0 0\n0 0 2\n0.1 0.2 3\n0.3 0.1 4\n");
  CHECK(rsba_problem_load_points_file((T + "/pts3.txt").c_str(), intr, &p) == RSBA_OK);
  CHECK(rsba_problem_num_observations(p) == 3 && rsba_problem_num_points(p) == 2);
  rsba_problem_free(p);
  p = nullptr;
  WriteFile(T + "/pts_bad.txt", "2 2 3\n0 0 1.5 2.5\n1 5 3.5 4.5\n1 1 5.5 6.5\n0 0 0\n0 0 1\n0 0 0\n0 0 2\n0.1 0.2 3\n0.3 0.1 4\n");
  CHECK(rsba_problem_load_points_file((T + "/pts_bad.txt").c_str(), intr, &p) != RSBA_OK);

  // ---- problem from arrays: index validation
  {
    const int32_t cam[3] = {0, 1, 1}, pt[3] = {0, 0, 1};
    const double obs[6] = {1, 2, 3, 4, 5, 6}, par[18] = {0}, k[8] = {600, 600, 320, 240, 600, 600, 320, 240};
    CHECK(rsba_problem_create_points(2, 2, 3, cam, pt, obs, par, k, &p) == RSBA_OK);
    rsba_problem_free(p);
    p = nullptr;
    const int32_t bad[3] = {0, 2, 1};
    CHECK(rsba_problem_create_points(2, 2, 3, bad, pt, obs, par, k, &p) != RSBA_OK);
    CHECK(rsba_problem_create_points(2, 2, 3, nullptr, pt, obs, par, k, &p) == RSBA_ERR_ARG);
    CHECK(rsba_problem_create_points(0, 0, 0, cam, pt, obs, par, k, &p) != RSBA_ERR_HIP);
    if (p) { rsba_problem_free(p); p = nullptr; }
  }

  // ---- the front end's pose algebra and EPnP (correspondencer.cpp:5-39, 119-147, 192-195)
  {
    const double a[6] = {0.1, -0.2, 0.3, 0.05, 0.02, 0.6}, b[6] = {-0.3, 0.1, 0.2, 0.01, -0.04, 0.1};
    double c[6], d[6], corners4[12];
    CHECK(rsba_base_pose_from_marker_detection(a, b, c) == RSBA_OK && rsba_marker_pose_in_camera(c, b, d) == RSBA_OK);
    for (int i = 0; i < 6; ++i) CHECK(std::fabs(d[i] - a[i]) < 1e-12);
    CHECK(rsba_marker_corners_in_camera(a, 0.0148, corners4) == RSBA_OK);
    CHECK(rsba_base_pose_from_marker_detection(nullptr, b, c) == RSBA_ERR_ARG);
    // EPnP on eight exact projections of a non-planar set
    const double K[4] = {630, 625, 318, 237};
    double obj[24], img[16], pose[6];
    const double truth[6] = {0.2, -0.1, 0.15, 0.03, -0.02, 1.2};
    for (int i = 0; i < 8; ++i) { obj[3 * i] = (i & 1) ? 0.1 : -0.1; obj[3 * i + 1] = (i & 2) ? 0.12 : -0.08; obj[3 * i + 2] = (i & 4) ? 0.09 : -0.11; }
    {
      // Rodrigues by hand
      const double th = std::sqrt(truth[0] * truth[0] + truth[1] * truth[1] + truth[2] * truth[2]);
      const double kx = truth[0] / th, ky = truth[1] / th, kz = truth[2] / th, cs = std::cos(th), sn = std::sin(th), c1 = 1 - cs;
      const double R[9] = {cs + c1 * kx * kx, c1 * kx * ky - sn * kz, c1 * kx * kz + sn * ky, c1 * kx * ky + sn * kz, cs + c1 * ky * ky, c1 * ky * kz - sn * kx,
                           c1 * kx * kz - sn * ky, c1 * ky * kz + sn * kx, cs + c1 * kz * kz};
      for (int i = 0; i < 8; ++i) {
        const double* X = obj + 3 * i;
        const double x = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + truth[3], y = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + truth[4], z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + truth[5];
        img[2 * i] = K[0] * x / z + K[2]; img[2 * i + 1] = K[1] * y / z + K[3];
      }
    }
    CHECK(rsba_solve_pnp_epnp(8, obj, img, K, pose) == RSBA_OK);
    for (int i = 0; i < 6; ++i) CHECK(std::fabs(pose[i] - truth[i]) < 1e-6);
    CHECK(rsba_solve_pnp_epnp(3, obj, img, K, pose) != RSBA_OK);
    for (int i = 0; i < 8; ++i) obj[3 * i + 2] = 0.0;   // coplanar: refused
    CHECK(rsba_solve_pnp_epnp(8, obj, img, K, pose) == RSBA_ERR_UNSUPPORTED);
  }
  rsba_options o;
  rsba_options_default(&o);
  CHECK(o.max_num_iterations == 50);
  CheckPlans();
  printf("host sanitize driver: ok\n");
  return 0;
}
