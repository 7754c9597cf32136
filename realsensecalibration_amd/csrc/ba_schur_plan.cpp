// Host-side planning of the point model's set-up (ba_schur_plan.hpp): every sum of the solve is added in the order laid
// down here, and the in-kernel waits of ba_schur_tiled.hpp rely on what it guarantees — tests/host_sanitize_driver.cpp
// checks those contracts on the CPU.
#include "ba_schur_plan.hpp"

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <utility>

namespace rsba {

SchurPlanSwitches SchurPlanSwitches::FromEnv() {
  SchurPlanSwitches sw;
  auto number = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
  sw.seg_per_cu = number("RSBA_SEG_PER_CU", kUnset);
  sw.seg_target = number("RSBA_SEG_TARGET", kUnset);
  sw.sparse_pairs = number("RSBA_SPARSE_PAIRS", 1) != 0;
  sw.balance = number("RSBA_BALANCE", 1);
  sw.balance_parity = number("RSBA_BALANCE_PARITY", 1) != 0;
  sw.red_delay = number("RSBA_RED_DELAY", 250);
  return sw;
}

namespace {

// ------------------------------------------------------------------------------------------------
// Segments of a tile.
// ------------------------------------------------------------------------------------------------
// nW words cut into about ns segments of WHOLE chunks — runs of k chunks, k what the target length is nearest to: how many
// segments that gives (0 without words), and k.
int WholeChunkSegments(int nW, int ns, int* run = nullptr) {
  const int k = std::max(1, (int)std::lround((double)nW / ns / RSBA_CW));
  if (run) *run = k;
  return (nW + RSBA_CW * k - 1) / (RSBA_CW * k);
}

// Word bounds of the segments one tile's points are cut into (ns + 1 values, in 64-point mask words).  The pair tiles'
// are the same for every pair tile: shared by the plan and by the point ordering below (whose units are these segments' chunks).
std::vector<int> SegmentBounds(int nW, int ns, double taper = 1.0) {
  // Tapered segments (taper > 1: the first of a tile is that many times as long as the last).  A launch is over when its last
  // block is, so long blocks first, short ones last.  At 64 cameras, pipelined, it measured nothing (a stage is only ~1-2
  // "rounds" of slots deep and two blocks share a CU's VALU, so a block's duration follows its CU-mate more than its own
  // length): 1.  Above 64 cameras (sparse pair segments, handed out by point range: the last ranges are the short ones)
  // the launch is 2.6 rounds of ~110 us blocks deep and its tail was 100 us long: 4 (419 -> 385 us at the config-5 shard).
  std::vector<int> bound(ns + 1, 0);
  if (taper == 1.0 && ns >= 1) {
    // as many segments as whole runs of k chunks give (PairSegmentsPerTile's and the self segments' rounding): cut exactly there — an even
    // split of the words (1563 words into 196: 7.97 each) drifts off the chunk boundaries, and a segment that straddles one stages two chunks
    int k;
    if (WholeChunkSegments(nW, ns, &k) == ns) {
      for (int i = 0; i <= ns; ++i) bound[i] = std::min(nW, i * RSBA_CW * k);
      return bound;
    }
  }
  const double hi = 2.0 * taper / (taper + 1.0), lo = 2.0 - hi;
  double cum = 0.0;
  for (int i = 0; i < ns; ++i) { cum += ns > 1 ? hi - (hi - lo) * i / (ns - 1) : 1.0; bound[i + 1] = (int)std::llround(nW * cum / ns); }
  bound[ns] = nW;
  bool ok = true;
  for (int i = 0; i < ns; ++i) ok = ok && bound[i + 1] > bound[i];
  if (!ok) for (int i = 0; i <= ns; ++i) bound[i] = (int)((int64_t)nW * i / ns);
  return bound;
}

// The taper of a pair tile's segments and whether its pair segments walk the sparse hit lists — one place for both
// the plan and the point ordering, whose balancing units must be the units the kernel really synchronises on.
// (above 64 cameras in EITHER schedule: the pipelined one there — round 4, the tiled factorisation beside the Schur kernel — runs the
//  same sparse, tapered pair segments in stage order)
double PairSegmentTaper(int C) { return 6 * C > RSBA_CHOL_MAXN ? 4.0 : 1.0; }
bool SparsePairSegments(int C, const SchurPlanSwitches& sw) { return sw.sparse_pairs && 6 * C > RSBA_CHOL_MAXN; }

// a 1-camera group has no off-diagonal pair
bool HasPairTile(int C, int ga, int gb) { return !(ga == gb && std::min(RSBA_TG, C - RSBA_TG * ga) < 2); }

int PairSegmentsPerTile(int C, int P, bool staged, int cus, const SchurPlanSwitches& sw) {
  const int ngroups = (C + RSBA_TG - 1) / RSBA_TG;
  int npair_tiles = 0;
  for (int ga = 0; ga < ngroups; ++ga) for (int gb = ga; gb < ngroups; ++gb) if (HasPairTile(C, ga, gb)) ++npair_tiles;
  // measured at 64 cameras: the pipelined schedule likes shorter workgroups (a stage ends with its last one), the
  // sequential one fewer partial sums
  // (RSBA_SEG_TARGET: the same number through the whole-chunk rounding below, which RSBA_SEG_PER_CU bypasses)
  const bool exact = sw.seg_per_cu != SchurPlanSwitches::kUnset;
  const int seg_per_cu = exact ? sw.seg_per_cu : sw.seg_target != SchurPlanSwitches::kUnset ? sw.seg_target : (6 * C > RSBA_CHOL_MAXN ? 6 : (staged ? 8 : 4));
  const int target = seg_per_cu * cus;
  const int nW = (P + 63) / 64;
  int ns = std::max(1, std::min((int)std::lround((double)target / std::max(1, npair_tiles)), nW));
  // Up to 64 cameras a segment is walked in chunks of RSBA_CW words, and a ragged last chunk (9.5 words per segment = a full
  // chunk and 98 points) is a staging round trip and a barrier for a handful of hits per lane: segments of WHOLE chunks —
  // as many chunks as the target length is nearest to.  64 cameras x 125k points (a rank's shard of config 4): 245 segments of one
  // chunk instead of 205 of 9.5 words, 0.437 against 0.471 ms per iteration (round 4); 100k points: 7.6 words, unchanged.
  // (round 6: also when the target length is only NEAR a chunk — three quarters of one or more: at 100k points the target was 7.6 words,
  //  205 ragged segments a tile, each staging a chunk's buffers for 488 points; 196 of exactly one chunk: 0.3398 - 0.3409 ms per step
  //  against 0.3431 - 0.3445, two alternating runs each, RSBA_SEG_TARGET=6 against the default on one box)
  if (!exact && !SparsePairSegments(C, sw) && 4 * (long)nW > 3L * RSBA_CW * ns) ns = std::max(1, WholeChunkSegments(nW, ns));
  return ns;
}

// (more than 64 cameras: at most 16 self segments per tile — two reduction groups, no reducer workgroups)
int SelfSegmentsPerTile(int C, int P, int ngroups, int cus, const SchurPlanSwitches& sw) {
  const int nW = (P + 63) / 64;  // mask words that hold points
  int ns_self = std::max(1, std::min((2 * cus + ngroups - 1) / ngroups, nW));   // (two self segments per CU over all tiles: the target before the rounding below)
  // (round 6: the self segments too in WHOLE chunks where their target length is three quarters of a chunk or more — they walk the chunk
  //  buffers like the pair segments do.  100k points: 98 segments of two chunks a tile instead of 128 of 12.2 words, 0.3357 - 0.3383 ms per
  //  step against 0.3423; 66 of three 0.3377 - 0.3395, 196 of one 0.3475 - 0.3493 — two alternating runs each on one box)
  if (!SparsePairSegments(C, sw) && 4 * (long)nW > 3L * RSBA_CW * ns_self) ns_self = std::max(1, WholeChunkSegments(nW, ns_self));
  return 6 * C > RSBA_CHOL_MAXN ? std::min(ns_self, 16) : ns_self;
}

// Host threads for the point dealing: the caller's cap, or as many as this process may run on — its affinity mask, not the
// machine's core count
int HostThreads(int cap) {
  if (cap > 0) return cap;
  cpu_set_t aff;
  return sched_getaffinity(0, sizeof(aff), &aff) == 0 ? CPU_COUNT(&aff) : 1;
}

// ------------------------------------------------------------------------------------------------
// Point order for the tiled Schur kernel.
//
// A lane of a pair tile walks the points its two cameras share, chunk by chunk (RSBA_CHUNK points of one segment), and
// a wavefront runs as many trips per chunk as its busiest lane: with the points in file order the hit counts of the
// 64 pairs of a wave are Binomial(~490, (k/C)^2) — at 64 cameras x 20 views the busiest lane has 38 % more hits than the
// mean, i.e. 26 % of the lane-trips of the dominant kernel are masked off.  Which point sits in which chunk is free (points are
// independent given the cameras), so the points are dealt to the chunks such that every camera PAIR gets about the same
// number of shared points in every chunk: greedily, each point (in a fixed pseudo-random order) goes to the best of a
// few candidate chunks, "best" = fewest points so far that share a pair with it, relative to the chunk's fill.
// Measured on the 64 x 100k x 20 problem: lane utilisation of the pair tiles 74 % -> 86 % for ~0.5 s of single-threaded
// set-up; the dealing runs as 8 independent streams on up to 8 host threads.
// The permutation is internal: parameters are uploaded / downloaded through it, nothing the caller sees changes order.
// Deterministic (fixed seed): two solvers of the same problem add in the same order.
// Returns perm (position -> original point); empty = keep the file order.
// ------------------------------------------------------------------------------------------------
std::vector<int> BalancedPointOrder(int C, int P, bool staged, int cus, const SchurPlanSwitches& sw, const std::vector<int>& ptr, const std::vector<int>& cam,
                                    int max_threads) {
  const int mode = sw.balance;
  if (mode == 0 || C < 2 || P < 4 * RSBA_CHUNK) return {};
  const int nW = (P + 63) / 64;
  const std::vector<int> bound = SegmentBounds(nW, PairSegmentsPerTile(C, P, staged, cus, sw), PairSegmentTaper(C));
  // units: what the lanes of a pair tile's wavefront synchronise on — the 512-point chunks of the masked search, or, with the
  // sparse hit lists (more than 64 cameras), the WHOLE pair segment: its lists run as many trips as the longest of a
  // wavefront's 64, over all of the segment's points.  (Until round 4 the units were cut with taper 1 whatever the plan used,
  // and into chunks whatever the pair segments walked: above 64 cameras the balance was computed against the wrong partition.)
  const bool whole_segments = SparsePairSegments(C, sw);
  std::vector<int> ubeg, ucap;
  for (size_t i = 0; i + 1 < bound.size(); ++i) {
    const int step = whole_segments ? std::max(1, bound[i + 1] - bound[i]) : RSBA_CW;
    for (int w = bound[i]; w < bound[i + 1]; w += step) {
      const int we = std::min(w + step, bound[i + 1]);
      ubeg.push_back(64 * w);
      ucap.push_back(std::min(64 * we, P) - 64 * w);
    }
  }
  const int nu = (int)ubeg.size();
  // (the pair counters, 2 bytes per unit and camera pair: at most 64 MB of host memory — beyond that the file order is kept)
  if (nu < 2 || (double)nu * C * C > 3.2e7) return {};
  const int64_t N = ptr[P];
  const double pairs_per_point = N > 0 ? 0.5 * ((double)N / P) * ((double)N / P) : 1.0;
  // candidates per point: bounded work (~6e8 counter reads), at least 2, at most 32 (or RSBA_BALANCE = number)
  int D = mode > 1 ? mode : (int)std::max(2.0, std::min(32.0, 6e8 / (std::max(1.0, pairs_per_point) * P)));
  D = std::min(D, nu);
  std::vector<uint16_t> cnt((size_t)nu * C * C, 0);   // [unit][a][b], a < b
  std::vector<int> fill(nu, 0), unit_of(P, 0);
  // fixed pseudo-random visiting order (splitmix64)
  auto mix = [](uint64_t& st) { uint64_t z = (st += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); };
  std::vector<int> visit(P);
  {
    uint64_t st = 0x9E3779B97F4A7C15ull;
    for (int j = 0; j < P; ++j) visit[j] = j;
    for (int j = P - 1; j > 0; --j) std::swap(visit[j], visit[(size_t)(mix(st) % (uint64_t)(j + 1))]);
  }
  // Independent streams: the units are cut into kStreams contiguous ranges, the visiting order into runs of matching
  // capacity, and every stream deals its run to its own units.  The number of streams is a constant (not the number of
  // threads that happen to run them): the order, and with it every sum of the solve, is the same on every machine.
  constexpr int kStreams = 8;
  const int nstream = nu >= 4 * kStreams ? kStreams : 1;
  std::vector<int> su(nstream + 1, 0), sp(nstream + 1, 0);
  for (int t = 0; t < nstream; ++t) {
    su[t + 1] = (int)((int64_t)nu * (t + 1) / nstream);
    int capsum = 0;
    for (int g = su[t]; g < su[t + 1]; ++g) capsum += ucap[g];
    sp[t + 1] = sp[t] + capsum;
  }
  if (sp[nstream] != P) return {};   // cannot happen: the capacities add up to P
  std::atomic<int> failed{0};
  auto run_stream = [&](int t) {
    const int g0 = su[t], ng = su[t + 1] - su[t];
    const int Dt = std::min(D, ng);
    uint64_t st = 0xD1B54A32D192ED03ull * (uint64_t)(t + 1);
    int open_from = g0;   // all units of the stream below are full
    for (int q = sp[t]; q < sp[t + 1]; ++q) {
      const int j = visit[q];
      const int b = ptr[j], k = ptr[j + 1] - b;
      const int* cj = cam.data() + b;
      int best = -1; double best_s = 0.0;
      auto score = [&](int g) {
        const uint16_t* c = &cnt[(size_t)g * C * C];
        long sum = 0;
        for (int x = 0; x < k; ++x) { const uint16_t* row = c + (size_t)cj[x] * C; for (int y = x + 1; y < k; ++y) sum += row[cj[y]]; }
        const double sc = (double)sum / (double)(fill[g] + 1);
        if (best < 0 || sc < best_s) { best = g; best_s = sc; }
      };
      if (ng <= D) {
        // few enough units in the stream: all of them that still have room (first minimum wins)
        for (int g = g0; g < g0 + ng; ++g) if (fill[g] < ucap[g]) score(g);
      } else {
        for (int d = 0, tries = 0; d < Dt || best < 0; ++tries) {
          int g;
          if (tries < 4 * Dt) { g = g0 + (int)(mix(st) % (uint64_t)ng); if (fill[g] >= ucap[g]) continue; }
          else { while (open_from < g0 + ng && fill[open_from] >= ucap[open_from]) ++open_from; g = open_from; if (g >= g0 + ng) break; }
          ++d;
          score(g);
          if (tries >= 4 * Dt) break;
        }
      }
      if (best < 0) { failed = 1; return; }
      uint16_t* c = &cnt[(size_t)best * C * C];
      for (int x = 0; x < k; ++x) { uint16_t* row = c + (size_t)cj[x] * C; for (int y = x + 1; y < k; ++y) if (row[cj[y]] != 0xFFFF) ++row[cj[y]]; }
      unit_of[j] = best; ++fill[best];
    }
  };
  {
    // (the streams, and with them the order, do not depend on the number of threads)
    const int nthreads = std::max(1, std::min<int>(nstream, HostThreads(max_threads)));
    std::atomic<int> next_stream{0};
    auto worker = [&]() { for (int t = next_stream++; t < nstream; t = next_stream++) run_stream(t); };
    std::vector<std::thread> pool;
    for (int i = 1; i < nthreads; ++i) pool.emplace_back(worker);
    worker();
    for (auto& th : pool) th.join();
  }
  if (failed) return {};
  // positions: the points of a unit in ascending original order
  std::vector<int> next(ubeg), perm(P, -1);
  for (int j = 0; j < P; ++j) perm[next[unit_of[j]]++] = j;
  for (int q = 0; q < P; ++q) if (perm[q] < 0) return {};
  // Inside every unit (round 5): which 64-point WORD a point sits in decides which half of a DIAGONAL tile's workgroup finds its
  // hits — the tile's 120 pairs sit in both halves, one walks the even words of a chunk, the other the odd ones (PairSegment,
  // PairSegmentSparse) — and the dealing above balances whole units only.  So the unit's points are dealt to its even / odd words
  // such that every pair of cameras of ONE group gets about the same number of shared points in either half (greedy, in the
  // unit's order: the half where the point's diagonal pairs have fewer hits so far, relative to the half's fill).  Measured offline
  // on the 64 x 100k x 20 problem (the kernel's lane -> pair map replayed on the host): lane utilisation of the diagonal tiles'
  // hit loops 69.8 % -> 75.3 %, of all pair tiles 81.9 % -> 83.6 %.
  // The pass walks every point's camera pairs twice, O(P k^2) on one thread: bounded like the dealing above (~6e8 pair visits:
  // 64 views x 1M points would add seconds of set-up, which count against max_solver_time_in_seconds) — beyond that the words stay as
  // dealt, which costs speed only.
  if (sw.balance_parity && 2.0 * pairs_per_point * P <= 6e8) {
    std::vector<uint16_t> hc((size_t)C * C * 2);
    std::vector<int> half[2];
    for (int g = 0; g < nu; ++g) {
      const int p0 = ubeg[g], np = ucap[g], nwu = (np + 63) / 64;
      if (nwu < 2) continue;
      int cap[2] = {0, 0};
      for (int w = 0; w < nwu; ++w) cap[w & 1] += std::min(64, np - 64 * w);
      std::fill(hc.begin(), hc.end(), (uint16_t)0);
      half[0].clear(); half[1].clear();
      for (int q = p0; q < p0 + np; ++q) {
        const int j = perm[q], b = ptr[j], k = ptr[j + 1] - b;
        const int* cj = cam.data() + b;
        long sc[2] = {0, 0};
        for (int x = 0; x < k; ++x) for (int y = x + 1; y < k; ++y) if (cj[x] / RSBA_TG == cj[y] / RSBA_TG) { const uint16_t* c = &hc[((size_t)cj[x] * C + cj[y]) * 2]; sc[0] += c[0]; sc[1] += c[1]; }
        int h;
        if ((int)half[0].size() >= cap[0]) h = 1;
        else if ((int)half[1].size() >= cap[1]) h = 0;
        else h = sc[0] * (long)(half[1].size() + 1) <= sc[1] * (long)(half[0].size() + 1) ? 0 : 1;
        half[h].push_back(j);
        for (int x = 0; x < k; ++x) for (int y = x + 1; y < k; ++y) if (cj[x] / RSBA_TG == cj[y] / RSBA_TG) { uint16_t& c = hc[((size_t)cj[x] * C + cj[y]) * 2 + h]; if (c != 0xFFFF) ++c; }
      }
      size_t i0 = 0, i1 = 0;
      for (int w = 0; w < nwu; ++w) { const int n = std::min(64, np - 64 * w); for (int l = 0; l < n; ++l) perm[p0 + 64 * w + l] = (w & 1) ? half[1][i1++] : half[0][i0++]; }
    }
  }
  return perm;
}

// ------------------------------------------------------------------------------------------------
// Static structure of the tiled Schur kernel: visibility bitsets, tiles, segments, launch orders, hit lists.
// ------------------------------------------------------------------------------------------------
// What the steps of BuildSchurPlan hand each other about the tiles
struct TileTable {
  std::vector<int> tab;                        // [ntiles][3]: ga, gb, self — pair tiles (ga <= gb) first, then one self tile per group
  std::vector<int> tsp;                        // [ntiles + 1] first compute segment of a tile
  std::vector<int> stage_of_tile;              // [ntiles]
  std::vector<int> stage_order;                // the order the stages are worked through
  std::vector<std::vector<int>> red_of_tile;   // [ntiles] the tile's reducer entries
  bool self(int t) const { return tab[3 * t + 2] != 0; }
};

void PlanMasks(const PointLayout& lay, SchurPlan* plan) {
  const int P = plan->P, nwords = plan->nwords, ncam = plan->ngroups * RSBA_TG;
  const std::vector<int>& pt_ptr = lay.ptr;
  const std::vector<int>& obs_cam = lay.cam;
  const int64_t N = pt_ptr[P];
  std::vector<unsigned long long>& mask = plan->mask;
  std::vector<int>&cptr = plan->cptr, &prefix = plan->prefix, &cmpos = plan->cmpos;
  mask.assign((size_t)ncam * nwords, 0ull);
  cptr.assign(ncam + 1, 0);
  for (int j = 0; j < P; ++j)
    for (int q = pt_ptr[j]; q < pt_ptr[j + 1]; ++q) { mask[(size_t)obs_cam[q] * nwords + (j >> 6)] |= 1ull << (j & 63); cptr[obs_cam[q] + 1]++; }
  for (int c = 0; c < ncam; ++c) cptr[c + 1] += cptr[c];
  prefix.assign((size_t)ncam * nwords, 0);
  cmpos.assign(std::max<int64_t>(N, 1), 0);
  for (int c = 0; c < ncam; ++c) { int run = 0; for (int w = 0; w < nwords; ++w) { prefix[(size_t)c * nwords + w] = run; run += __builtin_popcountll(mask[(size_t)c * nwords + w]); } }
  {
    // camera-major position of every (sorted) observation; a camera seeing the same point twice keeps file order
    std::vector<int> fill(cptr.begin(), cptr.end() - 1);
    for (int j = 0; j < P; ++j) for (int q = pt_ptr[j]; q < pt_ptr[j + 1]; ++q) cmpos[q] = fill[obs_cam[q]]++;
  }
  plan->u_cm.assign(cmpos.size(), 0.0);
  plan->v_cm.assign(cmpos.size(), 0.0);
  for (int64_t q = 0; q < N; ++q) { plan->u_cm[cmpos[q]] = lay.u[q]; plan->v_cm[cmpos[q]] = lay.v[q]; }
  plan->cm_pos.assign(std::max<size_t>(lay.sl_q.size(), 1), 0);
  for (size_t e = 0; e < lay.sl_q.size(); ++e) plan->cm_pos[e] = lay.sl_q[e] >= 0 ? cmpos[lay.sl_q[e]] : 0;
}

// Reduction tree of a tile of ns_t segments: the sizes of its groups, in order.  Groups of GRP consecutive segments, but the
// last segments in groups of 2, 2, 1, 1, 1, 1: a tile is over when its last group has been added, and that group is usually one of
// the last in order.
std::vector<int> GroupSizes(int ns_t, int GRP) {
  std::vector<int> gsize;
  int left = ns_t;
  // (a group of one segment goes straight into the group sum, SegmentOut in ba_schur_tiled.hpp; four of them and two pairs
  //  at the end: 0.4057 ms against 0.4087 with 1, 1, 2, 4 and 0.409 with eight or more single segments)
  const std::vector<int> tail = {1, 1, 1, 1, 2, 2};
  std::vector<int> last;
  if (ns_t >= 4 * GRP) for (size_t k = 0; k < tail.size() && left > tail[k]; ++k) { last.push_back(tail[k]); left -= tail[k]; }
  while (left > 0) { const int g = std::min(GRP, left); gsize.push_back(g); left -= g; }
  for (int k = (int)last.size() - 1; k >= 0; --k) gsize.push_back(last[k]);
  return gsize;
}

// Tiles, their compute segments and reduction groups, the reducer entries behind them, and the arrivals at the stages' counters.
void PlanSegments(bool staged, bool bordered, int cus, const SchurPlanSwitches& sw, SchurPlan* plan, TileTable* tt) {
  const int C = plan->C, P = plan->P, ngroups = plan->ngroups;
  // Stage of a tile.  Plain: the camera group of its columns — self tile g and the pair tiles (g, g' >= g): what the left-looking
  // factorisation needs for group g's panels.  With the last group Bg as a BORDER (ba_cholesky_border.hpp): the leading system's
  // tiles first — stage g < Bg: self tile g, pair tiles (g, g') with g' < Bg —, then the border's rows, tile (g, Bg) = stage
  // Bg + g, and last the border's own self and pair tile, stage 2 Bg.
  const int Bg = bordered ? ngroups - 1 : -1;
  auto stage_of = [&](int ga, int gb, bool self) { return !bordered ? ga : (ga == Bg ? 2 * Bg : (!self && gb == Bg ? Bg + ga : ga)); };
  // tiles: pair tiles (ga <= gb) and one self tile per group.  A workgroup's time per chunk is set by its
  // busiest lane, which is the same for diagonal and off-diagonal pair tiles (~10% of the points) and ~1/5 of
  // that for self tiles (31% of the points dealt to 16 lanes).
  std::vector<int>& tab = tt->tab;
  for (int ga = 0; ga < ngroups; ++ga) for (int gb = ga; gb < ngroups; ++gb) if (HasPairTile(C, ga, gb)) { tab.push_back(ga); tab.push_back(gb); tab.push_back(0); }
  for (int ga = 0; ga < ngroups; ++ga) { tab.push_back(ga); tab.push_back(ga); tab.push_back(1); }
  const int ntiles = plan->ntiles = (int)tab.size() / 3;
  plan->nstages = bordered ? 2 * Bg + 1 : ngroups;
  // the order the stages are worked through: a border's rows of group g, tile (g, Bg), right behind the leading system's stage g —
  // the border's workgroup then has one group's time for them (everything it needs of the leading factor is there by then)
  if (bordered) { for (int g = 0; g < Bg; ++g) { tt->stage_order.push_back(g); tt->stage_order.push_back(Bg + g); } tt->stage_order.push_back(2 * Bg); }
  else for (int g = 0; g < plan->nstages; ++g) tt->stage_order.push_back(g);
  tt->stage_of_tile.assign(ntiles, 0);
  for (int t = 0; t < ntiles; ++t) tt->stage_of_tile[t] = stage_of(tab[3 * t], tab[3 * t + 1], tt->self(t));
  // the pair tiles share `target` workgroups, same number for every tile; the self tiles (much lighter) get 2 per CU in
  // total.  (Sizing each stage's workgroups to whole rounds of slots was tried for the pipelined schedule: no gain, and
  // the two schedules would no longer add in the same order.)
  const int nW = (P + 63) / 64;  // mask words that hold points
  const int ns_pair = PairSegmentsPerTile(C, P, staged, cus, sw), ns_self = SelfSegmentsPerTile(C, P, ngroups, cus, sw);
  const std::vector<int> bound_pair = SegmentBounds(nW, ns_pair, PairSegmentTaper(C)), bound_self = SegmentBounds(nW, ns_self);
  // Up to 64 cameras (both schedules: they add in the same order) the reduction groups are smaller: the last arriver of a group adds it
  // through ONE compute unit (~30 GB/s beside the rest of the kernel: 22 us for eight partial blocks, measured), and a
  // group whose last segment ends late in its stage is what the stage's flag waits for
  // (measured at 64 cameras x 100k points, ms per iteration: groups of 8: 0.411, 6: 0.408, 5: 0.407, 4: 0.406, 3: 0.412, 2: 0.428
  //  — the reducers then read twice the group sums and fall behind)
  // (round 6, beside three factorisation workgroups: 3 and 8 no different from 4 — HISTORY.md)
  const int GRP = 6 * C > RSBA_CHOL_MAXN ? RSBA_GRP : RSBA_GRP_SMALL;
  std::vector<SchurSeg>& sg = plan->sg;
  std::vector<int>& tsp = tt->tsp;
  tsp.assign(ntiles + 1, 0);
  plan->ngrp = 0;
  for (int t = 0; t < ntiles; ++t) {
    const int ns = tt->self(t) ? ns_self : ns_pair;
    const std::vector<int>& bound = tt->self(t) ? bound_self : bound_pair;
    const int s0 = tsp[t], g0 = plan->ngrp;
    const std::vector<int> gsize = GroupSizes(ns, GRP);
    const int ng = (int)gsize.size();
    for (int g = 0, i = 0; g < ng; ++g)
      for (int k = 0; k < gsize[g]; ++k, ++i) {
        SchurSeg e; memset(&e, 0, sizeof(e));
        e.ga = tab[3 * t]; e.gb = tab[3 * t + 1]; e.self = tab[3 * t + 2];
        e.word_begin = bound[i]; e.word_end = bound[i + 1];
        e.tile = t; e.grp = g0 + g; e.grp_seg0 = s0 + i - k; e.grp_nseg = gsize[g];
        e.tile_grp0 = g0; e.tile_ngrp = ng;
        e.stage = tt->stage_of_tile[t];   // (stage_ntiles: below, once the reducers are known)
        sg.push_back(e);
      }
    tsp[t + 1] = (int)sg.size();
    plan->ngrp += ng;
  }
  plan->nseg = (int)sg.size();
  // reducer workgroups (see GroupReduce in ba_schur_tiled.hpp): entries behind the compute segments
  tt->red_of_tile.assign(ntiles, {});
  for (int t = 0; t < ntiles; ++t) {
    const bool self = tt->self(t);
    const SchurSeg first = sg[tsp[t]];
    // a pair tile: one reducer per 3 x 3 quadrant of the pairs' blocks, each finishing its own (ReducerQuadrant);
    // a self tile: one reducer per set of components the K factors do not couple (ReducerSelfSet: six sets of six or nine)
    const int nred = first.tile_ngrp <= RSBA_DIRECT_GROUPS ? 0 : (self ? RSBA_SELF_SETS : 4);
    for (int q = tsp[t]; q < tsp[t + 1]; ++q) sg[q].nred = nred;
    for (int r = 0; r < nred; ++r) {
      SchurSeg e = first;
      e.self = self ? 3 : 2; e.nred = nred;
      e.word_begin = r; e.word_end = r + (self ? (r == 1 || r == 5 ? 9 : 6) : 9);   // (set / quadrant r and its number of components)
      tt->red_of_tile[t].push_back((int)sg.size());
      sg.push_back(e);
    }
  }
  // arrivals at a stage's counter: its self tile, and per pair tile the finisher — or each of the four quadrant reducers
  {
    std::vector<int> arrivals(plan->nstages, 0);
    plan->self_arrivals = 0;
    for (int t = 0; t < ntiles; ++t) {
      const int n_t = sg[tsp[t]].nred != 0 ? sg[tsp[t]].nred : 1;
      arrivals[tt->stage_of_tile[t]] += n_t;
      if (tt->self(t)) plan->self_arrivals += n_t;
    }
    for (auto& e : sg) e.stage_ntiles = arrivals[e.stage];
  }
  for (size_t q = 0; q < sg.size(); ++q) sg[q].index = (int)q;
  plan->nblocks = (int)sg.size();
  plan->nsync = plan->ngrp + 2 * ntiles + RSBA_MAX_STAGES + 2;   // [ngrp] group members | [ntiles] groups done | [RSBA_MAX_STAGES] stage arrivals, [1] self tiles | [ntiles] spare
  plan->nseg_pair = 0;
  for (int q = 0; q < plan->nseg; ++q) if (!sg[q].self) ++plan->nseg_pair;  // pair tiles come first, self tiles after them, reducers last
}

// The compute segments of some tiles interleaved by position inside their tile, so that together they run long blocks first,
// short ones last and all the tiles end together (ties: in the order the tiles are given)
std::vector<int> InterleavedByPosition(const std::vector<int>& tiles, const std::vector<int>& tsp) {
  std::vector<std::pair<double, int>> ord;
  for (int t : tiles) for (int q = tsp[t]; q < tsp[t + 1]; ++q) ord.push_back({(q - tsp[t] + 0.5) / (tsp[t + 1] - tsp[t]), q});
  std::stable_sort(ord.begin(), ord.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first; });
  std::vector<int> out;
  out.reserve(ord.size());
  for (const auto& o : ord) out.push_back(o.second);
  return out;
}

// Block orders of the launch.  Pipelined: stage by stage — the stage's self tile, its pair tiles, then their reducers —
// so that camera group g's columns are complete as early as possible.  Sequential schedule: every pair tile first and
// the (much shorter) self workgroups last, where they fill the tail of the last round of pair workgroups (at 256
// cameras a pair workgroup runs 220 us and the launch is ~3 rounds deep), reducers behind everything.
void PlanOrders(bool staged, const SchurPlanSwitches& sw, SchurPlan* plan, const TileTable& tt) {
  const int ntiles = plan->ntiles, nseg = plan->nseg;
  const std::vector<SchurSeg>& sg = plan->sg;
  const std::vector<int>& tsp = tt.tsp;
  std::vector<int>& border = plan->border;
  border.reserve(plan->nblocks);
  auto append_reducers = [&](std::vector<int>* out, bool self) { for (int t = 0; t < ntiles; ++t) if (tt.self(t) == self) for (int q : tt.red_of_tile[t]) out->push_back(q); };
  if (staged) {
    std::vector<int> red_pending;
    for (int g : tt.stage_order) {
      std::vector<int> tiles_g;   // the stage's self tile, then its pair tiles
      for (int t = 0; t < ntiles; ++t) if (tt.self(t) && tt.stage_of_tile[t] == g) tiles_g.push_back(t);
      for (int t = 0; t < ntiles; ++t) if (!tt.self(t) && tt.stage_of_tile[t] == g) tiles_g.push_back(t);
      // the stage's tiles interleaved by position
      // (the self tile's segments ahead of the pair tiles', so that its slower finish — seven reducers, a tile sum — ends early: 0.400
      //  against 0.3975 ms, the stage's pair segments then all sit at its end)
      // The stage's reducers are drawn RSBA_RED_DELAY entries into the NEXT stage's compute entries, not right behind their own
      // stage's: a reducer holds a workgroup slot (its registers, 72 KB of LDS) from its first poll to the tile's last group, and
      // right behind the stage's last compute entries — which have 40 us to run — that was 46 - 63 us of waiting on 64 slots a launch,
      // 3.5 % of the slot time.  Everything a reducer waits for still has its ticket before it (no deadlock), and who runs what does not
      // change a sum.  Round 5, one box, six alternating runs each: 0 (as before) 0.3464 - 0.3523 (mean 0.3486), 250: 0.3446 - 0.3469
      // (0.3457), 300: 0.3459 - 0.3482 (0.3467), 350: 0.3452 - 0.3573 (0.3485): later than ~300 the stage's flag waits for them.
      int k = 0;
      for (int q : InterleavedByPosition(tiles_g, tsp)) {
        if (k++ == sw.red_delay) { for (int r : red_pending) border.push_back(r); red_pending.clear(); }
        border.push_back(q);
      }
      for (int r : red_pending) border.push_back(r);
      red_pending.clear();
      for (int t : tiles_g) for (int r : tt.red_of_tile[t]) red_pending.push_back(r);
      if (sw.red_delay <= 0) { for (int r : red_pending) border.push_back(r); red_pending.clear(); }
    }
    for (int r : red_pending) border.push_back(r);
  } else if (plan->sparse) {
    // More than 64 cameras (sparse pair segments, PairSegmentSparse): the short self segments first — behind the pair segments
    // their reducers sat in 112 of the 512 slots for 80 us each, waiting for them (there are no reducers any more: at most
    // 16 self segments per tile, two groups, finished by the last arrival) — then the pair segments by POINT RANGE (segment i
    // of every tile, then segment i + 1, ...): the workgroups running at any time gather their point records from a few
    // neighbouring ranges (pair segment 133 -> 110 us)
    for (int q = 0; q < nseg; ++q) if (sg[q].self == 1) border.push_back(q);
    append_reducers(&border, true);
    int ns_pair = 0;
    for (int t = 0; t < ntiles; ++t) if (!tt.self(t)) ns_pair = std::max(ns_pair, tsp[t + 1] - tsp[t]);
    for (int i = 0; i < ns_pair; ++i) for (int t = 0; t < ntiles; ++t) if (!tt.self(t) && i < tsp[t + 1] - tsp[t]) border.push_back(tsp[t] + i);
    append_reducers(&border, false);
  } else {
    for (int q = 0; q < nseg; ++q) border.push_back(q);   // segments are stored pair tiles first, self tiles after them
    for (int t = 0; t < ntiles; ++t) for (int q : tt.red_of_tile[t]) border.push_back(q);
  }
  // First step of a run (pipelined): every self tile ahead of the pair tiles, their reducers right behind them — every
  // camera's diag U is then known early (ready[9]), the factorisation forms its Jacobi scale and is gated stage by stage like
  // in every other iteration instead of waiting for the last stage.
  std::vector<int>& border_first = plan->border_first;
  if (staged) {
    std::vector<int> self_tiles;
    for (int t = 0; t < ntiles; ++t) if (tt.self(t)) self_tiles.push_back(t);
    border_first = InterleavedByPosition(self_tiles, tsp);
    append_reducers(&border_first, true);
    for (int g : tt.stage_order) {
      std::vector<int> pair_g;
      for (int t = 0; t < ntiles; ++t) if (!tt.self(t) && tt.stage_of_tile[t] == g) pair_g.push_back(t);
      for (int q : InterleavedByPosition(pair_g, tsp)) border_first.push_back(q);
      for (int t : pair_g) for (int q : tt.red_of_tile[t]) border_first.push_back(q);
    }
    if ((int)border_first.size() != plan->nblocks) border_first.clear();   // (cannot happen)
  }
  for (int q = 0; q < nseg; ++q) if (sg[q].self == 1) plan->border_self.push_back(q);
  append_reducers(&plan->border_self, true);
  plan->nblocks_self = (int)plan->border_self.size();
}

// More than 64 cameras: the pair segments' hit lists (PairSegmentSparse, ba_schur_tiled.hpp) — per pair segment and wavefront
// `trips` rows of 64 entries (point, the two observations' camera-major positions), a lane's hits dense from row 0.
void PlanHitLists(const PointLayout& lay, SchurPlan* plan, const TileTable& tt) {
  const auto th0 = std::chrono::steady_clock::now();
  const int P = plan->P, ngroups = plan->ngroups, ntiles = plan->ntiles, nseg_pair = plan->nseg_pair;
  const std::vector<int>&pt_ptr = lay.ptr, &obs_cam = lay.cam, &tsp = tt.tsp, &cmpos = plan->cmpos;
  const std::vector<SchurSeg>& sg = plan->sg;
  std::vector<int> tile_of((size_t)ngroups * ngroups, -1);
  for (int t = 0; t < ntiles; ++t) if (!tt.self(t)) tile_of[(size_t)tt.tab[3 * t] * ngroups + tt.tab[3 * t + 1]] = t;
  const int nW = (P + 63) / 64;
  // word -> segment of a pair tile (the same bounds for every pair tile)
  std::vector<int> seg_of_word(nW, 0);
  {
    int t0 = -1;
    for (int t = 0; t < ntiles; ++t) if (!tt.self(t)) { t0 = t; break; }
    for (int q = tsp[t0]; q < tsp[t0 + 1]; ++q) for (int w = sg[q].word_begin; w < sg[q].word_end && w < nW; ++w) seg_of_word[w] = q - tsp[t0];
  }
  // (thread of the workgroup that owns pair (a, b) of point j: see PairSegmentSparse)
  auto owner = [&](int a, int b, int j, int* seg, int* tid) {
    const int ga = a / RSBA_TG, gb = b / RSBA_TG, ia = a - RSBA_TG * ga, ib = b - RSBA_TG * gb;
    const int t = tile_of[(size_t)ga * ngroups + gb];
    const int w = j >> 6;
    *seg = tsp[t] + seg_of_word[w];
    if (ga != gb) { *tid = ia * RSBA_TG + ib; return; }
    const int dt = ia * 15 - ia * (ia - 1) / 2 + ib - ia - 1;           // index of (ia, ib), ia < ib, in kDiagPair
    const int half = (w - sg[*seg].word_begin) & 1;
    *tid = half * 128 + dt;
  };
  std::vector<unsigned> count((size_t)nseg_pair * 256, 0u);
  for (int j = 0; j < P; ++j)
    for (int qa = pt_ptr[j]; qa < pt_ptr[j + 1]; ++qa)
      for (int qb = qa + 1; qb < pt_ptr[j + 1]; ++qb) {
        int seg, tid;
        owner(obs_cam[qa], obs_cam[qb], j, &seg, &tid);
        ++count[(size_t)seg * 256 + tid];
      }
  std::vector<unsigned> off((size_t)nseg_pair * 4, 0u);
  std::vector<int> trips((size_t)nseg_pair * 4, 0);
  size_t entries = 0;
  for (int q = 0; q < nseg_pair; ++q)
    for (int wv = 0; wv < 4; ++wv) {
      unsigned m = 0;
      for (int l = 0; l < 64; ++l) m = std::max(m, count[(size_t)q * 256 + wv * 64 + l]);
      off[(size_t)q * 4 + wv] = (unsigned)entries; trips[(size_t)q * 4 + wv] = (int)m;
      entries += (size_t)m * 64;
    }
  if (entries >= (size_t)1 << 32) return;   // (entries are addressed with 32 bits: the masked search then)
  std::vector<unsigned> h(3 * std::max<size_t>(entries, 1), RSBA_HIT_NONE);
  std::fill(count.begin(), count.end(), 0u);
  for (int j = 0; j < P; ++j)
    for (int qa = pt_ptr[j]; qa < pt_ptr[j + 1]; ++qa)
      for (int qb = qa + 1; qb < pt_ptr[j + 1]; ++qb) {
        int seg, tid;
        owner(obs_cam[qa], obs_cam[qb], j, &seg, &tid);
        const unsigned n = count[(size_t)seg * 256 + tid]++;
        const size_t e = (size_t)off[(size_t)seg * 4 + (tid >> 6)] + (size_t)n * 64 + (tid & 63);
        h[3 * e] = (unsigned)j; h[3 * e + 1] = (unsigned)cmpos[qa]; h[3 * e + 2] = (unsigned)cmpos[qb];
      }
  plan->hits.swap(h); plan->hit_off.swap(off); plan->hit_trips.swap(trips);
  plan->hit_entries = entries;
  plan->hit_count = 0;
  for (unsigned c : count) plan->hit_count += c;
  plan->hit_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - th0).count();
}

}  // namespace

SchurPlan BuildSchurPlan(int C, int P, const PointLayout& layout, bool staged, bool bordered, int cus, const SchurPlanSwitches& sw) {
  SchurPlan plan;
  plan.C = C; plan.P = P;
  plan.ngroups = (C + RSBA_TG - 1) / RSBA_TG;
  plan.nwords = ((P + 63) / 64 + RSBA_CW - 1) / RSBA_CW * RSBA_CW;
  plan.nchunks = plan.nwords / RSBA_CW;
  plan.grid_pp = std::max(1, std::min((P + 255) / 256, 2048));
  // More than 64 cameras: the pair segments' hit lists.  RSBA_SPARSE_PAIRS=0: the masked search of the 512-point chunks, as below 65 cameras.
  plan.sparse = SparsePairSegments(C, sw);
  TileTable tt;
  PlanMasks(layout, &plan);
  PlanSegments(staged, bordered, cus, sw, &plan, &tt);
  PlanOrders(staged, sw, &plan, tt);
  if (plan.sparse && plan.nseg_pair > 0) PlanHitLists(layout, &plan, tt);
  return plan;
}

// ------------------------------------------------------------------------------------------------
// The observations: re-ordered by (point, camera) so that one point's records are contiguous; the permutation is kept so
// nothing the caller sees changes order.
// ------------------------------------------------------------------------------------------------
PointLayout SortObservations(int P, int64_t N, const int32_t* point_index, const int32_t* camera_index, const double* observations) {
  PointLayout lay;
  std::vector<int>& ptr = lay.ptr;
  ptr.assign(P + 1, 0);
  for (int64_t i = 0; i < N; ++i) ptr[point_index[i] + 1]++;
  for (int j = 0; j < P; ++j) { lay.max_views = std::max(lay.max_views, ptr[j + 1]); ptr[j + 1] += ptr[j]; }
  std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
  lay.order.resize(N);
  for (int64_t i = 0; i < N; ++i) lay.order[fill[point_index[i]]++] = i;
  for (int j = 0; j < P; ++j)
    std::stable_sort(lay.order.begin() + ptr[j], lay.order.begin() + ptr[j + 1], [&](int64_t a, int64_t b) { return camera_index[a] < camera_index[b]; });
  lay.u.resize(N); lay.v.resize(N); lay.cam.resize(N);
  for (int64_t q = 0; q < N; ++q) { const int64_t i = lay.order[q]; lay.u[q] = observations[2 * i]; lay.v[q] = observations[2 * i + 1]; lay.cam[q] = camera_index[i]; }
  for (int j = 0; j < P && !lay.duplicate; ++j) for (int q = ptr[j] + 1; q < ptr[j + 1]; ++q) if (lay.cam[q] == lay.cam[q - 1]) { lay.duplicate = true; break; }
  return lay;
}

void OrderAndSlice(int C, int P, bool balance, bool staged, int cus, const SchurPlanSwitches& sw, PointLayout* layout, int max_threads) {
  PointLayout& lay = *layout;
  if (balance) {
    // chunk-balanced point order for the tiled kernel (BalancedPointOrder): everything below is laid out in it
    std::vector<int> perm = BalancedPointOrder(C, P, staged, cus, sw, lay.ptr, lay.cam, max_threads);
    if (!perm.empty()) {
      const std::vector<int>& ptr = lay.ptr;
      const size_t N = lay.cam.size();
      std::vector<int> ptr2(P + 1, 0), cam2(N);
      std::vector<double> u2(N), v2(N);
      std::vector<int64_t> order2(N);
      for (int jn = 0; jn < P; ++jn) ptr2[jn + 1] = ptr2[jn] + (ptr[perm[jn] + 1] - ptr[perm[jn]]);
      for (int jn = 0; jn < P; ++jn) {
        const int b0 = ptr[perm[jn]], n = ptr[perm[jn] + 1] - b0, d0 = ptr2[jn];
        for (int t = 0; t < n; ++t) { u2[d0 + t] = lay.u[b0 + t]; v2[d0 + t] = lay.v[b0 + t]; cam2[d0 + t] = lay.cam[b0 + t]; order2[d0 + t] = lay.order[b0 + t]; }
      }
      lay.ptr.swap(ptr2); lay.cam.swap(cam2); lay.u.swap(u2); lay.v.swap(v2); lay.order.swap(order2);
      lay.pt_perm.swap(perm);
    }
  }
  // sliced-ELL layout: slice = 64 consecutive points, as wide as its widest point
  const std::vector<int>& ptr = lay.ptr;
  const int nslices = (P + 63) / 64;
  lay.sl_ptr.assign(nslices + 1, 0);
  for (int sl = 0; sl < nslices; ++sl) {
    int w = 0;
    for (int j = 64 * sl; j < std::min(P, 64 * sl + 64); ++j) w = std::max(w, ptr[j + 1] - ptr[j]);
    lay.sl_ptr[sl + 1] = lay.sl_ptr[sl] + w;
  }
  lay.sl_elems = (size_t)lay.sl_ptr[nslices] * 64;
  lay.sl_q.assign(lay.sl_elems, -1);
  lay.sl_cam.assign(std::max<size_t>(lay.sl_elems, 1), -1);
  lay.sl_uv.assign(std::max<size_t>(2 * lay.sl_elems, 2), 0.0);
  for (int j = 0; j < P; ++j)
    for (int q = ptr[j]; q < ptr[j + 1]; ++q) {
      const size_t e = ((size_t)lay.sl_ptr[j >> 6] + (q - ptr[j])) * 64 + (j & 63);
      lay.sl_q[e] = q; lay.sl_cam[e] = lay.cam[q]; lay.sl_uv[2 * e] = lay.u[q]; lay.sl_uv[2 * e + 1] = lay.v[q];
    }
}

// ------------------------------------------------------------------------------------------------
namespace {
template <typename T>
unsigned long long Fnv1a(const std::vector<T>& v) {
  unsigned long long h = 0xcbf29ce484222325ull;
  const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t i = 0, n = v.size() * sizeof(T); i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
  return h;
}
}  // namespace

void PrintPlanDigests(const PointLayout& l, const SchurPlan& p) {
#define RSBA_DG(name, vec) fprintf(stderr, " " name "=%016llx", Fnv1a(vec))
  fprintf(stderr, "rsba: plan digest");
  RSBA_DG("ptr", l.ptr); RSBA_DG("cam", l.cam); RSBA_DG("u", l.u); RSBA_DG("v", l.v); RSBA_DG("order", l.order); RSBA_DG("pt_perm", l.pt_perm);
  RSBA_DG("sl_ptr", l.sl_ptr); RSBA_DG("sl_q", l.sl_q); RSBA_DG("sl_cam", l.sl_cam); RSBA_DG("sl_uv", l.sl_uv);
  RSBA_DG("mask", p.mask); RSBA_DG("prefix", p.prefix); RSBA_DG("cptr", p.cptr); RSBA_DG("cmpos", p.cmpos); RSBA_DG("u_cm", p.u_cm); RSBA_DG("v_cm", p.v_cm);
  RSBA_DG("sg", p.sg); RSBA_DG("border", p.border); RSBA_DG("border_first", p.border_first); RSBA_DG("border_self", p.border_self); RSBA_DG("cm_pos", p.cm_pos);
  RSBA_DG("hits", p.hits); RSBA_DG("hit_off", p.hit_off); RSBA_DG("hit_trips", p.hit_trips);
#undef RSBA_DG
  fprintf(stderr, " max_views=%d duplicate=%d ngroups=%d nwords=%d nchunks=%d ntiles=%d nstages=%d ngrp=%d nseg=%d nseg_pair=%d nblocks=%d nblocks_self=%d nsync=%d"
                  " self_arrivals=%d grid_pp=%d hit_entries=%zu\n",
          l.max_views, (int)l.duplicate, p.ngroups, p.nwords, p.nchunks, p.ntiles, p.nstages, p.ngrp, p.nseg, p.nseg_pair, p.nblocks, p.nblocks_self, p.nsync,
          p.self_arrivals, p.grid_pp, p.hit_entries);
}

}  // namespace rsba
