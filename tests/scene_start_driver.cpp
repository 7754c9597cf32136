// Stand-alone check of the scene start's host units (csrc/ba_scene_start_plan.hpp, csrc/ba_resection.hpp with markers as a third kind of
// block), built with -fsanitize=address,undefined by tests/test_scene_start_plan_host.py and run as a program:
//   plan FILE   cases of "C T M N sweeps has_known base_marker", the C + T + M flags when has_known, then N lines "camera time marker": each
//               is planned, the contracts the kernels rely on are checked here (the lists, the launches' blocks, grids and byte counts, the
//               buffers; with every marker flagged, that the launches are PlanRigStart's), and the rounds, sweeps and unreachable blocks are
//               printed as one JSON line for the test to hold against tests/scene_start_ref.py
//   fit FILE    one problem: "all_markers C T M N has_dist side sweeps has_known", intrinsics, coefficients, parameters, flags, then N lines
//               "camera time marker" + eight corner values.  The whole start runs serially: FitMarkerPose per detection, then every
//               launch of the plan block by block through ResectBlock<SerialLanes>, summing in observation order.  Prints the C + T + M
//               blocks, statuses, RMS and iteration counts as one JSON line.
//   (no argument)   the cases a file does not express: empty problems, refused arguments.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ba_resection.hpp"
#include "ba_scene_start_plan.hpp"

namespace {

int g_fail = 0;
void Expect(bool ok, const char* what, int where) {
  if (!ok) { ++g_fail; if (g_fail < 20) fprintf(stderr, "FAIL %s (%d)\n", what, where); }
}

unsigned GridOf(int which, int count) { return which == rsba::kRigStartTime ? (unsigned)((count + 3) / 4) : (unsigned)count; }

void CheckPlan(const rsba::SceneStartPlan& p, const std::vector<int32_t>& cam, const std::vector<int32_t>& tim, const std::vector<int32_t>& mar,
               const uint8_t* flags, bool base_marker, int sweeps, bool with_dist, int id) {
  const int C = p.C, T = p.T, M = p.M;
  const size_t N = (size_t)p.N, nb = (size_t)C + T + M;
  const std::vector<int>* ptrs[3] = {&p.time_ptr, &p.camera_ptr, &p.marker_ptr};
  const std::vector<int>* lists[3] = {&p.time_obs, &p.camera_obs, &p.marker_obs};
  const std::vector<int32_t>* keys[3] = {&tim, &cam, &mar};
  const int counts[3] = {T, C, M};
  const size_t base[3] = {(size_t)C, 0, (size_t)C + T};
  // the lists: every observation once, in its block, ascending
  for (int kind = 0; kind < 3; ++kind) {
    const std::vector<int>&ptr = *ptrs[kind], &obs = *lists[kind];
    const int n = counts[kind];
    Expect((int)ptr.size() == n + 1 && obs.size() == N && ptr[0] == 0 && ptr[(size_t)n] == (int)N, "list sizes", id);
    std::vector<int> seen(N, 0);
    for (int b = 0; b < n; ++b) {
      Expect(ptr[(size_t)b] <= ptr[(size_t)b + 1], "ptr ascending", id);
      for (int k = ptr[(size_t)b]; k < ptr[(size_t)b + 1]; ++k) {
        const int o = obs[(size_t)k];
        Expect(o >= 0 && (size_t)o < N && (*keys[kind])[(size_t)o] == b, "observation in its block", id);
        if (o >= 0 && (size_t)o < N) ++seen[(size_t)o];
        if (k > ptr[(size_t)b]) Expect(obs[(size_t)k - 1] < o, "ascending inside a block", id);
      }
    }
    for (size_t o = 0; o < N; ++o) Expect(seen[o] == 1, "every observation once", id);
  }
  // the given blocks
  for (size_t b = 0; b < nb; ++b) {
    const bool want = (flags && flags[b]) || (b == 0 && C > 0) || (b == (size_t)C + T && M > 0 && base_marker);
    Expect((p.given[b] != 0) == want, "given", (int)b);
  }
  // the launches: a round fits a block once, and only a block with a detection whose two other blocks were known before the round
  size_t at = 0;
  int rounds = 0;
  std::vector<int> fitted(nb, 0);
  std::vector<uint8_t> known(p.given);
  for (size_t k = 0; k < p.launches.size(); ++k) {
    const rsba::RigStartLaunch& l = p.launches[k];
    Expect(l.which >= 0 && l.which <= 2, "kind", id);
    if (l.which < 0 || l.which > 2) return;
    Expect((size_t)l.first == at && l.count > 0 && at + (size_t)l.count <= p.blocks.size(), "block range", id);
    Expect(l.grid == GridOf(l.which, l.count) && (size_t)l.grid * (l.which == rsba::kRigStartTime ? 4 : 1) >= (size_t)l.count, "grid", id);
    int64_t nobs = 0;
    const std::vector<int>&ptr = *ptrs[l.which], &obs = *lists[l.which];
    const std::vector<uint8_t> before(known);
    for (int j = 0; j < l.count; ++j) {
      const int b = p.blocks[at + (size_t)j];
      Expect(b >= 0 && b < counts[l.which], "block index", id);
      if (b < 0 || b >= counts[l.which]) continue;
      if (j > 0) Expect(p.blocks[at + (size_t)j - 1] < b, "blocks ascending", id);
      nobs += ptr[(size_t)b + 1] - ptr[(size_t)b];
      const size_t pb = base[l.which] + (size_t)b;
      Expect(!p.given[pb], "a given block is never fitted", id);
      if (l.sweep == 0) {
        Expect(fitted[pb] == 0 && p.round_of[pb] == (int)k, "a round fits a block once", id);
        fitted[pb] = 1;
        bool usable = false;
        for (int q = ptr[(size_t)b]; q < ptr[(size_t)b + 1]; ++q) {
          const size_t o = (size_t)obs[(size_t)q];
          const bool c = before[(size_t)cam[o]] != 0, t = before[(size_t)C + tim[o]] != 0, m = before[(size_t)C + T + mar[o]] != 0;
          usable = usable || (l.which == rsba::kRigStartTime ? c && m : l.which == rsba::kRigStartCamera ? t && m : c && t);
        }
        Expect(usable, "a fitted block has a usable detection", id);
        known[pb] = 1;
      } else {
        Expect(fitted[pb] == 1, "a sweep fits what the rounds reached", id);
      }
    }
    Expect(l.observations == nobs && l.list_bytes == (size_t)l.count * 4 && l.read_bytes == (size_t)nobs * 80, "byte counts", id);
    if (l.sweep == 0) { Expect((int)k == rounds, "rounds first", id); ++rounds; }
    if (k > 0 && l.sweep == 0) Expect(p.launches[k - 1].which != l.which, "rounds take turns", id);
    Expect(l.sweep >= 0 && l.sweep <= sweeps, "sweep number", id);
    at += (size_t)l.count;
  }
  Expect(at == p.blocks.size() && rounds == p.num_rounds, "launches cover the block list", id);
  for (size_t b = 0; b < nb; ++b) {
    const bool unreachable = p.round_of[b] == -2;
    Expect((p.round_of[b] == -1) == (p.given[b] != 0) && (unreachable == (!p.given[b] && !fitted[b])), "round_of", id);
  }
  Expect(p.unreachable_times.size() + p.unreachable_cameras.size() + p.unreachable_markers.size() + (size_t)std::count(fitted.begin(), fitted.end(), 1) +
             (size_t)std::count(p.given.begin(), p.given.end(), 1) == nb, "every block is given, fitted or unreachable", id);
  // the buffers: in order, aligned, each as large as its array
  const rsba::SceneStartBuffers& b = p.buffers;
  const size_t off[] = {b.observations, b.intrinsics, b.distortion, b.parameters, b.own_pose, b.own_rms, b.block_rms, b.camera_index, b.time_index,
                        b.marker_index, b.own_status, b.masked_index, b.time_ptr, b.time_obs, b.camera_ptr, b.camera_obs, b.marker_ptr, b.marker_obs, b.blocks,
                        b.block_status, b.block_iterations, b.known, b.total};
  const size_t need[] = {64 * N, 32 * (size_t)C, with_dist ? 40 * (size_t)C : 0, 48 * nb, 48 * N, 8 * N, 8 * nb, 4 * N, 4 * N,
                         4 * N, 4 * N, 4 * N, 4 * ((size_t)T + 1), 4 * N, 4 * ((size_t)C + 1), 4 * N, 4 * ((size_t)M + 1), 4 * N, 4 * p.blocks.size(),
                         4 * nb, 4 * nb, nb + 1};
  size_t up = 0;
  for (int k = 0; k < 22; ++k) {
    Expect(off[k] % 8 == 0 && off[k + 1] >= off[k] + need[k] && off[k + 1] < off[k] + need[k] + 8, "buffer", k);
    if (k != 4 && k != 5 && k != 10 && k != 11) up += off[k + 1] - off[k];   // (own fits and masked indices are made on the device)
  }
  // the hidden flag: past every block's, where a time launch (known[index]) and a camera launch (known[C + index]) both find it
  Expect((size_t)rsba::SceneStartHiddenIndex(rsba::kRigStartTime, C, T, M) == nb && (size_t)C + (size_t)rsba::SceneStartHiddenIndex(rsba::kRigStartCamera, C, T, M) == nb,
         "hidden index", id);
  Expect(b.observations == 0 && p.upload_bytes == up && p.download_bytes == 48 * nb + 8 * nb + 8 * nb, "transfer sizes", id);
  // every marker flagged: the launches of the whole-rig start for the same camera and time flags
  bool all_markers = flags != nullptr;
  for (int m = 0; m < M && all_markers; ++m) all_markers = flags[(size_t)C + T + m] != 0;
  if (all_markers) {
    rsba::RigStartPlan r;
    Expect(rsba::PlanRigStart(C, T, M, p.N, cam.data(), tim.data(), flags, sweeps, with_dist, &r), "the rig plan", id);
    bool same = r.launches.size() == p.launches.size() && r.blocks == p.blocks && r.num_rounds == p.num_rounds && r.unreachable_times == p.unreachable_times &&
                r.unreachable_cameras == p.unreachable_cameras && p.unreachable_markers.empty();
    for (size_t k = 0; same && k < r.launches.size(); ++k) {
      const rsba::RigStartLaunch &x = r.launches[k], &y = p.launches[k];
      same = x.which == y.which && x.sweep == y.sweep && x.first == y.first && x.count == y.count && x.grid == y.grid && x.observations == y.observations;
    }
    Expect(same, "every marker flagged: the whole-rig start's launches", id);
  }
}

void PrintList(const char* name, const std::vector<int>& v, const char* tail) {
  printf("\"%s\": [", name);
  for (size_t k = 0; k < v.size(); ++k) printf("%s%d", k ? ", " : "", v[k]);
  printf("]%s", tail);
}

int Plan(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  int C, T, M, sweeps, has_known, base_marker, id = 0;
  long long N;
  while (fscanf(f, "%d %d %d %lld %d %d %d", &C, &T, &M, &N, &sweeps, &has_known, &base_marker) == 7) {
    std::vector<uint8_t> known((size_t)C + T + M, 0);
    if (has_known) for (uint8_t& v : known) { int x = 0; if (fscanf(f, "%d", &x) != 1) { fclose(f); return 2; } v = (uint8_t)x; }
    std::vector<int32_t> cam((size_t)N), tim((size_t)N), mar((size_t)N);
    for (long long i = 0; i < N; ++i) if (fscanf(f, "%d %d %d", &cam[(size_t)i], &tim[(size_t)i], &mar[(size_t)i]) != 3) { fclose(f); return 2; }
    rsba::SceneStartPlan p;
    const bool with_dist = id % 2 == 1;
    const uint8_t* flags = has_known ? known.data() : nullptr;
    const bool ok = rsba::PlanSceneStart(C, T, M, N, cam.data(), tim.data(), mar.data(), flags, base_marker != 0, sweeps, with_dist, &p);
    Expect(ok, "planned", id);
    if (ok) CheckPlan(p, cam, tim, mar, flags, base_marker != 0, sweeps, with_dist, id);
    printf("{\"launches\": [");
    for (size_t k = 0; k < p.launches.size(); ++k) {
      const rsba::RigStartLaunch& l = p.launches[k];
      printf("%s{\"which\": %d, \"sweep\": %d, \"grid\": %u, ", k ? ", " : "", l.which, l.sweep, l.grid);
      PrintList("blocks", std::vector<int>(p.blocks.begin() + l.first, p.blocks.begin() + l.first + l.count), "}");
    }
    printf("], \"num_rounds\": %d, ", p.num_rounds);
    PrintList("unreachable_times", p.unreachable_times, ", ");
    PrintList("unreachable_cameras", p.unreachable_cameras, ", ");
    PrintList("unreachable_markers", p.unreachable_markers, ", ");
    PrintList("time_ptr", p.time_ptr, ", ");
    PrintList("camera_ptr", p.camera_ptr, ", ");
    PrintList("marker_ptr", p.marker_ptr, ", ");
    PrintList("time_obs", p.time_obs, ", ");
    PrintList("camera_obs", p.camera_obs, ", ");
    PrintList("marker_obs", p.marker_obs, "}\n");
    ++id;
  }
  fclose(f);
  return 0;
}

int Fit(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  int all_markers, C, T, M, has_dist, sweeps, has_known;
  long long N;
  double side;
  if (fscanf(f, "%d %d %d %d %lld %d %lf %d %d", &all_markers, &C, &T, &M, &N, &has_dist, &side, &sweeps, &has_known) != 9) { fclose(f); return 2; }
  const size_t nb = (size_t)C + T + M, n = (size_t)N;
  std::vector<double> intr(4 * (size_t)C), dist(5 * (size_t)C), params(6 * nb), obs(8 * n);
  std::vector<uint8_t> known(nb, 0);
  std::vector<int32_t> cam(n), tim(n), mar(n);
  bool ok = true;
  for (double& v : intr) ok = ok && fscanf(f, "%lf", &v) == 1;
  if (has_dist) for (double& v : dist) ok = ok && fscanf(f, "%lf", &v) == 1;
  for (double& v : params) ok = ok && fscanf(f, "%lf", &v) == 1;
  if (has_known) for (uint8_t& v : known) { int x = 0; ok = ok && fscanf(f, "%d", &x) == 1; v = (uint8_t)x; }
  for (size_t i = 0; i < n; ++i) {
    ok = ok && fscanf(f, "%d %d %d", &cam[i], &tim[i], &mar[i]) == 3;
    for (int q = 0; q < 8; ++q) ok = ok && fscanf(f, "%lf", &obs[8 * i + (size_t)q]) == 1;
  }
  fclose(f);
  if (!ok) { fprintf(stderr, "malformed problem file\n"); return 2; }
  rsba::SceneStartPlan plan;
  const uint8_t* flags = has_known ? known.data() : nullptr;
  if (!rsba::PlanSceneStart(C, T, M, N, cam.data(), tim.data(), mar.data(), flags, all_markers == 0, sweeps, has_dist != 0, &plan)) return 2;
  CheckPlan(plan, cam, tim, mar, flags, all_markers == 0, sweeps, has_dist != 0, 0);
  std::vector<double> own_pose(6 * n), own_rms(n), rms(nb, -1.0);
  std::vector<int32_t> own_status(n), status(nb), iterations(nb, 0);
  for (size_t i = 0; i < n; ++i)
    own_status[i] = rsba::FitMarkerPose(&obs[8 * i], &intr[4 * (size_t)cam[i]], has_dist ? &dist[5 * (size_t)cam[i]] : nullptr, side, &own_pose[6 * i], &own_rms[i]);
  for (size_t b = 0; b < nb; ++b) status[b] = plan.given[b] ? rsba::BLOCK_GIVEN : rsba::BLOCK_UNREACHED;
  std::vector<uint8_t> state(plan.given);
  const std::vector<double> before(params);
  rsba::ResectionArgs a{};
  a.all_markers = all_markers; a.C = C; a.T = T; a.half = 0.5 * side;
  a.camera_index = cam.data(); a.time_index = tim.data(); a.marker_index = mar.data();
  a.observations = obs.data(); a.intrinsics = intr.data(); a.distortion = has_dist ? dist.data() : nullptr;
  a.own_pose = own_pose.data(); a.own_rms = own_rms.data(); a.own_status = own_status.data();
  a.parameters = params.data(); a.known = state.data(); a.status = status.data(); a.rms = rms.data(); a.iterations = iterations.data();
  a.markers_flagged = 1;
  rsba::SerialLanes lanes;
  for (const rsba::RigStartLaunch& l : plan.launches) {
    a.blocks = plan.blocks.data() + l.first;
    a.num_blocks = l.count;
    a.list_ptr = l.which == rsba::kRigStartTime ? plan.time_ptr.data() : l.which == rsba::kRigStartCamera ? plan.camera_ptr.data() : plan.marker_ptr.data();
    a.list_obs = l.which == rsba::kRigStartTime ? plan.time_obs.data() : l.which == rsba::kRigStartCamera ? plan.camera_obs.data() : plan.marker_obs.data();
    const int which = l.which == rsba::kRigStartTime ? rsba::RESECT_TIME : l.which == rsba::kRigStartCamera ? rsba::RESECT_CAMERA : rsba::RESECT_MARKER;
    for (int k = 0; k < l.count; ++k) rsba::ResectBlock(a, which, a.blocks[k], lanes);
  }
  // a block without a fit keeps its bits
  for (size_t b = 0; b < nb; ++b)
    if (status[b] > rsba::BLOCK_ITERATION_CAP) Expect(memcmp(&params[6 * b], &before[6 * b], 48) == 0, "kept bits", (int)b);
  printf("{\"blocks\": [");
  for (size_t k = 0; k < 6 * nb; ++k) printf("%s%.17g", k ? ", " : "", params[k]);
  printf("], \"rms\": [");
  for (size_t k = 0; k < nb; ++k) printf("%s%.17g", k ? ", " : "", rms[k]);
  printf("], \"status\": [");
  for (size_t k = 0; k < nb; ++k) printf("%s%d", k ? ", " : "", status[k]);
  printf("], \"iterations\": [");
  for (size_t k = 0; k < nb; ++k) printf("%s%d", k ? ", " : "", iterations[k]);
  printf("]}\n");
  return 0;
}

void Builtin() {
  rsba::SceneStartPlan p;
  // empty problems
  Expect(rsba::PlanSceneStart(0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, true, 2, false, &p) && p.launches.empty() && p.blocks.empty() && p.buffers.total % 8 == 0,
         "nothing at all", 0);
  CheckPlan(p, {}, {}, {}, nullptr, true, 2, false, 100);
  Expect(rsba::PlanSceneStart(3, 4, 2, 0, nullptr, nullptr, nullptr, nullptr, true, 1, true, &p) && p.launches.empty(), "no observations", 1);
  CheckPlan(p, {}, {}, {}, nullptr, true, 1, true, 101);
  Expect(p.unreachable_times.size() == 4 && p.unreachable_cameras.size() == 2 && p.unreachable_markers.size() == 1 && p.given[0] == 1 && p.given[7] == 1,
         "no observations: all but the base camera and the base marker unreachable", 1);
  Expect(rsba::PlanSceneStart(3, 4, 2, 0, nullptr, nullptr, nullptr, nullptr, false, 1, true, &p) && p.unreachable_markers.size() == 2 && p.given[7] == 0,
         "every marker an ordinary block: marker 0 is not given", 2);
  // refused
  const int32_t c1[2] = {0, 3}, t1[2] = {0, 1}, m1[2] = {0, 2}, tneg[2] = {0, -1}, mneg[2] = {-1, 0};
  Expect(!rsba::PlanSceneStart(3, 2, 3, 2, c1, t1, m1, nullptr, true, 0, false, &p), "camera index out of range", 3);
  Expect(!rsba::PlanSceneStart(4, 1, 3, 2, c1, t1, m1, nullptr, true, 0, false, &p), "time index out of range", 4);
  Expect(!rsba::PlanSceneStart(4, 2, 2, 2, c1, t1, m1, nullptr, true, 0, false, &p), "marker index out of range", 5);
  Expect(!rsba::PlanSceneStart(4, 2, 3, 2, c1, tneg, m1, nullptr, true, 0, false, &p), "negative time index", 6);
  Expect(!rsba::PlanSceneStart(4, 2, 3, 2, c1, t1, mneg, nullptr, true, 0, false, &p), "negative marker index", 7);
  Expect(!rsba::PlanSceneStart(4, 2, 3, 2, c1, t1, m1, nullptr, true, -1, false, &p), "negative sweeps", 8);
  Expect(!rsba::PlanSceneStart(4, 2, 3, 2, c1, t1, nullptr, nullptr, true, 0, false, &p), "null indices", 9);
  Expect(!rsba::PlanSceneStart(4, 2, 3, (int64_t)1 << 31, c1, t1, m1, nullptr, true, 0, false, &p), "too many observations", 10);
  Expect(!rsba::PlanSceneStart(4, 2, 3, 2, c1, t1, m1, nullptr, true, 0, false, nullptr), "null plan", 11);
  Expect(rsba::PlanSceneStart(4, 2, 3, 2, c1, t1, m1, nullptr, true, 0, false, &p) && p.num_rounds == 1, "the same arguments in range", 12);
}

}  // namespace

int main(int argc, char** argv) {
  int rc = 0;
  if (argc == 3 && std::string(argv[1]) == "plan") rc = Plan(argv[2]);
  else if (argc == 3 && std::string(argv[1]) == "fit") rc = Fit(argv[2]);
  else if (argc == 1) Builtin();
  else { fprintf(stderr, "usage: scene_start_driver [plan FILE | fit FILE]\n"); return 2; }
  if (rc) return rc;
  if (g_fail) { fprintf(stderr, "scene start driver: %d failures\n", g_fail); return 1; }
  fprintf(stderr, "scene start driver: ok\n");
  return 0;
}
