// Stand-alone check of the whole-rig start's host units (csrc/ba_rig_start_plan.hpp, csrc/ba_resection.hpp), built with
// -fsanitize=address,undefined by tests/test_rig_start_plan_host.py and run as a program:
//   plan FILE   cases of "C T M N sweeps has_known", the C + T flags when has_known, then N lines "camera time": each is planned, the
//               contracts the kernels rely on are checked here (the lists, the launches' blocks, grids and byte counts, the buffers), and
//               the rounds, sweeps and unreachable blocks are printed as one JSON line for the test to hold against tests/rig_start_ref.py
//   fit FILE    one problem: "all_markers C T M N has_dist side sweeps has_known", intrinsics, coefficients, parameters, flags, then N lines
//               "camera time marker" + eight corner values.  The whole start runs serially: FitMarkerPose per detection, then every
//               launch of the plan block by block through ResectBlock<SerialLanes>, summing in observation order.  Prints the C + T
//               blocks, statuses, RMS and iteration counts as one JSON line.
//   (no argument)   the cases a file does not express: empty problems, refused arguments.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ba_resection.hpp"
#include "ba_rig_start_plan.hpp"

namespace {

int g_fail = 0;
void Expect(bool ok, const char* what, int where) {
  if (!ok) { ++g_fail; if (g_fail < 20) fprintf(stderr, "FAIL %s (%d)\n", what, where); }
}

void CheckPlan(const rsba::RigStartPlan& p, const std::vector<int32_t>& cam, const std::vector<int32_t>& tim, int sweeps, bool with_dist, int id) {
  const int C = p.C, T = p.T;
  const size_t N = (size_t)p.N;
  // the lists: every observation once, in its block, ascending
  for (int pass = 0; pass < 2; ++pass) {
    const std::vector<int>& ptr = pass ? p.camera_ptr : p.time_ptr;
    const std::vector<int>& obs = pass ? p.camera_obs : p.time_obs;
    const std::vector<int32_t>& key = pass ? cam : tim;
    const int n = pass ? C : T;
    Expect((int)ptr.size() == n + 1 && obs.size() == N && ptr[0] == 0 && ptr[(size_t)n] == (int)N, "list sizes", id);
    std::vector<int> seen(N, 0);
    for (int b = 0; b < n; ++b) {
      Expect(ptr[(size_t)b] <= ptr[(size_t)b + 1], "ptr ascending", id);
      for (int k = ptr[(size_t)b]; k < ptr[(size_t)b + 1]; ++k) {
        const int o = obs[(size_t)k];
        Expect(o >= 0 && (size_t)o < N && key[(size_t)o] == b, "observation in its block", id);
        if (o >= 0 && (size_t)o < N) ++seen[(size_t)o];
        if (k > ptr[(size_t)b]) Expect(obs[(size_t)k - 1] < o, "ascending inside a block", id);
      }
    }
    for (size_t o = 0; o < N; ++o) Expect(seen[o] == 1, "every observation once", id);
  }
  // the launches
  size_t at = 0;
  int rounds = 0;
  std::vector<int> fitted((size_t)C + T, 0);
  for (size_t k = 0; k < p.launches.size(); ++k) {
    const rsba::RigStartLaunch& l = p.launches[k];
    Expect((size_t)l.first == at && l.count > 0 && at + (size_t)l.count <= p.blocks.size(), "block range", id);
    Expect(l.grid == (l.which == rsba::kRigStartTime ? (unsigned)((l.count + 3) / 4) : (unsigned)l.count), "grid", id);
    Expect((size_t)l.grid * (l.which == rsba::kRigStartTime ? 4 : 1) >= (size_t)l.count, "grid covers the blocks", id);
    int64_t nobs = 0;
    for (int j = 0; j < l.count; ++j) {
      const int b = p.blocks[at + (size_t)j];
      const int n = l.which == rsba::kRigStartTime ? T : C;
      Expect(b >= 0 && b < n, "block index", id);
      if (b < 0 || b >= n) continue;
      if (j > 0) Expect(p.blocks[at + (size_t)j - 1] < b, "blocks ascending", id);
      const std::vector<int>& ptr = l.which == rsba::kRigStartTime ? p.time_ptr : p.camera_ptr;
      nobs += ptr[(size_t)b + 1] - ptr[(size_t)b];
      const size_t pb = l.which == rsba::kRigStartTime ? (size_t)C + b : (size_t)b;
      Expect(!p.given[pb], "a given block is never fitted", id);
      if (l.sweep == 0) { Expect(fitted[pb] == 0 && p.round_of[pb] == (int)k, "a round fits a block once", id); fitted[pb] = 1; }
      else Expect(fitted[pb] == 1, "a sweep fits what the rounds reached", id);
    }
    Expect(l.observations == nobs && l.list_bytes == (size_t)l.count * 4 && l.read_bytes == (size_t)nobs * 80, "byte counts", id);
    if (l.sweep == 0) { Expect((int)k == rounds, "rounds first", id); ++rounds; }
    if (k > 0 && l.sweep == 0) Expect(p.launches[k - 1].which != l.which, "rounds alternate", id);
    Expect(l.sweep >= 0 && l.sweep <= sweeps, "sweep number", id);
    at += (size_t)l.count;
  }
  Expect(at == p.blocks.size() && rounds == p.num_rounds, "launches cover the block list", id);
  for (size_t b = 0; b < (size_t)C + T; ++b) {
    const bool unreachable = p.round_of[b] == -2;
    Expect((p.round_of[b] == -1) == (p.given[b] != 0) && (unreachable == (!p.given[b] && !fitted[b])), "round_of", id);
  }
  Expect(p.unreachable_times.size() + p.unreachable_cameras.size() + (size_t)std::count(fitted.begin(), fitted.end(), 1) +
             (size_t)std::count(p.given.begin(), p.given.end(), 1) == (size_t)C + T, "every block is given, fitted or unreachable", id);
  // the buffers: in order, aligned, each as large as its array
  const rsba::RigStartBuffers& b = p.buffers;
  const size_t nb = (size_t)C + T, M = (size_t)p.M;
  const size_t off[] = {b.observations, b.intrinsics, b.distortion, b.parameters, b.own_pose, b.own_rms, b.block_rms, b.camera_index, b.time_index,
                        b.marker_index, b.own_status, b.time_ptr, b.time_obs, b.camera_ptr, b.camera_obs, b.blocks, b.block_status, b.block_iterations,
                        b.known, b.total};
  const size_t need[] = {64 * N, 32 * (size_t)C, with_dist ? 40 * (size_t)C : 0, 48 * (nb + M), 48 * N, 8 * N, 8 * nb, 4 * N, 4 * N,
                         4 * N, 4 * N, 4 * ((size_t)T + 1), 4 * N, 4 * ((size_t)C + 1), 4 * N, 4 * p.blocks.size(), 4 * nb, 4 * nb, nb};
  size_t up = 0;
  for (int k = 0; k < 19; ++k) {
    Expect(off[k] % 8 == 0 && off[k + 1] >= off[k] + need[k] && off[k + 1] < off[k] + need[k] + 8, "buffer", k);
    if (k != 4 && k != 5 && k != 10) up += off[k + 1] - off[k];
  }
  Expect(b.observations == 0 && p.upload_bytes == up && p.download_bytes == 48 * nb + 8 * nb + 8 * nb, "transfer sizes", id);
}

void PrintList(const char* name, const std::vector<int>& v, const char* tail) {
  printf("\"%s\": [", name);
  for (size_t k = 0; k < v.size(); ++k) printf("%s%d", k ? ", " : "", v[k]);
  printf("]%s", tail);
}

int Plan(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  int C, T, M, sweeps, has_known, id = 0;
  long long N;
  while (fscanf(f, "%d %d %d %lld %d %d", &C, &T, &M, &N, &sweeps, &has_known) == 6) {
    std::vector<uint8_t> known((size_t)C + T, 0);
    if (has_known) for (uint8_t& v : known) { int x = 0; if (fscanf(f, "%d", &x) != 1) return 2; v = (uint8_t)x; }
    std::vector<int32_t> cam((size_t)N), tim((size_t)N);
    for (long long i = 0; i < N; ++i) if (fscanf(f, "%d %d", &cam[(size_t)i], &tim[(size_t)i]) != 2) return 2;
    rsba::RigStartPlan p;
    const bool with_dist = id % 2 == 1;
    const bool ok = rsba::PlanRigStart(C, T, M, N, cam.data(), tim.data(), has_known ? known.data() : nullptr, sweeps, with_dist, &p);
    Expect(ok, "planned", id);
    if (ok) CheckPlan(p, cam, tim, sweeps, with_dist, id);
    printf("{\"launches\": [");
    for (size_t k = 0; k < p.launches.size(); ++k) {
      const rsba::RigStartLaunch& l = p.launches[k];
      printf("%s{\"which\": %d, \"sweep\": %d, \"grid\": %u, ", k ? ", " : "", l.which, l.sweep, l.grid);
      PrintList("blocks", std::vector<int>(p.blocks.begin() + l.first, p.blocks.begin() + l.first + l.count), "}");
    }
    printf("], \"num_rounds\": %d, ", p.num_rounds);
    PrintList("unreachable_times", p.unreachable_times, ", ");
    PrintList("unreachable_cameras", p.unreachable_cameras, ", ");
    PrintList("time_ptr", p.time_ptr, ", ");
    PrintList("camera_ptr", p.camera_ptr, ", ");
    PrintList("time_obs", p.time_obs, ", ");
    PrintList("camera_obs", p.camera_obs, "}\n");
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
  if (fscanf(f, "%d %d %d %d %lld %d %lf %d %d", &all_markers, &C, &T, &M, &N, &has_dist, &side, &sweeps, &has_known) != 9) return 2;
  const size_t nb = (size_t)C + T, n = (size_t)N;
  std::vector<double> intr(4 * (size_t)C), dist(5 * (size_t)C), params(6 * (nb + (size_t)M)), obs(8 * n);
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
  rsba::RigStartPlan plan;
  if (!rsba::PlanRigStart(C, T, M, N, cam.data(), tim.data(), has_known ? known.data() : nullptr, sweeps, has_dist != 0, &plan)) return 2;
  CheckPlan(plan, cam, tim, sweeps, has_dist != 0, 0);
  std::vector<double> own_pose(6 * n), own_rms(n), rms(nb, -1.0);
  std::vector<int32_t> own_status(n), status(nb), iterations(nb, 0);
  for (size_t i = 0; i < n; ++i)
    own_status[i] = rsba::FitMarkerPose(&obs[8 * i], &intr[4 * (size_t)cam[i]], has_dist ? &dist[5 * (size_t)cam[i]] : nullptr, side, &own_pose[6 * i], &own_rms[i]);
  for (size_t b = 0; b < nb; ++b) status[b] = plan.given[b] ? rsba::BLOCK_GIVEN : rsba::BLOCK_UNREACHED;
  std::vector<uint8_t> flags(plan.given);
  const std::vector<double> before(params);
  rsba::ResectionArgs a{};
  a.all_markers = all_markers; a.C = C; a.T = T; a.half = 0.5 * side;
  a.camera_index = cam.data(); a.time_index = tim.data(); a.marker_index = mar.data();
  a.observations = obs.data(); a.intrinsics = intr.data(); a.distortion = has_dist ? dist.data() : nullptr;
  a.own_pose = own_pose.data(); a.own_rms = own_rms.data(); a.own_status = own_status.data();
  a.parameters = params.data(); a.known = flags.data(); a.status = status.data(); a.rms = rms.data(); a.iterations = iterations.data();
  rsba::SerialLanes lanes;
  for (const rsba::RigStartLaunch& l : plan.launches) {
    a.blocks = plan.blocks.data() + l.first;
    a.num_blocks = l.count;
    a.list_ptr = l.which == rsba::kRigStartTime ? plan.time_ptr.data() : plan.camera_ptr.data();
    a.list_obs = l.which == rsba::kRigStartTime ? plan.time_obs.data() : plan.camera_obs.data();
    for (int k = 0; k < l.count; ++k) rsba::ResectBlock(a, l.which == rsba::kRigStartTime ? rsba::RESECT_TIME : rsba::RESECT_CAMERA, a.blocks[k], lanes);
  }
  // a block without a fit keeps its bits, the markers always do
  for (size_t b = 0; b < nb + (size_t)M; ++b)
    if (b >= nb || status[b] > rsba::BLOCK_ITERATION_CAP) Expect(memcmp(&params[6 * b], &before[6 * b], 48) == 0, "kept bits", (int)b);
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
  rsba::RigStartPlan p;
  // empty problems
  Expect(rsba::PlanRigStart(0, 0, 0, 0, nullptr, nullptr, nullptr, 2, false, &p) && p.launches.empty() && p.blocks.empty() && p.buffers.total % 8 == 0, "nothing at all", 0);
  CheckPlan(p, {}, {}, 2, false, 100);
  Expect(rsba::PlanRigStart(3, 4, 2, 0, nullptr, nullptr, nullptr, 1, true, &p) && p.launches.empty(), "no observations", 1);
  CheckPlan(p, {}, {}, 1, true, 101);
  Expect(p.unreachable_times.size() == 4 && p.unreachable_cameras.size() == 2 && p.given[0] == 1, "no observations: all but the base camera unreachable", 1);
  // refused
  const int32_t c1[2] = {0, 3}, t1[2] = {0, 1}, tneg[2] = {0, -1};
  Expect(!rsba::PlanRigStart(3, 2, 1, 2, c1, t1, nullptr, 0, false, &p), "camera index out of range", 2);
  Expect(!rsba::PlanRigStart(4, 1, 1, 2, c1, t1, nullptr, 0, false, &p), "time index out of range", 3);
  Expect(!rsba::PlanRigStart(4, 2, 1, 2, c1, tneg, nullptr, 0, false, &p), "negative time index", 4);
  Expect(!rsba::PlanRigStart(4, 2, 1, 2, c1, t1, nullptr, -1, false, &p), "negative sweeps", 5);
  Expect(!rsba::PlanRigStart(4, 2, 1, 2, nullptr, t1, nullptr, 0, false, &p), "null indices", 6);
  Expect(!rsba::PlanRigStart(4, 2, 1, (int64_t)1 << 31, c1, t1, nullptr, 0, false, &p), "too many observations", 7);
  Expect(!rsba::PlanRigStart(4, 2, 1, 2, c1, t1, nullptr, 0, false, nullptr), "null plan", 8);
  Expect(rsba::PlanRigStart(4, 2, 1, 2, c1, t1, nullptr, 0, false, &p) && p.num_rounds == 1, "the same arguments in range", 9);
}

}  // namespace

int main(int argc, char** argv) {
  int rc = 0;
  if (argc == 3 && std::string(argv[1]) == "plan") rc = Plan(argv[2]);
  else if (argc == 3 && std::string(argv[1]) == "fit") rc = Fit(argv[2]);
  else if (argc == 1) Builtin();
  else { fprintf(stderr, "usage: rig_start_plan_driver [plan FILE | fit FILE]\n"); return 2; }
  if (rc) return rc;
  if (g_fail) { fprintf(stderr, "rig start driver: %d failures\n", g_fail); return 1; }
  fprintf(stderr, "rig start driver: ok\n");
  return 0;
}
